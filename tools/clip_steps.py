"""Step time of an optimizer with clipvalue / clipnorm / global_clipnorm against the unclipped
steps, in one process with the variants interleaved (device events on the trainer's stream,
median over the samples; every sample is one epoch of `steps` steps after an untimed begin_epoch).

  step, per-step graphs : run_steps_allreduce(steps, identity): [fwd+bwd -> G] graph, apply graph
                          (unclipped: the materialised-gradient step as it was; clipped: + clip.hip)
  apply graph alone     : the captured apply (update + counter advance; clipped: + partial sums, scales)
  step, chunk graph     : run_steps(steps): one graph replay per GRAPH_CHUNK steps (the clipped
                          training path; unclipped with persist=0: the fused row-chain / grouped step)
  persistent            : run_steps(steps) on the persistent plan (MNIST shape only)

  python tools/clip_steps.py mnist|wide [samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import elephas_amd  # noqa: E402,F401
import torch  # noqa: E402

SHAPES = {
    # name: dims, dropout, policy, R, B, steps per sample (= one epoch)
    "mnist": ((784, 128, 128, 10), 0.2, "float32", 8, 64, 64),
    "wide": ((4096, 4096, 4096, 1000), 0.0, "mixed_bfloat16", 1, 1024, 16),
}
CLIPS = {"none": {}, "clipvalue": dict(clipvalue=0.01), "clipnorm": dict(clipnorm=1.0),
         "global_clipnorm": dict(global_clipnorm=1.0)}


def build(dims, dropout, clip):
    from elephas_amd.models import Sequential, Dense, Dropout, initializers
    from elephas_amd.models.optimizers import SGD
    initializers.set_seed(1)
    m = Sequential()
    for i, h in enumerate(dims[1:-1]):
        m.add(Dense(h, activation="relu", **({"input_dim": dims[0]} if i == 0 else {})))
        if dropout:
            m.add(Dropout(dropout))
    m.add(Dense(dims[-1], activation="softmax"))
    m.compile(SGD(0.01, **clip), "categorical_crossentropy", ["acc"])
    return m


def main():
    shape = sys.argv[1] if len(sys.argv) > 1 else "mnist"
    samples = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    dims, dropout, policy, R, B, steps = SHAPES[shape]
    from elephas_amd import config
    from elephas_amd.ops.plan import build_plan
    from elephas_amd.ops.native_engine import NativeTrainer
    config.set_policy(policy)
    rng = np.random.default_rng(0)
    n = steps * B
    xs = [rng.random((n, dims[0]), dtype=np.float32) for _ in range(R)]
    ys = [np.eye(dims[-1], dtype=np.float32)[rng.integers(0, dims[-1], n)] for _ in range(R)]

    def trainer(clip, persist):
        m = build(dims, dropout, CLIPS[clip])
        t = NativeTrainer(m, build_plan(m), R, B, torch.device("cuda"), seed=7, persist=persist)
        t.set_data(xs, ys, 0.0, shuffle=True)
        return t

    ident = lambda G: None
    variants = {}   # name -> (trainer, run)
    for clip in CLIPS:
        t = trainer(clip, 0)
        variants[f"{clip}: step, per-step graphs"] = (t, lambda t=t: t.run_steps_allreduce(steps, ident, use_graph=True))
        variants[f"{clip}: apply graph alone"] = (t, lambda t=t: [t.exe.replay(t._graph(1, 2), t.s) for _ in range(steps)])
        variants[f"{clip}: step, chunk graph"] = (t, lambda t=t: t.run_steps(steps, use_graph=True))
        print(f"{clip}: {t.plan_name()}", flush=True)
    if shape == "mnist":
        t = trainer("none", None)
        assert t.exe.persistent(), t.plan_reason
        variants["none: persistent"] = (t, lambda t=t: t.run_steps(steps))
        print(f"persistent: {t.plan_name()}", flush=True)

    def sample(t, run):
        t.begin_epoch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(t.stream)
        run()
        e1.record(t.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps   # us per step

    for _ in range(3):   # warmup: captures every graph, loads every code object
        for t, run in variants.values():
            sample(t, run)
    res = {k: [] for k in variants}
    for _ in range(samples):
        for k, (t, run) in variants.items():
            res[k].append(sample(t, run))
    nparams = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    print(f"shape {shape}: {'-'.join(map(str, dims))}, {policy}, {R} x {B}, {nparams} parameters per replica; "
          f"{samples} samples of {steps} steps, interleaved; us per step")
    for k, v in res.items():
        v = np.array(v)
        print(f"  {k:42s} median {np.median(v):9.2f}   p10 {np.percentile(v, 10):9.2f}   p90 {np.percentile(v, 90):9.2f}")
    for t, _ in variants.values():
        assert np.isfinite(t.get_weights_flat()).all()


if __name__ == "__main__":
    main()
