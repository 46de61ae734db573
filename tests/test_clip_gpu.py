"""Optimizer gradient clipping on the native engine (GPU only): the clip kernels
(csrc/kernels/clip.hip: fp64 partial sums of squares per chunk, then scales) against numpy
fp64, and training with clipvalue / clipnorm / global_clipnorm against the torch engine."""
import numpy as np
import pytest

import elephas_amd  # noqa: F401  (before torch: it sets the HIP runtime's environment)
import torch

pytestmark = pytest.mark.gpu

DIMS = (130, 200, 72, 9)


def _mlp(dims, bias=True, seed=77):
    from elephas_amd.models import Sequential, Dense, initializers
    initializers.set_seed(seed)   # the initial weights must not depend on which tests ran before
    m = Sequential()
    m.add(Dense(dims[1], input_dim=dims[0], activation="relu", use_bias=bias))
    for h in dims[2:-1]:
        m.add(Dense(h, activation="relu", use_bias=bias))
    m.add(Dense(dims[-1], activation="softmax", use_bias=bias))
    return m


def _data(n, d, k, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, d)).astype(np.float32), np.eye(k, dtype=np.float32)[rng.integers(0, k, n)]


def _flat(ws):
    return np.concatenate([np.asarray(w).reshape(-1) for w in ws])


# ---------------------------------------------------------------- 1. the kernels
LAYOUTS = {
    # variables of 130-200-72-9 with biases: n = 41329 (odd), so replica 1's row starts 1 mod 4
    "biases_R2": ([26000, 200, 14400, 72, 648, 9], 2),
    # 97-127-5 without biases: an odd variable count, the second variable starts 3 mod 4
    "nobias_R3": ([12319, 635], 3),
}
_G = {}


def _layout(name):
    """(G on the device, G on the host, [(offset, length)], R), built once per layout."""
    if name not in _G:
        sizes, R = LAYOUTS[name]
        n = sum(sizes)
        rng = np.random.default_rng(len(sizes))
        mags = np.logspace(-3, 2, len(sizes))
        G = np.empty((R, n), np.float32)
        for r in range(R):
            off = 0
            for t, sz in enumerate(sizes):   # per-variable magnitudes 1e-3 .. 1e2, rotated per replica
                G[r, off:off + sz] = rng.normal(size=sz) * mags[(t + r) % len(sizes)]
                off += sz
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        _G[name] = (torch.tensor(G, device="cuda"), G, [(int(o), int(s)) for o, s in zip(offs, sizes)], R)
    return _G[name]


def _scales_np(G, vars_, gs, cv, cn, gn):
    out = np.empty((G.shape[0], len(vars_)))
    for r in range(G.shape[0]):
        v = G[r].astype(np.float64) * gs
        if cv is not None:
            v = np.clip(v, -cv, cv)
        ss = np.array([(v[o:o + n] ** 2).sum() for o, n in vars_])
        if gn is not None:
            out[r] = gn / max(np.sqrt(ss.sum()), gn)
        else:
            out[r] = cn / np.maximum(np.sqrt(ss), cn)
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("mode", ["clipnorm", "global_clipnorm", "clipvalue+clipnorm", "clipvalue+global_clipnorm"])
def test_clip_kernels_match_numpy_fp64(layout, mode):
    from elephas_amd.ops import native
    C = native.require()
    Gd, Gh, vars_, R = _layout(layout)
    gs = 0.5
    cv = 0.75 if "clipvalue" in mode else None
    # thresholds from replica 0 (after the clamp): the median variable norm, half the global norm
    v0 = Gh[0].astype(np.float64) * gs
    if cv is not None:
        v0 = np.clip(v0, -cv, cv)
    norms0 = np.sqrt([(v0[o:o + n] ** 2).sum() for o, n in vars_])
    cn = float(np.median(norms0)) if mode.endswith("clipnorm") and "global" not in mode else None
    gn = float(0.5 * np.sqrt((norms0 ** 2).sum())) if "global" in mode else None
    want = _scales_np(Gh, vars_, gs, cv, cn, gn)
    assert (want < 1).any() and ((want == 1).any() or gn is not None)   # both sides of the threshold
    outs = []
    for _ in range(2):
        sc = torch.full((R, C.CLIP_MAX_VAR), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        C.clip_scales(Gd.data_ptr(), Gd.shape[1], R, vars_, gs, cv, cn, gn, sc.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(sc.cpu().numpy())
    got = outs[0][:, :len(vars_)].astype(np.float64)
    # fp32 products summed in fp64: the norm is exact to a few fp32 ulps
    rel = np.abs(got - want) / want
    print(layout, mode, "max rel err", rel.max())
    assert rel.max() < 1e-6, rel
    assert outs[0].tobytes() == outs[1].tobytes()   # a second call: bit-identical


# ---------------------------------------------------------------- 2. training vs the torch engine
B, STEPS = 32, 6
_CAL = {}
_PLAIN = {}


def _shards():
    x, y = _data(2 * B * STEPS, DIMS[0], DIMS[-1], seed=4)
    return [x[:B * STEPS], x[B * STEPS:]], [y[:B * STEPS], y[B * STEPS:]]


def _trainers(optim, policy, xs, ys, R=2, sync=False):
    from elephas_amd import config
    from elephas_amd.ops.plan import build_plan
    from elephas_amd.ops.native_engine import NativeTrainer
    from elephas_amd.ops.torch_engine import TorchTrainer
    config.set_policy(policy)
    model = _mlp(DIMS)
    model.compile(optim, "categorical_crossentropy", ["acc"])
    plan = build_plan(model)
    nat = NativeTrainer(model, plan, R, B, torch.device("cuda"), seed=3, sync=sync)
    ref = TorchTrainer(model, plan, R, B, torch.device("cuda"), seed=3)
    for t in (nat, ref):
        t.set_data(xs, ys, 0.0, shuffle=False)
    return model, nat, ref


def _calibration():
    """Thresholds from the reference's step-0 gradient of replica 0 (computed once)."""
    if not _CAL:
        from elephas_amd.models import optimizers as O
        xs, ys = _shards()
        model, nat, ref = _trainers(O.SGD(0.05), "float32", xs, ys)
        g = ref._grads(0, ref.xs[0][:B], ref.ys[0][:B])[0].double().cpu().numpy()
        sizes = [w.size for w in model.get_weights()]
        norms = np.sqrt([(v ** 2).sum() for v in np.split(g, np.cumsum(sizes)[:-1])])
        _CAL.update(clipnorm=float(np.median(norms)), global_clipnorm=float(0.5 * np.sqrt((g ** 2).sum())),
                    clipvalue=float(np.percentile(np.abs(g), 90)), norms=norms)
    return _CAL


def _plain_native(policy, optim_factory):
    """The unclipped native run of the same optimizer (once per policy)."""
    if policy not in _PLAIN:
        xs, ys = _shards()
        _, nat, _ = _trainers(optim_factory(), policy, xs, ys)
        nat.fit(1)
        _PLAIN[policy] = nat.get_weights_flat()
    return _PLAIN[policy]


def _compare(wn, wr, w0, policy, family):
    """The criteria of tests/test_native_gpu.py::test_one_step_matches_reference."""
    if policy == "float32" and family == "sgd":
        err, tol = np.abs(wn - wr).max() / np.abs(wr - w0).max(), 1e-3
    elif policy == "float32":
        err, tol = np.abs(wn - wr).mean() / np.abs(wr - w0).mean(), 1e-2
    else:
        err, tol = np.abs(wn - wr).mean() / np.abs(wr - w0).mean(), 0.15
    print(policy, family, "err", err, "tol", tol)
    assert err < tol, err


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
@pytest.mark.parametrize("case", ["sgd:clipvalue", "sgd:clipnorm", "sgd:global_clipnorm", "sgd:clipvalue+clipnorm",
                                  "sgd:clipvalue+global_clipnorm", "adam:clipvalue"])
def test_clipped_training_matches_reference(policy, case):
    from elephas_amd import config
    from elephas_amd.models import optimizers as O
    cal = _calibration()
    family, mode = case.split(":")
    clip = {k: cal[k] for k in mode.split("+")}
    if "clipnorm" in clip:   # some variables clipped, some not
        assert (cal["norms"] > clip["clipnorm"]).any() and (cal["norms"] < clip["clipnorm"]).any()
    make = (lambda **kw: O.SGD(0.05, momentum=0.9, **kw)) if family == "sgd" else (lambda **kw: O.Adam(0.002, **kw))
    xs, ys = _shards()
    model, nat, ref = _trainers(make(**clip), policy, xs, ys)
    assert not nat.exe.persistent()
    w0 = np.stack([_flat(model.get_weights())] * 2)
    nat.fit(1)
    ref.fit(1)
    wn, wr = nat.get_weights_flat(), ref.get_weights_flat()
    assert np.isfinite(wn).all()
    try:
        _compare(wn, wr, w0, policy, family)
        if family == "sgd":
            # the clip reached the update: far from the unclipped native run
            plain = _plain_native(policy, make)
            assert np.abs(wn - plain).max() > 0.1 * np.abs(wr - w0).max()
    finally:
        config.set_policy("float32")


# ---------------------------------------------------------------- 3. ragged shards
def test_partial_batches_and_a_replica_out_of_batches():
    from elephas_amd.models import optimizers as O
    x, y = _data(170, DIMS[0], DIMS[-1], seed=5)
    xs, ys = [x[:100], x[100:]], [y[:100], y[100:]]   # 4 batches (last of 4 rows) and 3 (last of 6)
    model, nat, ref = _trainers(O.SGD(0.05, momentum=0.9, global_clipnorm=_calibration()["global_clipnorm"]),
                                "float32", xs, ys)
    w0 = np.stack([_flat(model.get_weights())] * 2)
    nat.fit(1)
    ref.fit(1)
    assert list(nat.iterations()) == [4, 3]
    _compare(nat.get_weights_flat(), ref.get_weights_flat(), w0, "float32", "sgd")


# ---------------------------------------------------------------- 4. clipping after the aggregation
def test_sync_replicas_clip_the_mean_gradient():
    from elephas_amd.models import optimizers as O
    xs, ys = _shards()
    model, nat, ref = _trainers(O.SGD(0.05, momentum=0.9, global_clipnorm=_calibration()["global_clipnorm"]),
                                "float32", xs, ys, sync=True)
    w0 = np.stack([_flat(model.get_weights())] * 2)
    nat.fit(1)
    ref.fit(1, allreduce=lambda G: G.copy_(G.mean(0, keepdim=True).expand_as(G)))
    wn, wr = nat.get_weights_flat(), ref.get_weights_flat()
    assert np.array_equal(wn[0], wn[1])
    _compare(wn, wr, w0, "float32", "sgd")


# ---------------------------------------------------------------- 5. replay and determinism
def test_graph_replay_equals_eager_and_runs_repeat_bit_for_bit():
    from elephas_amd import config
    from elephas_amd.models import optimizers as O
    from elephas_amd.ops.plan import build_plan
    from elephas_amd.ops.native_engine import NativeTrainer
    config.set_policy("float32")
    cal = _calibration()
    model = _mlp(DIMS)
    model.compile(O.SGD(0.05, momentum=0.9, clipvalue=cal["clipvalue"], clipnorm=cal["clipnorm"]),
                  "categorical_crossentropy")
    x, y = _data(400, DIMS[0], DIMS[-1], seed=4)
    ws = []
    for graph in (True, False, True):
        t = NativeTrainer(model, build_plan(model), 2, B, torch.device("cuda"), seed=3)
        t.set_data([x, x[::-1].copy()], [y, y[::-1].copy()], 0.0, shuffle=False)
        t.begin_epoch()
        t.run_steps(12, use_graph=graph)
        ws.append(t.get_weights_flat())
        assert list(t.iterations()) == [12, 12]
    assert np.array_equal(ws[0], ws[1])   # one replayed graph == eager launches
    assert np.array_equal(ws[0], ws[2])   # and the same bits again
    assert not np.array_equal(ws[0][0], ws[0][1])


# ---------------------------------------------------------------- 6. routing
def test_clipping_takes_the_materialised_gradient_step():
    from elephas_amd import config
    from elephas_amd.models import optimizers as O
    from elephas_amd.ops.plan import build_plan
    from elephas_amd.ops.native_engine import NativeTrainer
    config.set_policy("float32")
    for kw, persistent in ((dict(clipnorm=1.0), False), ({}, True)):
        model = _mlp((784, 128, 128, 10))
        model.compile(O.SGD(0.1, **kw), "categorical_crossentropy", ["acc"])
        t = NativeTrainer(model, build_plan(model), 2, 64, torch.device("cuda"))
        assert bool(t.exe.persistent()) == persistent
        if not persistent:
            assert "clipping" in t.exe.plan_reason() and "clipping" in t.plan_reason
        else:
            assert t.exe.plan_reason() == ""


# ---------------------------------------------------------------- 7. SparkModel, native vs torch
@pytest.mark.parametrize("gran", ["fit", "batch"])
def test_spark_model_clipnorm_native_vs_torch(gran, tmp_path):
    from elephas_amd import config
    from elephas_amd.data import SparkContext
    from elephas_amd.models.optimizers import SGD
    from elephas_amd.spark_model import SparkModel
    config.set_policy("float32")
    x, y = _data(600, 40, 5, seed=2)
    ws = []
    try:
        for engine in ("native", "torch"):
            config.set_engine(engine)
            m = _mlp((40, 64, 32, 5), seed=3)
            m.compile(SGD(0.05, momentum=0.9, clipnorm=0.02), "categorical_crossentropy", ["acc"])
            sm = SparkModel(m, mode="synchronous", sync_granularity=gran)
            rdd = SparkContext.getOrCreate().parallelize(list(zip(x, y)), 3)
            sm.fit(rdd, epochs=3, batch_size=32, verbose=0, shuffle=False, checkpoint_dir=str(tmp_path / engine))
            ws.append(_flat(sm.master_network.get_weights()))
    finally:
        config.set_engine("auto")
    assert np.abs(ws[0] - ws[1]).max() < 2e-4, np.abs(ws[0] - ws[1]).max()


# ---------------------------------------------------------------- 8. parameter-server workers
def test_async_batch_workers_clip_on_the_host_side_path():
    """frequency='batch' with the device parameter server: a clipping optimizer's plan is not
    persistent, so the in-launch push / pull hook is not offered and the workers run their
    captured host-side rounds -- every step of every worker clipped.  Plain SGD moves a variable
    by at most lr * clipnorm per step; unclipped, this model's first steps move it ~100x as far."""
    from elephas_amd import config
    from elephas_amd.data import SparkContext
    from elephas_amd.models.optimizers import SGD
    from elephas_amd.spark_model import SparkModel
    from elephas_amd.utils.rdd_utils import to_simple_rdd
    config.set_policy("float32")
    lr, c, bs, epochs = 0.1, 1e-3, 64, 2
    x, y = _data(1000, 784, 10, seed=8)
    model = _mlp((784, 128, 128, 10))
    model.compile(SGD(lr, clipnorm=c), "categorical_crossentropy", ["acc"])
    w0 = [w.copy() for w in model.get_weights()]
    sm = SparkModel(model, mode="asynchronous", frequency="batch", parameter_server_mode="device", num_workers=2)
    sm.fit(to_simple_rdd(SparkContext.getOrCreate(), x, y), epochs=epochs, batch_size=bs, verbose=0)
    w1 = sm.master_network.get_weights()
    steps = epochs * (1000 // bs + 8)   # every worker's steps land in the server (<= 8 partial last batches)
    moved = [float(np.sqrt(((a - b).astype(np.float64) ** 2).sum())) for a, b in zip(w1, w0)]
    print("moved", moved, "bound", steps * lr * c)
    assert all(np.isfinite(w).all() for w in w1) and min(moved) > 0
    assert max(moved) <= steps * lr * c * (1 + 1e-4)
