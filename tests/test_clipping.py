"""Optimizer gradient clipping (Keras 2.10 optimizer_v2 ``clipvalue`` / ``clipnorm`` /
``global_clipnorm``) on the torch engine: the transform against closed forms in numpy fp64,
the optimizer contract (validation, attributes, configs, HDF5), and training through
TorchTrainer / SparkModel on the CPU."""
import numpy as np
import pytest

from elephas_amd.models import Dense, Sequential
from elephas_amd.models import optimizers as O
from elephas_amd.models.optimizers import SGD, Adam

import torch  # noqa: E402  (after elephas_amd, which sets the HIP runtime's environment)


def clip_np(grads, clipvalue=None, clipnorm=None, global_clipnorm=None):
    """Rules 1-4 written out in fp64: clipvalue, then clipnorm per variable, then global_clipnorm."""
    g = [np.asarray(x, np.float64) for x in grads]
    if clipvalue is not None:
        g = [np.minimum(np.maximum(x, -clipvalue), clipvalue) for x in g]
    if clipnorm is not None:
        g = [x * clipnorm / max(np.sqrt((x * x).sum()), clipnorm) for x in g]
    if global_clipnorm is not None:
        n = np.sqrt(sum((x * x).sum() for x in g))
        g = [x * global_clipnorm / max(n, global_clipnorm) for x in g]
    return g


def _apply(opt, grads):
    out = opt.clip_gradients([torch.tensor(np.asarray(g, np.float32)) for g in grads])
    return [o.numpy() for o in out]


GRADS = [np.array([[3.0, -0.1], [0.2, -4.0]]), np.array([0.3, -0.4]), np.array([[1e-3, 2e-3, -1e-3]])]


def test_clipvalue_clamps_every_element():
    out = _apply(SGD(0.1, clipvalue=0.25), GRADS)
    assert np.allclose(out[0], [[0.25, -0.1], [0.2, -0.25]], rtol=1e-6)
    assert np.allclose(out[1], [0.25, -0.25], rtol=1e-6)
    assert np.allclose(out[2], GRADS[2], rtol=1e-6)


def test_clipnorm_is_per_variable_on_both_sides_of_the_threshold():
    c = 1.0   # ||g0|| ~ 5.0 and ||g1|| = 0.5, ||g2|| ~ 2.4e-3: one variable clipped, two untouched
    norms = [np.sqrt((g * g).sum()) for g in GRADS]
    assert norms[0] > c > norms[1] > norms[2]
    out = _apply(SGD(0.1, clipnorm=c), GRADS)
    assert np.allclose(out[0], GRADS[0] * c / norms[0], rtol=1e-6)
    assert np.isclose(np.sqrt((out[0].astype(np.float64) ** 2).sum()), c, rtol=1e-6)
    assert np.allclose(out[1], GRADS[1], rtol=1e-6) and np.allclose(out[2], GRADS[2], rtol=1e-6)
    for o, e in zip(out, clip_np(GRADS, clipnorm=c)):
        assert np.allclose(o, e, rtol=1e-6, atol=0)


@pytest.mark.parametrize("c,clipped", [(2.0, True), (10.0, False)])
def test_global_clipnorm_scales_all_variables_by_one_factor(c, clipped):
    n = np.sqrt(sum((g * g).sum() for g in GRADS))
    assert (n > c) == clipped
    out = _apply(Adam(global_clipnorm=c), GRADS)
    f = c / n if clipped else 1.0
    for o, g in zip(out, GRADS):
        assert np.allclose(o, g * f, rtol=1e-6, atol=0)
    if clipped:
        assert np.isclose(np.sqrt(sum((o.astype(np.float64) ** 2).sum() for o in out)), c, rtol=1e-6)


@pytest.mark.parametrize("kw", [dict(clipvalue=1.0, clipnorm=1.0), dict(clipvalue=1.0, global_clipnorm=1.0)])
def test_order_is_clipvalue_then_norm(kw):
    g = [np.array([3.0, 0.1]), np.array([0.5])]
    cv = kw["clipvalue"]
    norm_kw = {k: v for k, v in kw.items() if k != "clipvalue"}
    right = clip_np(g, **kw)
    wrong = clip_np(clip_np(g, **norm_kw), clipvalue=cv)   # the norm first, then the clamp
    assert np.abs(right[0] - wrong[0]).max() > 1e-2        # the input tells the two orders apart
    out = _apply(SGD(0.1, **kw), g)
    for o, e in zip(out, right):
        assert np.allclose(o, e, rtol=1e-6, atol=0)


def test_no_clip_arguments_returns_the_gradients_untouched():
    gs = [torch.ones(3), torch.zeros(2, 2)]
    assert SGD(0.1).clip_gradients(gs) is gs


def test_validation():
    with pytest.raises(ValueError):
        SGD(0.1, clipnorm=1.0, global_clipnorm=1.0)
    for k in ("clipnorm", "clipvalue", "global_clipnorm"):
        with pytest.raises(ValueError):
            Adam(**{k: -0.5})
        assert getattr(O.RMSprop(**{k: None}), k) is None
        assert k not in O.RMSprop(**{k: None}).get_config()


def test_attributes_and_config():
    plain = SGD(0.1)
    assert plain.clipnorm is None and plain.clipvalue is None and plain.global_clipnorm is None
    assert not {"clipnorm", "clipvalue", "global_clipnorm"} & set(plain.get_config())
    assert plain.clip_args() == (None, None, None)
    with pytest.raises(AttributeError):
        plain.no_such_hyper
    opt = SGD(0.1, momentum=0.9, clipvalue=0.5, clipnorm=2)
    assert opt.clipvalue == 0.5 and opt.clipnorm == 2.0 and opt.global_clipnorm is None
    assert opt.clip_args() == (0.5, 2.0, None)
    cfg = opt.get_config()
    assert cfg["clipvalue"] == 0.5 and cfg["clipnorm"] == 2.0 and "global_clipnorm" not in cfg
    # the native hyper-parameter dict is copied key by key into OptParams: no clip keys there
    assert not any("clip" in k for k in opt.native()[1])


@pytest.mark.parametrize("cls", [SGD, O.RMSprop, Adam, O.Adagrad, O.Adamax, O.Adadelta, O.Nadam])
def test_serialize_deserialize_clone_keep_the_values(cls):
    opt = cls(clipvalue=0.5, global_clipnorm=3.0)
    for o in (O.deserialize(O.serialize(opt)), O.clone(opt), O.get(O.serialize(opt))):
        assert type(o) is cls
        assert o.clip_args() == (0.5, None, 3.0)


def _mlp(opt, in_dim=6, hidden=5, out=3):
    from elephas_amd.models import initializers
    initializers.set_seed(11)
    m = Sequential()
    m.add(Dense(hidden, activation="tanh", input_dim=in_dim))
    m.add(Dense(out, activation="softmax"))
    m.compile(opt, "categorical_crossentropy", ["acc"])
    return m


def _data(n, in_dim=6, out=3, seed=0, scale=3.0):
    rng = np.random.default_rng(seed)
    x = (scale * rng.normal(size=(n, in_dim))).astype(np.float32)
    y = np.eye(out, dtype=np.float32)[rng.integers(0, out, n)]
    return x, y


def test_json_and_hdf5_round_trip(tmp_path):
    from elephas_amd.models import load_model, model_from_json
    m = _mlp(SGD(0.05, momentum=0.9, clipnorm=1.5, clipvalue=0.25))
    assert model_from_json(m.to_json()).to_json() == m.to_json()
    p = str(tmp_path / "clip.h5")
    m.save(p)
    opt = load_model(p).optimizer
    assert type(opt) is SGD and opt.clip_args() == (0.25, 1.5, None) and opt.momentum == 0.9


# ---- training: an independent loop (torch autograd + the formulas above) ---------------------
def _grads(ws, x, y):
    ps = [torch.tensor(w, requires_grad=True) for w in ws]
    h = torch.tanh(torch.tensor(x) @ ps[0] + ps[1])
    logp = torch.log_softmax(h @ ps[2] + ps[3], -1)
    loss = -(torch.tensor(y) * logp).sum(-1).mean()
    return [g.numpy().astype(np.float64) for g in torch.autograd.grad(loss, ps)]


def _momentum_step(ws, vs, gs, lr, mom):
    for w, v, g in zip(ws, vs, gs):
        v *= mom
        v -= lr * g
        w += v.astype(np.float32)


def _flat(ws):
    return np.concatenate([np.asarray(w).reshape(-1) for w in ws])


def _reference_run(w0, x, y, B, steps, lr, mom, clip):
    ws = [w.copy() for w in w0]
    vs = [np.zeros(w.shape, np.float64) for w in w0]
    for s in range(steps):
        gs = clip_np(_grads(ws, x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]), **clip)
        _momentum_step(ws, vs, gs, lr, mom)
    return _flat(ws)


def _median_norm(w0, x, y, B):
    g = _grads(w0, x[:B], y[:B])
    return float(np.median([np.sqrt((v * v).sum()) for v in g])), float(np.sqrt(sum((v * v).sum() for v in g))), g


@pytest.mark.parametrize("mode", ["clipvalue", "clipnorm", "global_clipnorm", "clipvalue+clipnorm",
                                  "clipvalue+global_clipnorm"])
def test_torch_trainer_three_steps_match_independent_loop(mode):
    from elephas_amd.ops.plan import build_plan
    from elephas_amd.ops.torch_engine import TorchTrainer
    B, steps, lr, mom = 8, 3, 0.05, 0.9
    x, y = _data(B * steps)
    w0 = _mlp(SGD(lr)).get_weights()
    med, glob, g0 = _median_norm(w0, x, y, B)
    vals = dict(clipvalue=float(np.percentile(np.abs(_flat(g0)), 90)), clipnorm=med, global_clipnorm=0.5 * glob)
    clip = {k: vals[k] for k in mode.split("+")}
    runs = {}
    for name, kw in (("clipped", clip), ("plain", {})):
        m = _mlp(SGD(lr, momentum=mom, **kw))
        t = TorchTrainer(m, build_plan(m), 1, B, "cpu", seed=0)
        t.set_data([x], [y], 0.0, shuffle=False)
        t.fit(1)
        runs[name] = t.get_weights_flat()[0]
    want = _reference_run(w0, x, y, B, steps, lr, mom, clip)
    assert np.abs(runs["clipped"] - want).max() / np.abs(want).max() < 1e-6
    step = np.abs(runs["plain"] - _flat(w0)).max()
    assert np.abs(runs["clipped"] - runs["plain"]).max() > 0.1 * step   # the clip did change the training


def test_fit_allreduce_clips_after_the_mean():
    from elephas_amd.ops.plan import build_plan
    from elephas_amd.ops.torch_engine import TorchTrainer
    B, lr, mom = 8, 0.05, 0.9
    xa, ya = _data(B, seed=1)
    xb, yb = _data(B, seed=2, scale=0.3)   # a second shard with a much smaller gradient
    w0 = _mlp(SGD(lr)).get_weights()
    ga, gb = _grads(w0, xa, ya), _grads(w0, xb, yb)
    na, nb = (np.sqrt(sum((v * v).sum() for v in g)) for g in (ga, gb))
    mean = [(a + b) / 2 for a, b in zip(ga, gb)]
    nm = np.sqrt(sum((v * v).sum() for v in mean))
    c = float(0.8 * nm)
    assert nm > c and max(na, nb) > c   # the mean is clipped, and so would a replica's own gradient be
    after = clip_np(mean, global_clipnorm=c)
    before = [(a + b) / 2 for a, b in zip(clip_np(ga, global_clipnorm=c), clip_np(gb, global_clipnorm=c))]
    assert np.abs(_flat(after) - _flat(before)).max() > 0.05 * np.abs(_flat(after)).max()
    m = _mlp(SGD(lr, momentum=mom, global_clipnorm=c))
    t = TorchTrainer(m, build_plan(m), 2, B, "cpu", seed=0)
    t.set_data([xa, xb], [ya, yb], 0.0, shuffle=False)

    def mean_allreduce(G):
        G.copy_(G.mean(0, keepdim=True).expand_as(G))

    t.fit(1, allreduce=mean_allreduce)
    got = t.get_weights_flat()
    want = _flat(w0) - lr * _flat(after)
    wrong = _flat(w0) - lr * _flat(before)
    assert np.array_equal(got[0], got[1])
    assert np.abs(got[0] - want).max() < 1e-6 * np.abs(want).max()
    assert np.abs(got[0] - wrong).max() > 100 * np.abs(got[0] - want).max()


def test_spark_model_sync_fit_ships_the_clip_to_the_workers(spark_context, monkeypatch):
    from elephas_amd import config
    from elephas_amd.ops import engine
    from elephas_amd.spark_model import SparkModel
    config.set_engine("torch")
    built = []
    make = engine.make_trainer

    def recording(*a, **kw):
        t = make(*a, **kw)
        built.append(t)
        return t

    monkeypatch.setattr(engine, "make_trainer", recording)
    try:
        x, y = _data(80)
        m = _mlp(SGD(0.05, clipnorm=0.125))
        w0 = _flat(m.get_weights())
        sm = SparkModel(m, mode="synchronous")
        sm.fit(spark_context.parallelize(list(zip(x, y)), 2), epochs=2, batch_size=8, verbose=0, shuffle=False)
        assert sm.master_optimizer["config"]["clipnorm"] == 0.125
        w1 = _flat(sm.master_network.get_weights())
        assert np.isfinite(w1).all() and not np.array_equal(w0, w1)
        opts = [o for t in built for o in getattr(t, "opts", [])]
        assert len(opts) >= 2 and all(o.clipnorm == 0.125 for o in opts)
        # every step moved every variable by at most lr * clipnorm: 2 epochs x 5 steps of lr 0.05
        assert np.abs(w1 - w0).max() <= 10 * 0.05 * 0.125 * (1 + 1e-5)
    finally:
        config.set_engine("auto")
