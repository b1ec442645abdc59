"""GPU tests of Keras 2.11's SGD, RMSprop, Adagrad, Adamax, amsgrad Adam, AdamW and of the per-step learning-rate schedules on the
k_opt.hip kernels, against the NumPy restatement of tests/keras_opt_ref.py (formulas restated from Keras 2.11, not pinned by a
TensorFlow run): six teacher-forced steps on a gradient written to the device, in the eager form (k_opt), in a captured graph of two
steps replayed three times (k_opt_dev: the second step of every replay takes its iteration count, and with it the schedule's learning
rate, from the device-side counter) and, on the net's own gradient, in the fused tail (k_reduce_opt) against the flushed reduction +
k_opt; then fit() end to end.

The optimizer streams run over the context's whole parameter vector, whose length the net's configuration fixes and whose buffers the
allocator aligns to 16 bytes: a vector of 1 or 7 parameters or a misaligned start cannot be reached through the C ABI.  The nets are
the smallest cfg_ms ones whose P leaves a scalar tail of 1, 2 and 3 behind the 16-byte body, one of them with more than one block
(P > 1024); 1, 7 and 1031 are the batch sizes (the rows of the fused tail's reduction)."""
import ctypes as C

import numpy as np
import pytest

from tests import keras_opt_ref as K
from tests.cfgs import cfg_ms
from tests.test_gpu_parity import _make

pytestmark = pytest.mark.gpu

f32 = np.float32
NETS = {"p441": cfg_ms(), "p1535": cfg_ms(n=16, nst=12), "p414": cfg_ms(n=8, nst=5)}      # P % 4 = 1, 3, 2
BATCHES = (1, 7, 1031)
BAR = 2e-6                      # relative L2 per slot and for theta: the bar tests/test_gpu_optimizers.py holds for Adam and AdaBelief
MEASURED = {}


def _x(v):
    return float(f32(v))


def _opt(name):
    from nif_amd import optimizers as P
    S = P.schedules
    return {
        "sgd": lambda: P.SGD(1e-3),
        "sgd_momentum": lambda: P.SGD(1e-3, momentum=0.9),
        "sgd_nesterov": lambda: P.SGD(1e-3, momentum=0.9, nesterov=True),
        "rmsprop": lambda: P.RMSprop(),
        "rmsprop_momentum": lambda: P.RMSprop(momentum=0.5),
        "rmsprop_centered_momentum": lambda: P.RMSprop(momentum=0.5, centered=True),
        "adagrad": lambda: P.Adagrad(1e-2),
        "adamax": lambda: P.Adamax(),
        "adam_ams": lambda: P.Adam(amsgrad=True),
        "adamw": lambda: P.AdamW(weight_decay=1e-2),
        "adamw_ams": lambda: P.AdamW(weight_decay=1e-2, amsgrad=True),
        "sgd_momentum_exponential_staircase": lambda: P.SGD(S.ExponentialDecay(1e-3, 2, 0.5, staircase=True), momentum=0.9),
        "rmsprop_inverse_time": lambda: P.RMSprop(S.InverseTimeDecay(1e-3, 3, 0.5)),
        "adamax_cosine": lambda: P.Adamax(S.CosineDecay(1e-3, 4, alpha=0.1)),
        "adam_ams_polynomial_cycle": lambda: P.Adam(S.PolynomialDecay(1e-3, 2, 1e-4, power=2.0, cycle=True), amsgrad=True),
        "adagrad_exponential": lambda: P.Adagrad(S.ExponentialDecay(1e-2, 3, 0.7)),
        "adamw_polynomial": lambda: P.AdamW(S.PolynomialDecay(1e-3, 4, 1e-4, power=0.5), weight_decay=1e-2),
    }[name]()


VARIANTS = ["sgd", "sgd_momentum", "sgd_nesterov", "rmsprop", "rmsprop_momentum", "rmsprop_centered_momentum", "adagrad", "adamax",
            "adam_ams", "adamw", "adamw_ams", "sgd_momentum_exponential_staircase", "rmsprop_inverse_time", "adamax_cosine",
            "adam_ams_polynomial_cycle", "adagrad_exponential", "adamw_polynomial"]


def _layout(opt):
    from nif_amd.optimizers import slot_layout
    return slot_layout(opt)


def _gradients(P, seed):
    """three gradients for steps (1, 2), (3, 4), (5, 6): zeros, small and large magnitudes, and a sign change between them"""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(P) * 10.0 ** rng.uniform(-4, 1, P)).astype(f32)
    g[::5] = 0.0
    g2 = (-g * f32(0.5)).astype(f32)                       # every component changes its sign
    g3 = (g * rng.uniform(0.5, 2.0, P)).astype(f32)
    g3[1::7] = 0.0
    return [g, g2, g3]


def _put_grad(e, g):
    from nif_amd._lib import check
    buf = np.concatenate([g, [f32(0.5)]]).astype(f32)
    check(e.lib.nif_h2d(e.ctx, C.c_void_p(e.grad_dev_ptr()), buf.ctypes.data_as(C.c_void_p), buf.nbytes))


def _state(e):
    th = e.get_flat()
    m, v, t = e.get_opt_state()
    return th, m, v, e.get_opt_slot(2), t


def _engine(net, B=8):
    m_, model, spec, ws, x, y, sw = _make((NETS[net], B))
    return m_, m_._engine, x, y


def _eager(variant, net):
    """six steps by nif_opt_step_dev on a context whose slots are fresh (Adagrad's accumulator and the third slot are the library's to
    initialise); every step against the restatement applied to the GPU's previous state.  -> final state, worst relative L2"""
    opt = _opt(variant)
    o = opt.as_opt()
    keep, e, _, _ = _engine(net)
    gs = _gradients(e.n_params, 11)
    worst = {"theta": 0.0, "s0": 0.0, "s1": 0.0, "s2": 0.0}
    _, _, second, third = _layout(opt)
    for k in range(6):
        th, s0, s1, s2, t = _state(e)
        if k == 0 and o.kind == K.ADAGRAD:
            assert not s0.any()                            # still zero: the first step writes initial_accumulator_value
            s0 = np.full_like(s0, o.init_acc)
        g = gs[k // 2]
        _put_grad(e, g)
        e.opt_step_dev(o)
        after = _state(e)
        assert after[4] == t + 1 == k + 1
        want = K.update(o, t + 1, th, g, s0, s1, s2)
        used = [True, True, second, third]
        for nm, got, ref, on in zip(("theta", "s0", "s1", "s2"), after[:4], want, used):
            if on:
                worst[nm] = max(worst[nm], K.rel_l2(got, ref))
            else:
                assert not got.any(), (variant, nm)        # a slot the kind does not use is not touched
        assert np.all(np.isfinite(after[0]))
    return _state(e), worst


def _graph(variant, net):
    """the same six steps from a captured graph of two steps, replayed three times with a new gradient before each replay"""
    opt = _opt(variant)
    o = opt.as_opt()
    keep, e, _, _ = _engine(net)
    gs = _gradients(e.n_params, 11)
    z = np.zeros((e.n_params,), f32)
    e.set_opt_state(np.full_like(z, o.init_acc), z, 0)     # (a capture cannot initialise a slot: Model.fit does this as well)
    if _layout(opt)[3]:
        e.set_opt_slot(2, z)
    e.reserve(8)
    e.graph_begin()
    e.opt_step_dev(o)
    e.opt_step_dev(o)
    gid = e.graph_end()
    for k in range(3):
        _put_grad(e, gs[k])
        e.graph_launch_opt(gid, o)
    st = _state(e)
    e.graph_destroy(gid)
    return st


@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("variant", VARIANTS)
def test_eager_and_captured_steps_agree_bitwise_and_with_the_restatement(variant, net):
    """bars: theta and every slot within 2e-6 relative L2 of the restatement at each of the six steps; eager and captured bitwise equal.
    Measured worst over all 51 cases x 6 steps: 0 for theta and every slot, as Lion measures in tests/test_gpu_optimizers.py (the kernels
    run the restatement's float sequence, contraction off)"""
    eager, worst = _eager(variant, net)
    MEASURED[(variant, net)] = worst
    print("WORST", variant, net, worst)
    assert max(worst.values()) <= BAR, worst
    graph = _graph(variant, net)
    assert graph[4] == eager[4] == 6
    for i, nm in enumerate(("theta", "s0", "s1", "s2")):
        assert np.array_equal(eager[i].view(np.int32), graph[i].view(np.int32)), (variant, net, nm)


def _tail_steps(variant, net, B, fuse):
    opt = _opt(variant)
    o = opt.as_opt()
    keep, e, x, y = _engine(net, B)
    e.set_option("fuse_tail", fuse)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    for _ in range(5):
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
        e.opt_step_dev(o)
    _, g = e.grad_read()
    return _state(e) + (g,)


@pytest.mark.parametrize("case", list(zip(sorted(NETS), BATCHES)))
@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_tail_is_bit_identical(variant, case):
    """five steps on the net's own gradient of 1, 7 and 1031 rows: the update fused behind the row reduction (k_reduce_opt) against the
    flushed reduction followed by the stand-alone update (k_opt, the eager form of the test above)"""
    net, B = case
    a = _tail_steps(variant, net, B, 1)
    b = _tail_steps(variant, net, B, 0)
    assert a[4] == b[4] == 5
    for i in (0, 1, 2, 3, 5):
        assert np.array_equal(a[i], b[i], equal_nan=True), (variant, case, i)
    assert np.all(np.isfinite(a[0]))


def test_graph_refuses_another_kind_or_slot_shaping_flag():
    import nif_amd
    from nif_amd import NifError
    from nif_amd import optimizers as P
    keep, e, _, _ = _engine("p441")
    z = np.zeros((e.n_params,), f32)
    e.set_opt_state(z, z, 0)
    e.set_opt_slot(2, z)
    e.reserve(8)
    _put_grad(e, _gradients(e.n_params, 3)[0])

    def record(o, step=None):
        e.graph_begin()
        (step or e.opt_step_dev)(o)
        return e.graph_end()

    gid = record(P.Adam(amsgrad=True).as_opt())
    th0 = e.get_flat()
    for other in (P.Adam().as_opt(), P.AdamW(amsgrad=True).as_opt(), P.SGD().as_opt(), P.AdaBeliefOptimizer(amsgrad=True).as_opt()):
        with pytest.raises(NifError, match="another optimizer"):
            e.graph_launch_opt(gid, other)
    with pytest.raises(NifError, match="nif_graph_launch_opt"):
        e.graph_launch(gid, nif_amd.Adam().as_struct())          # the Adam-only entry point: not an amsgrad graph
    assert np.array_equal(e.get_flat(), th0) and e.get_opt_state()[2] == 0
    e.graph_launch_opt(gid, P.Adam(3e-3, amsgrad=True).as_opt())  # other hyper-parameters of the same kind are the replay's to set
    assert e.get_opt_state()[2] == 1
    e.graph_destroy(gid)
    gid = record(P.RMSprop().as_opt())
    with pytest.raises(NifError, match="another optimizer"):
        e.graph_launch_opt(gid, P.RMSprop(centered=True).as_opt())
    e.graph_launch_opt(gid, P.RMSprop(momentum=0.5).as_opt())     # momentum does not shape the slots
    e.graph_destroy(gid)
    e.graph_begin()
    e.opt_step_dev(P.SGD().as_opt())
    with pytest.raises(NifError, match="capture already holds"):
        e.opt_step_dev(P.Adamax().as_opt())
    e.graph_destroy(e.graph_end())
    # a capture cannot initialise Adagrad's accumulator or create the third slot
    keep2, e2, x, y = _engine("p441")
    e2.reserve(8)
    d_x, d_y = e2.alloc(x.size), e2.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    for o in (P.Adagrad().as_opt(), P.RMSprop(centered=True).as_opt()):
        e2.graph_begin()
        e2.loss_grad_dev(d_x.at(0), d_y.at(0), None, 8, 8)
        with pytest.raises(NifError, match="before the capture"):
            e2.opt_step_dev(o)
        e2.graph_destroy(e2.graph_end())


def _wave(n, seed):
    import nif_amd
    return nif_amd.data.synthetic_wave_batch(n, seed=seed)


def test_fit_follows_a_cosine_schedule_through_captured_epochs():
    """3 epochs x 4 batches with Adam(CosineDecay): 12 iterations, the learning rate nif_opt_scalars reports at the final iteration count
    is the schedule at step 11; the epochs replayed from a captured graph (the schedule evaluated per step on the device) give the
    weights of the eager epochs bit for bit"""
    import nif_amd
    from nif_amd import _lib
    from nif_amd import optimizers as P
    kind, cs, cp = cfg_ms(n=16, nst=12, p_act="swish")
    x, y = _wave(4 * 64, 2)
    sch = P.schedules.CosineDecay(_x(1e-3), 16, alpha=_x(0.1))
    runs = {}
    for graph in (True, False):
        nif_amd.set_seed(5)
        m = nif_amd.NIFMultiScale(cs, cp); model = m.build()
        model._graph_epochs = graph
        opt = P.Adam(sch)
        model.compile(opt, "mse")
        e = m._engine
        launches = []
        orig = e.graph_launch_opt
        e.graph_launch_opt = lambda gid, o, orig=orig: (launches.append(gid), orig(gid, o))
        model.fit(x, y, epochs=3, batch_size=64, shuffle=False, verbose=0)
        t = e.get_opt_state()[2]
        assert t == 12 and len(launches) == (3 if graph else 0)
        out = (C.c_double * 5)()
        _lib.check(e.lib.nif_opt_scalars(C.byref(opt.as_opt()), t, out))
        assert abs(out[0] - float(sch(11))) <= 1e-12 * float(sch(11))
        assert out[0] < 0.5 * _x(1e-3) and opt.lr is sch
        runs[graph] = (e.get_flat(), e.get_opt_slot(0), e.get_opt_slot(1))
    for a, b in zip(runs[True], runs[False]):
        assert np.array_equal(a, b)


def test_default_adam_through_fit_is_nif_adam_step_dev_by_hand():
    """the zero-field path: Adam() through fit() against nif_loss_grad_dev + nif_adam_step_dev by hand, bit for bit"""
    import nif_amd
    kind, cs, cp = cfg_ms(n=16, nst=12, p_act="swish")
    x, y = _wave(300, 3)
    nif_amd.set_seed(2)
    m1 = nif_amd.NIFMultiScale(cs, cp); model1 = m1.build()
    w0 = model1.get_weights()
    model1.compile(nif_amd.Adam(), "mse")
    model1.fit(x, y, epochs=2, batch_size=128, shuffle=False, verbose=0)
    m2 = nif_amd.NIFMultiScale(cs, cp); model2 = m2.build()
    model2.set_weights(w0)
    e = m2._engine
    z = np.zeros((e.n_params,), f32)
    e.set_opt_state(z, z, 0)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    adam = nif_amd.Adam().as_struct()
    for _ in range(2):
        for b0 in range(0, 300, 128):
            b = min(128, 300 - b0)
            e.loss_grad_dev(d_x.at(b0 * 2), d_y.at(b0), None, b, b)
            e.adam_step_dev(adam)
    assert e.get_opt_state()[2] == 6
    assert np.array_equal(m1._engine.get_flat(), e.get_flat())
    for s in (0, 1):
        assert np.array_equal(m1._engine.get_opt_slot(s), e.get_opt_slot(s))


def test_fit_with_each_new_kind_trains_and_saves(tmp_path):
    """fit -> save -> load -> fit equals an uninterrupted fit, bit for bit, for Adagrad (its accumulator's start) and centered RMSprop
    (the third slot); the loss falls"""
    import nif_amd
    kind, cs, cp = cfg_ms(n=16, nst=12, p_act="swish")
    x, y = _wave(256, 4)
    for variant in ("adagrad", "rmsprop_centered_momentum"):
        nif_amd.set_seed(3)
        ma = nif_amd.NIFMultiScale(cs, cp); a = ma.build()
        w0 = a.get_weights()
        a.compile(_opt(variant), "mse")
        h = a.fit(x, y, epochs=4, batch_size=64, shuffle=False, verbose=0)
        assert h.history["loss"][-1] < h.history["loss"][0]
        mb = nif_amd.NIFMultiScale(cs, cp); b = mb.build()
        b.set_weights(w0)
        b.compile(_opt(variant), "mse")
        b.fit(x, y, epochs=2, batch_size=64, shuffle=False, verbose=0)
        b.save_weights(str(tmp_path / variant))
        mc = nif_amd.NIFMultiScale(cs, cp); c = mc.build()
        c.compile(_opt(variant), "mse")
        c.load_weights(str(tmp_path / variant))
        c.fit(x, y, epochs=2, batch_size=64, shuffle=False, verbose=0)
        assert mc._engine.get_opt_state()[2] == ma._engine.get_opt_state()[2] == 16
        assert np.array_equal(mc._engine.get_flat(), ma._engine.get_flat())
        for s in (0, 1, 2):
            assert np.array_equal(mc._engine.get_opt_slot(s), ma._engine.get_opt_slot(s))
