"""GPU tests of Keras' use_ema on the k_opt.hip kernels: the weight average (optimizer slot 3) kept behind the update of every kind, in
the eager form (k_opt), the fused tail (k_reduce_opt) and captured graphs (k_opt_dev), the overwrite rule, the state's call orders,
and fit / save_weights / load_weights / TFPLBFGS end to end.

Every comparison is bitwise.  The new arithmetic is avg = mom * avg + (1 - mom) * theta in float32 with contraction off -- two
multiplies, one subtraction of constants and one add, each rounded once -- which NumPy's float32 scalars and arrays reproduce exactly
(_ema below), so there is no tolerance.  The semantics are Keras 2.11's, restated from its documentation and not pinned by a
TensorFlow run.

The nets are those of tests/test_gpu_keras_optimizers.py: the smallest cfg_ms ones whose P leaves a scalar tail of 1, 2 and 3 behind
the 16-byte body of the four-wide stream, one of them with more than one block (P > 1024); plain Adam runs one parameter per thread.
1, 7 and 1031 are the batch sizes (the rows of the fused tail's reduction)."""
import ctypes as C

import numpy as np
import pytest

from tests.cfgs import cfg_ms
from tests.test_gpu_parity import _make

pytestmark = pytest.mark.gpu

f32 = np.float32
NETS = {"p441": cfg_ms(), "p1535": cfg_ms(n=16, nst=12), "p414": cfg_ms(n=8, nst=5)}      # P % 4 = 1, 3, 2
BATCHES = (1, 7, 1031)
CASES = list(zip(sorted(NETS), BATCHES))
KINDS = ["adam_plain", "adam_ams", "adamw", "sgd_momentum", "rmsprop_centered", "adagrad", "adamax", "lion", "adabelief"]
MOM = 0.9


def _opt(name):
    from nif_amd import optimizers as P
    return {
        "adam_plain": lambda: P.Adam(1e-3),                                  # nif_adam_step_dev / nif_graph_launch
        "adam_ams": lambda: P.Adam(1e-3, amsgrad=True),
        "adamw": lambda: P.AdamW(1e-3, weight_decay=1e-2),
        "sgd_momentum": lambda: P.SGD(1e-3, momentum=0.9),
        "rmsprop_centered": lambda: P.RMSprop(momentum=0.5, centered=True),
        "adagrad": lambda: P.Adagrad(1e-2),
        "adamax": lambda: P.Adamax(),
        "lion": lambda: P.Lion(1e-4, wd=1e-2),
        "adabelief": lambda: P.AdaBeliefOptimizer(1e-3, amsgrad=True),
    }[name]()


def _stepper(e, opt):
    """(one eager step, one replay of graph gid) of the optimizer: plain Adam through the nif_adam entry points, else a nif_opt"""
    from nif_amd import optimizers as P
    if isinstance(opt, P.Adam) and opt.is_plain:
        s = opt.as_struct()
        return (lambda: e.adam_step_dev(s)), (lambda gid: e.graph_launch(gid, s))
    o = opt.as_opt()
    return (lambda: e.opt_step_dev(o)), (lambda gid: e.graph_launch_opt(gid, o))


def _fresh(e, opt):
    """what Model.fit writes for a freshly compiled optimizer (a capture cannot initialise a slot); resets the average"""
    from nif_amd.optimizers import slot_layout
    z = np.zeros((e.n_params,), f32)
    e.set_opt_state(np.full_like(z, opt.as_opt().init_acc), z, 0)
    if slot_layout(opt)[3]:
        e.set_opt_slot(2, z)


def _engine(net, B=8):
    m_, model, spec, ws, x, y, sw = _make((NETS[net], B))
    return m_, m_._engine, x, y


def _gradients(P, seed=11):
    """gradients of mixed magnitudes with zeros and a sign change, as tests/test_gpu_keras_optimizers.py writes them"""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(P) * 10.0 ** rng.uniform(-4, 1, P)).astype(f32)
    g[::5] = 0.0
    g2 = (-g * f32(0.5)).astype(f32)
    g3 = (g * rng.uniform(0.5, 2.0, P)).astype(f32)
    g3[1::7] = 0.0
    return [g, g2, g3]


def _put_grad(e, g):
    from nif_amd._lib import check
    buf = np.concatenate([g, [f32(0.5)]]).astype(f32)
    check(e.lib.nif_h2d(e.ctx, C.c_void_p(e.grad_dev_ptr()), buf.ctypes.data_as(C.c_void_p), buf.nbytes))


def _snap(e):
    """(theta, slot 0, 1, 2, the average, iteration count)"""
    return (e.get_flat(),) + tuple(e.get_opt_slot(s) for s in range(4)) + (e.get_opt_state()[2],)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ema(mom, avg, th):
    """the kernels' expression in NumPy float32: each product, the difference and the sum rounded once, no contraction"""
    return f32(mom) * avg + (f32(1) - f32(mom)) * th


def _forced_run(kind, net, mom, freq, steps=7):
    """`steps` eager steps on gradients written to the device (k_opt); -> the state before the first step and after every step.
    mom None: EMA off"""
    opt = _opt(kind)
    keep, e, _, _ = _engine(net)
    _fresh(e, opt)
    if mom is not None:
        e.set_ema(mom, freq)
    step, _ = _stepper(e, opt)
    gs = _gradients(e.n_params)
    out = [_snap(e)]
    for k in range(steps):
        _put_grad(e, gs[(k // 2) % 3])
        step()
        out.append(_snap(e))
    return out


# ---- 1. the recurrence, every kind ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("kind", KINDS)
def test_average_follows_the_recurrence_and_leaves_the_update_alone(kind, net):
    """seven eager steps without overwriting: slot 3 is the NumPy recurrence over the device's own theta sequence bit for bit, seeded
    with theta_0 (avg_1 = mom theta_0 + (1 - mom) theta_1); theta and the kind's slots are those of the same run with EMA off"""
    mom = 0.99 if (kind, net) == ("adam_plain", "p1535") else MOM
    on = _forced_run(kind, net, mom, None)
    off = _forced_run(kind, net, None, None)
    assert not on[0][4].any()                            # slot 3 reads zeros before it exists
    avg = on[0][0]                                       # the seed: theta as it stands before the first step's update
    for k in range(1, 8):
        assert on[k][5] == off[k][5] == k
        avg = _ema(mom, avg, on[k][0])
        assert avg.dtype == f32 and _same(on[k][4], avg), (kind, net, k)
        for i in range(4):
            assert _same(on[k][i], off[k][i]), (kind, net, k, i)
        assert not off[k][4].any()
        assert not _same(on[k][0], on[k - 1][0]) and np.all(np.isfinite(on[k][0]))
    assert not _same(on[7][4], on[7][0])


# ---- 2. the three forms ---------------------------------------------------------------------------------------------------------------
def _own_gradient_run(kind, net, B, freq, form):
    """six steps on the net's own gradient: form "plain" (flushed reduction + k_opt), "fused" (k_reduce_opt), "graph" (two recorded
    steps replayed three times, k_opt_dev: the overwrite decision of each recorded step is taken on the device)"""
    opt = _opt(kind)
    keep, e, x, y = _engine(net, B)
    e.set_option("fuse_tail", 1 if form == "fused" else 0)
    _fresh(e, opt)
    e.set_opt_slot(3, e.get_flat())                      # the seed a first eager step would write; a capture needs it to exist
    e.set_ema(MOM, freq)
    step, launch = _stepper(e, opt)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    e.reserve(B)
    if form == "graph":
        e.graph_begin()
        for _ in range(2):
            e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
            step()
        gid = e.graph_end()
        for _ in range(3):
            launch(gid)
        st = _snap(e)
        e.graph_destroy(gid)
        return st
    for _ in range(6):
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
        step()
    return _snap(e)


@pytest.mark.parametrize("case", [c + (None,) for c in CASES] + [("p1535", 7, 3)])
@pytest.mark.parametrize("kind", KINDS)
def test_the_three_forms_are_bit_identical(kind, case):
    """theta, every slot and the average after six steps; with f = 3 the overwrite steps (t = 3, 6) fall inside the captured sequence"""
    net, B, freq = case
    plain, fused, graph = (_own_gradient_run(kind, net, B, freq, form) for form in ("plain", "fused", "graph"))
    assert plain[5] == fused[5] == graph[5] == 6
    for i in range(5):
        assert _same(plain[i], fused[i]), (kind, case, "fused", i)
        assert _same(plain[i], graph[i]), (kind, case, "graph", i)
    assert np.all(np.isfinite(plain[0])) and plain[4].any()
    assert _same(plain[0], plain[4]) == (freq == 3)      # t = 6 is an overwrite step of f = 3


# ---- 3. overwriting -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam_plain", "sgd_momentum", "lion"])
def test_overwrite_every_f_steps(kind):
    net = "p1535"
    a = _forced_run(kind, net, MOM, None)
    b = _forced_run(kind, net, MOM, 3)
    for k in (0, 1, 2):
        for i in range(5):
            assert _same(a[k][i], b[k][i]), (k, i)
    assert _same(b[3][0], b[3][4]) and _same(b[3][4], a[3][4])      # the average of the updated theta, written back over it
    assert not _same(a[3][0], a[3][4])
    for k in range(4, 8):
        if k % 3 == 0:
            assert _same(b[k][0], b[k][4]), k
        else:
            assert _same(b[k][4], _ema(MOM, b[k - 1][4], b[k][0])), k
            assert not _same(b[k][0], b[k][4])
    c = _forced_run(kind, net, MOM, 1)
    for k in range(1, 8):
        assert _same(c[k][0], c[k][4]), k
        assert not _same(c[k][0], c[k - 1][0])


# ---- 4. the edges of the momentum -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam_plain", "adamax"])
def test_momentum_zero_and_one(kind):
    zero = _forced_run(kind, "p414", 0.0, None, steps=4)
    one = _forced_run(kind, "p414", 1.0, None, steps=4)
    for k in range(1, 5):
        assert np.array_equal(zero[k][4], zero[k][0])    # 0 avg + 1 theta
        assert _same(one[k][4], one[0][0])               # 1 avg + 0 theta: the seed theta_0
        assert _same(one[k][0], zero[k][0])


# ---- 5. state and call orders -----------------------------------------------------------------------------------------------------------
def _err(code):
    return r"error %d:" % code


def test_capture_needs_the_average_and_a_graph_is_tied_to_ema_on_or_off():
    from nif_amd import NifError
    from nif_amd import optimizers as P
    keep, e, x, y = _engine("p441")
    sgd = P.SGD(1e-3, momentum=0.9)
    step, launch = _stepper(e, sgd)
    _fresh(e, sgd)
    e.reserve(8)
    _put_grad(e, _gradients(e.n_params)[0])
    e.set_ema(MOM)
    e.graph_begin()
    with pytest.raises(NifError, match=_err(-4) + ".*before the capture"):
        step()
    e.graph_destroy(e.graph_end())
    assert e.get_opt_state()[2] == 0 and not e.get_opt_slot(3).any()
    step()                                               # one eager step creates it
    th1, avg1 = e.get_flat(), e.get_opt_slot(3)
    e.graph_begin()
    step()
    with pytest.raises(NifError, match=_err(-4)):        # no change of the state inside a capture
        e.set_option("ema", 0)
    with pytest.raises(NifError, match=_err(-4)):
        e.set_option("ema_momentum_bits", 0)
    with pytest.raises(NifError, match=_err(-4)):
        e.set_opt_slot(3, avg1)
    g_on = e.graph_end()
    # recorded with EMA on: refuses a context with EMA off, and nothing moves
    e.set_ema(None)
    with pytest.raises(NifError, match=_err(-4) + ".*weight averaging"):
        launch(g_on)
    assert _same(e.get_flat(), th1) and e.get_opt_state()[2] == 1
    e.graph_begin()
    step()
    g_off = e.graph_end()
    launch(g_off)
    assert _same(e.get_opt_slot(3), avg1) and e.get_opt_state()[2] == 2      # an EMA-off step leaves the average alone
    e.set_ema(MOM)
    with pytest.raises(NifError, match=_err(-4) + ".*weight averaging"):
        launch(g_off)
    th2 = e.get_flat()
    launch(g_on)
    assert _same(e.get_opt_slot(3), _ema(MOM, avg1, e.get_flat())) and not _same(e.get_flat(), th2)
    # momentum and frequency are the replay's: read when the graph is launched
    e.set_ema(0.5, 1)
    avg3 = e.get_opt_slot(3)
    launch(g_on)
    assert e.get_opt_state()[2] == 4 and _same(e.get_flat(), e.get_opt_slot(3))
    assert not _same(e.get_opt_slot(3), avg3)
    e.graph_destroy(g_on); e.graph_destroy(g_off)


def test_mixing_on_and_off_inside_one_capture_is_refused():
    """one setting per graph: the switch between two recorded steps is what is refused (NIF_ERR_STATE, in either direction), so the
    steps behind it record with the setting of the first and the graph replays as a whole with it"""
    from nif_amd import NifError
    from nif_amd import optimizers as P
    for first_on in (True, False):
        keep, e, x, y = _engine("p441")
        sgd = P.SGD(1e-3)
        step, launch = _stepper(e, sgd)
        _fresh(e, sgd)
        e.reserve(8)
        _put_grad(e, _gradients(e.n_params)[0])
        e.set_ema(MOM)
        step()
        avg1 = e.get_opt_slot(3)
        if not first_on:
            e.set_ema(None)
        e.graph_begin()
        step()
        with pytest.raises(NifError, match=_err(-4) + ".*not inside a graph capture"):
            e.set_ema(None if first_on else MOM)
        step()
        gid = e.graph_end()
        launch(gid)
        assert e.get_opt_state()[2] == 3
        assert _same(e.get_opt_slot(3), avg1) == (not first_on)
        e.graph_destroy(gid)


def test_set_option_refuses_bad_values():
    from nif_amd import NifError
    keep, e, _, _ = _engine("p441")
    bits = lambda v: int(np.array([v], f32).view(np.int32)[0])
    for v in (-2, -100):
        with pytest.raises(NifError, match=_err(-1)):
            e.set_option("ema", v)
    for v in (1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(NifError, match=_err(-1)):
            e.set_option("ema_momentum_bits", bits(v))
    with pytest.raises(ValueError):
        e.set_ema(0.9, 0)
    for v in (0.0, 1.0, 0.99):
        e.set_option("ema_momentum_bits", bits(v))
    for v in (-1, 0, 1, 7):
        e.set_option("ema", v)
    for slot in (-1, 4):
        with pytest.raises(NifError, match=_err(-1) + ".*3 weight average"):
            e.get_opt_slot(slot)
    assert not e.get_opt_slot(3).any()


def test_default_momentum_is_099():
    from nif_amd import optimizers as P
    keep, e, _, _ = _engine("p414")
    sgd = P.SGD(1e-3)
    step, _ = _stepper(e, sgd)
    _put_grad(e, _gradients(e.n_params)[0])
    th0 = e.get_flat()
    e.set_option("ema", -1)                              # "ema_momentum_bits" never set
    step()
    assert _same(e.get_opt_slot(3), _ema(0.99, th0, e.get_flat()))


def test_set_opt_state_reseeds_and_set_params_does_not():
    from nif_amd import optimizers as P
    opt = P.Adam(1e-3)
    for reset in (True, False):
        keep, e, _, _ = _engine("p1535")
        step, _ = _stepper(e, opt)
        gs = _gradients(e.n_params)
        e.set_ema(MOM)
        _put_grad(e, gs[0])
        step()
        th1, avg1 = e.get_flat(), e.get_opt_slot(3)
        if reset:
            m, v, t = e.get_opt_state()
            e.set_opt_state(m, v, t)
            assert not e.get_opt_slot(3).any()           # reset: reads zeros until the next step seeds it
            base = th1
        else:
            base = avg1
            th1 = (th1 * f32(0.5)).astype(f32)
            e.set_flat(th1)                              # Keras' set_weights does not touch optimizer variables
            assert _same(e.get_opt_slot(3), avg1)
        _put_grad(e, gs[1])
        step()
        assert _same(e.get_opt_slot(3), _ema(MOM, base, e.get_flat())), reset
        assert not _same(e.get_flat(), th1)
    # a written slot 3 after the reset restores one
    m, v, t = e.get_opt_state()
    e.set_opt_state(m, v, t)
    e.set_opt_slot(3, avg1)
    _put_grad(e, gs[2])
    step()
    assert _same(e.get_opt_slot(3), _ema(MOM, avg1, e.get_flat()))


def test_the_setting_at_step_time_applies_to_a_pending_fused_tail():
    from nif_amd import optimizers as P
    opt = P.SGD(1e-3, momentum=0.9)
    B = 7
    runs = {}
    for name in ("late_on", "never", "late_off"):
        keep, e, x, y = _engine("p414", B)
        e.set_option("fuse_tail", 1)
        step, _ = _stepper(e, opt)
        d_x, d_y = e.alloc(x.size), e.alloc(y.size)
        d_x.upload(x); d_y.upload(y)
        th0 = e.get_flat()
        if name == "late_off":
            e.set_ema(MOM)
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)      # the row reduction waits for the step
        if name == "late_on":
            e.set_ema(MOM)
        if name == "late_off":
            e.set_ema(None)
        step()
        runs[name] = (th0, e.get_flat(), e.get_opt_slot(0), e.get_opt_slot(3), e.grad_read()[1])
    for i in (1, 2, 4):
        assert _same(runs["late_on"][i], runs["never"][i]) and _same(runs["late_off"][i], runs["never"][i])
    assert _same(runs["late_on"][3], _ema(MOM, runs["late_on"][0], runs["late_on"][1]))
    assert not runs["late_off"][3].any() and not runs["never"][3].any()


# ---- 6. the Python surface --------------------------------------------------------------------------------------------------------------
def _wave(n, seed):
    import nif_amd
    return nif_amd.data.synthetic_wave_batch(n, seed=seed)


def _fit_model(seed=5):
    import nif_amd
    kind, cs, cp = cfg_ms(n=16, nst=12, p_act="swish")
    nif_amd.set_seed(seed)
    m = nif_amd.NIFMultiScale(cs, cp)
    return m, m.build()


def test_fit_finalises_eager_and_captured_epochs_alike():
    """Adam(use_ema=True) through fit: the weights end as their average; the epochs replayed from a captured graph give the same bits"""
    import nif_amd
    x, y = _wave(4 * 64, 2)
    runs = {}
    for graph in (False, True):
        m, model = _fit_model()
        model._graph_epochs = graph
        e = m._engine
        launches = []
        orig = e.graph_launch
        e.graph_launch = lambda gid, a, orig=orig: (launches.append(gid), orig(gid, a))
        model.compile(nif_amd.Adam(1e-3, use_ema=True, ema_momentum=0.9), "mse")
        th0 = e.get_flat()
        h = model.fit(x, y, epochs=2, batch_size=64, shuffle=False, verbose=0, validation_data=(x[:32], y[:32]))
        assert len(launches) == (2 if graph else 0) and e.get_opt_state()[2] == 8
        assert _same(e.get_flat(), e.get_opt_slot(3)) and not _same(e.get_flat(), th0)
        assert len(h.history["val_loss"]) == 2
        runs[graph] = (e.get_flat(), e.get_opt_slot(0), e.get_opt_slot(1), e.get_opt_slot(3))
        # the state was fit's: a step by hand afterwards keeps no average
        d_x, d_y = e.alloc(128), e.alloc(64)
        d_x.upload(x[:64]); d_y.upload(y[:64])
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, 64, 64)
        e.adam_step_dev(nif_amd.Adam(1e-3).as_struct())
        assert _same(e.get_opt_slot(3), runs[graph][3])
    for a, b in zip(runs[False], runs[True]):
        assert _same(a, b)
    # the same fit without use_ema: the same slots, other weights (the average, not the last iterate)
    m, model = _fit_model()
    model.compile(nif_amd.Adam(1e-3), "mse")
    model.fit(x, y, epochs=2, batch_size=64, shuffle=False, verbose=0)
    assert _same(m._engine.get_opt_slot(0), runs[False][1]) and _same(m._engine.get_opt_slot(1), runs[False][2])
    assert not _same(m._engine.get_flat(), runs[False][0]) and not m._engine.get_opt_slot(3).any()


@pytest.mark.parametrize("variant", ["adam", "rmsprop_f3"])
def test_save_after_an_epoch_and_resume_equals_the_uninterrupted_fit(variant, tmp_path):
    """saved behind epoch 1 (from a callback: ahead of the finalise), loaded into a fresh model, epoch 2 run there: the weights, the
    slots and the average of the uninterrupted two epochs, bit for bit -- in the Adam file layout and in the nif_opt one"""
    from nif_amd import optimizers as P
    make = {"adam": lambda: P.Adam(1e-3, use_ema=True, ema_momentum=0.9),
            "rmsprop_f3": lambda: P.RMSprop(centered=True, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=3)}[variant]
    x, y = _wave(256, 4)
    ma, a = _fit_model(3)
    w0 = a.get_weights()
    a.compile(make(), "mse")

    class Save(object):
        def on_epoch_end(self, epoch, logs=None):
            if epoch == 0:
                a.save_weights(str(tmp_path / variant))

    a.fit(x, y, epochs=2, batch_size=64, shuffle=False, verbose=0, callbacks=[Save()])
    d = np.load(str(tmp_path / (variant + ".npz")))
    assert "opt_ema" in d and ("adam_m" in d) == (variant == "adam")
    mb, b = _fit_model(4)
    b.compile(make(), "mse")
    b.load_weights(str(tmp_path / variant))
    assert _same(mb._engine.get_opt_slot(3), d["opt_ema"]) and mb._engine.get_opt_state()[2] == 4
    b.fit(x, y, epochs=2, initial_epoch=1, batch_size=64, shuffle=False, verbose=0)
    ea, eb = ma._engine, mb._engine
    assert ea.get_opt_state()[2] == eb.get_opt_state()[2] == 8
    assert _same(ea.get_flat(), eb.get_flat()) and _same(ea.get_flat(), ea.get_opt_slot(3))
    for s in range(4):
        assert _same(ea.get_opt_slot(s), eb.get_opt_slot(s)), s
    assert not _same(ea.get_flat(), np.concatenate([w.ravel() for w in w0]))


def test_lbfgs_starts_from_the_averaged_weights():
    import nif_amd
    from nif_amd.optimizers import TFPLBFGS
    x, y = _wave(256, 6)
    m, model = _fit_model(7)
    model.compile(nif_amd.Adam(1e-3, use_ema=True, ema_momentum=0.9), "mse")
    model.fit(x, y, epochs=2, batch_size=64, shuffle=False, verbose=0)
    e = m._engine
    avg = e.get_opt_slot(3)
    t = TFPLBFGS(model, "mse", x, y, display_epoch=1 << 30)
    assert _same(t.position, avg)
    hist = t.minimize(rounds=1, max_iter=2)
    assert len(hist["loss"]) >= 2 and np.all(np.isfinite(hist["loss"])) and min(hist["loss"]) < hist["loss"][0]
    assert _same(e.get_opt_slot(3), avg) and not _same(e.get_flat(), avg)      # the fine-tuner moves the weights, not the average
