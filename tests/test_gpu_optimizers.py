"""GPU tests of the Lion / AdaBelief updates (k_opt.hip, nif_opt_step_dev) against the NumPy restatement of tests/opt_ref.py:
crafted gradients, a teacher-forced trajectory on the three kernel families of test_gpu_tail.py, the fused tail against the plain
reduction + update, captured epochs against eager ones, and fit / save / load end to end.  Every bar states the value measured
against it ("Lion and AdaBelief")."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import opt_ref as R
from tests.test_gpu_parity import _make
from tests.test_gpu_tail import CASES

pytestmark = pytest.mark.gpu

f32 = np.float32


def _opt(name):
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    return {
        "lion": lambda: Lion(),
        "lion_wd_decay": lambda: Lion(learning_rate=1e-3, wd=1e-2, decay=1e-3),
        "adabelief": lambda: AdaBeliefOptimizer(),
        "adabelief_norect": lambda: AdaBeliefOptimizer(rectify=False),
        "adabelief_ams": lambda: AdaBeliefOptimizer(amsgrad=True),
        "adabelief_wd": lambda: AdaBeliefOptimizer(weight_decay=1e-2),
        "adabelief_warmup": lambda: AdaBeliefOptimizer(total_steps=10, warmup_proportion=0.3, min_lr=1e-5),
        "adabelief_reg": lambda: AdaBeliefOptimizer(learning_rate=1e-2),
        "lion_reg": lambda: Lion(learning_rate=1e-3),
    }[name]()


def _state(e, opt):
    th = e.get_flat()
    m, v, t = e.get_opt_state()
    vh = e.get_opt_slot(2) if opt.amsgrad else None
    return th, m, v, vh, t


def _restated(opt, th, g, m, v, vh, t):
    if opt.kind == 1:
        th2, m2 = R.lion(th, g, m, opt, t)
        return th2, m2, v, vh
    return R.adabelief(th, g, m, v, vh, opt, t)


def _check_update(opt, before, g, after, what=""):
    """m / v / vhat within 2 ulp; Lion theta within 2 ulp where the sign of c is unambiguous in fp32 (else one of the three outcomes);
    AdaBelief: the change of theta within 1e-5 relative (+ 2 ulp of theta for the final rounding)"""
    th0, m0, v0, vh0, t0 = before
    th1, m1, v1, vh1, t1 = after
    assert t1 == t0 + 1
    th_r, m_r, v_r, vh_r = _restated(opt, th0, g, m0, v0, vh0, t1)
    worst = {"m": float(R.ulps(m1, m_r).max())}
    assert worst["m"] <= 2, (what, worst)
    if opt.kind == 1:
        c, big = R.lion_c(g, m0, opt)
        amb = np.abs(c) <= 4 * np.spacing(big.astype(f32)).astype(np.float64)
        u = R.ulps(th1, th_r)
        worst["theta"] = float(u[~amb].max()) if (~amb).any() else 0.0
        assert worst["theta"] <= 2, (what, worst)
        if amb.any():          # one of sign = -1, 0, +1
            lr = f32(R.scalars(opt, t1)[0])
            cands = [th0[amb] - lr * (f32(s) + th0[amb] * f32(opt.wd)) for s in (-1.0, 0.0, 1.0)]
            assert np.all(np.any([np.abs(th1[amb] - cnd) <= 2 * np.spacing(np.abs(cnd)) for cnd in cands], axis=0)), what
    else:
        worst["v"] = float(R.ulps(v1, v_r).max())
        assert worst["v"] <= 2, (what, worst)
        if opt.amsgrad:
            worst["vhat"] = float(R.ulps(vh1, vh_r).max())
            assert worst["vhat"] <= 2, (what, worst)
        d_gpu = th1.astype(np.float64) - th0
        d_ref = th_r.astype(np.float64) - th0
        err = np.abs(d_gpu - d_ref) - 2 * np.spacing(np.abs(th_r)).astype(np.float64)
        rel = np.max(np.maximum(err, 0) / np.maximum(np.abs(d_ref), 1e-30))
        worst["dtheta_rel"] = float(rel)
        assert rel <= 1e-5, (what, worst)
    print("WORST", what, worst)
    return worst


# ---- 1. crafted gradients ------------------------------------------------------------------------------------------------------
def _crafted(P, opt, rng):
    """theta, g, m, v, vhat with exact zeros (m = 0), exact Lion ties b1 m = -(1-b1) g, denormals and large magnitudes"""
    th = rng.uniform(-2, 2, P).astype(f32)
    g = (rng.standard_normal(P) * 10.0 ** rng.uniform(-8, 2, P)).astype(f32)
    m = (rng.standard_normal(P) * 10.0 ** rng.uniform(-8, 1, P)).astype(f32)
    v = (10.0 ** rng.uniform(-12, 2, P)).astype(f32)
    q = P // 8
    g[:q] = 0; m[:q] = 0                                                     # exact zeros
    b1, ob1 = f32(opt.beta_1), f32(1) - f32(opt.beta_1)
    cand_m = rng.uniform(-4, 4, 4 * q).astype(f32)
    cand_g = (-(cand_m * b1) / ob1).astype(f32)
    tie = (cand_g * ob1) == -(cand_m * b1)                                   # the fp32 products cancel exactly
    k = min(q, int(tie.sum()))
    assert k > 8
    m[q:q + k] = cand_m[tie][:k]; g[q:q + k] = cand_g[tie][:k]
    g[2 * q:2 * q + q // 2] = f32(1e-40) * np.sign(rng.standard_normal(q // 2)).astype(f32)   # denormal gradients
    m[2 * q + q // 2:3 * q] = f32(3e-41)
    g[3 * q:3 * q + q // 2] = (rng.uniform(1e15, 1e18, q // 2) * np.sign(rng.standard_normal(q // 2))).astype(f32)   # large
    th[3 * q + q // 2:4 * q] = rng.uniform(1e20, 1e25, q - q // 2).astype(f32)
    vh = (v * rng.uniform(0.5, 2.0, P)).astype(f32)
    return th, g, m, v, vh


@pytest.mark.parametrize("name", ["lion", "lion_wd_decay", "adabelief", "adabelief_norect", "adabelief_ams", "adabelief_wd"])
@pytest.mark.parametrize("step0", [0, 9])
def test_crafted_gradients(name, step0):
    """measured over all twelve cases: m / v / vhat 0 ulp, Lion theta 0 ulp outside the ties, AdaBelief dtheta 0 beyond the 2-ulp
    rounding allowance (bars 2 ulp, 2 ulp, 1e-5 relative)"""
    opt = _opt(name)
    m_, model, spec, ws, x, y, sw = _make(CASES["small_nif_32x2"])
    e = m_._engine
    P = e.n_params
    assert P % 4 != 0
    th, g, m, v, vh = _crafted(P, opt, np.random.default_rng(step0 + 7))
    e.set_flat(th)
    e.set_opt_state(m, v, step0)
    if opt.amsgrad:
        e.set_opt_slot(2, vh)
    buf = np.concatenate([g, [f32(0.5)]]).astype(f32)
    from nif_amd._lib import check
    check(e.lib.nif_h2d(e.ctx, C.c_void_p(e.grad_dev_ptr()), buf.ctypes.data_as(C.c_void_p), buf.nbytes))
    before = (th, m, v, vh if opt.amsgrad else None, step0)
    e.opt_step_dev(opt.as_opt())
    after = _state(e, opt)
    _check_update(opt, before, g, after, name)
    if opt.kind == 1 and opt.wd == 0:
        q = P // 8
        assert np.array_equal(after[0][:q].view(np.int32), th[:q].view(np.int32))      # g = m = 0: theta bit-unchanged
    assert np.all(np.isfinite(after[0]))


# ---- 2. teacher-forced trajectory -------------------------------------------------------------------------------------------------
VARIANTS = ["lion", "lion_wd_decay", "adabelief", "adabelief_norect", "adabelief_ams", "adabelief_wd", "adabelief_warmup", "adabelief_reg",
            "lion_reg"]


@pytest.mark.parametrize("family", sorted(CASES))
@pytest.mark.parametrize("variant", VARIANTS)
def test_teacher_forced_trajectory(family, variant):
    """12 steps; each one against the restatement applied to the GPU's previous state and this step's GPU gradient.  AdaBelief's
    default covers the momentum steps 1-5 and the rectified steps from 6; adabelief_warmup runs past total_steps = 10.  Measured
    worst over all 27 cases x 12 steps: m / v / vhat 0 ulp, Lion theta 0 ulp, AdaBelief dtheta 0 beyond the 2-ulp rounding allowance
    (bars 2 ulp, 2 ulp, 1e-5 relative): the kernels run the restatement's float sequence, contraction off"""
    opt = _opt(variant)
    m_, model, spec, ws, x, y, sw = _make(CASES[family])
    e = m_._engine
    if variant.endswith("_reg"):
        n_pnet = sum(int(np.prod(s)) for nm, s in spec.param_shapes() if nm.startswith("pnet_"))
        e.set_regularizer(0.0, 1e-3, 0, n_pnet)
    z = np.zeros((e.n_params,), f32)
    e.set_opt_state(z, z, 0)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    B = x.shape[0]
    for _ in range(12):
        before = _state(e, opt)
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
        _, g = e.grad_read()                      # (the regulariser term included, once)
        e.opt_step_dev(opt.as_opt())
        _check_update(opt, before, g, _state(e, opt), "%s/%s step %d" % (family, variant, before[4] + 1))
    assert e.get_opt_state()[2] == 12


# ---- 3. fused tail ---------------------------------------------------------------------------------------------------------------
def _steps(name, fuse, variant, nsteps=3):
    opt = _opt(variant)
    m_, model, spec, ws, x, y, sw = _make(CASES[name])
    e = m_._engine
    e.set_option("fuse_tail", fuse)
    z = np.zeros((e.n_params,), f32)
    e.set_opt_state(z, z, 0)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    losses = []
    for _ in range(nsteps):
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, x.shape[0], x.shape[0])
        e.opt_step_dev(opt.as_opt())
        losses.append(e.last_loss())
    mm, vv, step = e.get_opt_state()
    _, g = e.grad_read()
    return np.array(losses), e.get_flat(), mm, vv, e.get_opt_slot(2), g, step


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("variant", ["lion_wd_decay", "adabelief", "adabelief_ams"])
def test_fused_tail_is_bit_identical(name, variant):
    a = _steps(name, 1, variant)
    b = _steps(name, 0, variant)
    assert a[6] == b[6] == 3
    for i in range(6):
        assert np.array_equal(a[i], b[i]), (name, variant, i)


# ---- 4. captured epochs --------------------------------------------------------------------------------------------------------
def _cfg0():
    cs = {"input_dim": 1, "output_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    cp = {"input_dim": 1, "latent_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    return cs, cp


@pytest.mark.parametrize("variant", ["lion", "adabelief_ams"])
def test_graph_epochs_equal_eager_epochs_configs0(variant):
    """BASELINE configs[0] at its own size: 10 000 points, batch 512, 20 steps per epoch, 4 epochs.  Lion (decay 0): bit-identical
    (measured 0); AdaBelief with amsgrad: within 2e-6, the Adam bar (measured 0)"""
    import nif_amd
    cs, cp = _cfg0()
    x, y = O.synthetic_wave_batch(10000, seed=0)
    runs = {}
    for graph in (True, False):
        nif_amd.set_seed(4)
        m = nif_amd.NIF(cs, cp); model = m.build()
        model._graph_epochs = graph
        model.compile(_opt(variant), "mse")
        e = m._engine
        launches = []
        orig = e.graph_launch_opt
        e.graph_launch_opt = lambda gid, o: (launches.append(gid), orig(gid, o))
        h = model.fit(x, y, epochs=4, batch_size=512, shuffle=False, verbose=0)
        assert e.get_opt_state()[2] == 80
        assert len(launches) == (4 if graph else 0)          # epoch 1 records the graph, every epoch runs it
        runs[graph] = (np.array(h.history["loss"]), e.get_flat(), e.get_opt_slot(0), e.get_opt_slot(2))
    if variant == "lion":
        for a, b in zip(runs[True], runs[False]):
            assert np.array_equal(a, b)
    else:
        assert np.allclose(runs[True][0], runs[False][0], rtol=2e-6)
        assert np.abs(runs[True][1] - runs[False][1]).max() < 2e-6
    assert runs[True][0][-1] < runs[True][0][0]


def test_graph_kind_mismatches_raise():
    import nif_amd
    from nif_amd import NifError
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    cs, cp = _cfg0()
    x, y = O.synthetic_wave_batch(2048, seed=1)
    nif_amd.set_seed(4)
    m = nif_amd.NIF(cs, cp); m.build()
    e = m._engine
    e.reserve(512)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    lion, ab, adam = Lion().as_opt(), AdaBeliefOptimizer().as_opt(), nif_amd.Adam(1e-3).as_struct()
    e.graph_begin()
    for b in range(4):
        e.loss_grad_dev(d_x.at(b * 512 * 2), d_y.at(b * 512), None, 512, 512)
        e.opt_step_dev(lion)
    gid = e.graph_end()
    th0 = e.get_flat()
    with pytest.raises(NifError, match="another optimizer"):
        e.graph_launch_opt(gid, ab)
    with pytest.raises(NifError, match="Lion / AdaBelief"):
        e.graph_launch(gid, adam)
    with pytest.raises(NifError, match="another optimizer"):
        e.graph_launch_opt(gid, AdaBeliefOptimizer(amsgrad=True).as_opt())
    assert np.array_equal(e.get_flat(), th0) and e.get_opt_state()[2] == 0      # nothing ran
    e.graph_launch_opt(gid, lion)
    assert e.get_opt_state()[2] == 4 and not np.array_equal(e.get_flat(), th0)
    e.graph_destroy(gid)
    # kinds mixed inside one capture: the mixing step fails, nothing is silently recorded
    for first, second in ((lion, ab), (adam, lion), (lion, adam)):
        e.graph_begin()
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, 512, 512)
        (e.adam_step_dev if first is adam else e.opt_step_dev)(first)
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, 512, 512)
        with pytest.raises(NifError, match="capture already holds"):
            (e.adam_step_dev if second is adam else e.opt_step_dev)(second)
        e.graph_destroy(e.graph_end())


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["lion_wd_decay", "adabelief_ams"])
def test_fit_equals_the_manual_sequence(variant):
    """fit() for 2 epochs against nif_loss_grad_dev + nif_opt_step_dev by hand: bit for bit"""
    import nif_amd
    from tests.test_gpu_parity import _cfg
    kind, cs, cp = _cfg("NIFMultiScale", 64, 2, 32, 2, 1, 1, 1, 1, p_act="swish")
    x, y = nif_amd.data.synthetic_wave_batch(1500, seed=3)
    nif_amd.set_seed(2)
    m1 = nif_amd.NIFMultiScale(cs, cp); model1 = m1.build()
    w0 = model1.get_weights()
    model1.compile(_opt(variant), "mse")
    model1.fit(x, y, epochs=2, batch_size=512, shuffle=False, verbose=0)
    m2 = nif_amd.NIFMultiScale(cs, cp); model2 = m2.build()
    model2.set_weights(w0)
    e = m2._engine
    z = np.zeros((e.n_params,), f32)
    e.set_opt_state(z, z, 0)
    e.set_opt_slot(2, z)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    o = _opt(variant).as_opt()
    for _ in range(2):
        for b0 in range(0, 1500, 512):
            b = min(512, 1500 - b0)
            e.loss_grad_dev(d_x.at(b0 * 2), d_y.at(b0), None, b, b)
            e.opt_step_dev(o)
    assert np.array_equal(m1._engine.get_flat(), e.get_flat())
    assert np.array_equal(m1._engine.get_opt_slot(1), e.get_opt_slot(1))


@pytest.mark.parametrize("variant", ["lion", "adabelief"])
def test_loss_falls_on_the_travelling_wave(variant):
    """80 epochs of 4 batches, reference defaults but Lion at 3e-4.  Measured last / first epoch loss: Lion 0.101, AdaBelief 0.737
    (eps 1e-14 makes its early steps nearly sign-like at lr 1e-3); bars 0.5 and 0.85"""
    import nif_amd
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    from tests.test_gpu_parity import _cfg
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "traveling_wave.npz"))["data"]
    data, _, _ = O.standard_normalize(d.astype(np.float64))
    x, y = data[:, :2].astype(np.float32), data[:, 2:3].astype(np.float32)
    kind, cs, cp = _cfg("NIFMultiScale", 32, 2, 32, 2, 1, 1, 1, 1, p_act="swish")
    nif_amd.set_seed(1)
    model = nif_amd.NIFMultiScale(cs, cp).build()
    model.compile(Lion(learning_rate=3e-4) if variant == "lion" else AdaBeliefOptimizer(learning_rate=1e-3), loss="mse")
    model._shuffle_seed = 0
    h = model.fit(x, y, epochs=80, batch_size=500, shuffle=True, verbose=0)
    print("LOSS", variant, h.history["loss"][0], h.history["loss"][-1])
    assert h.history["loss"][-1] < (0.5 if variant == "lion" else 0.85) * h.history["loss"][0], h.history["loss"][::10]


@pytest.mark.parametrize("variant", ["lion_wd_decay", "adabelief_ams"])
def test_save_load_continue_equals_an_uninterrupted_run(variant, tmp_path):
    import nif_amd
    from tests.test_gpu_parity import _cfg
    kind, cs, cp = _cfg("NIFMultiScale", 64, 2, 32, 2, 1, 1, 1, 1, p_act="swish")
    x, y = nif_amd.data.synthetic_wave_batch(1200, seed=5)
    nif_amd.set_seed(3)
    ma = nif_amd.NIFMultiScale(cs, cp); a = ma.build()
    w0 = a.get_weights()
    a.compile(_opt(variant), "mse")
    a.fit(x, y, epochs=4, batch_size=256, shuffle=False, verbose=0)
    mb = nif_amd.NIFMultiScale(cs, cp); b = mb.build()
    b.set_weights(w0)
    b.compile(_opt(variant), "mse")
    b.fit(x, y, epochs=2, batch_size=256, shuffle=False, verbose=0)
    b.save_weights(str(tmp_path / "ck"))
    mc = nif_amd.NIFMultiScale(cs, cp); c = mc.build()
    c.compile(_opt(variant), "mse")
    c.load_weights(str(tmp_path / "ck"))
    c.fit(x, y, epochs=2, batch_size=256, shuffle=False, verbose=0)
    assert mc._engine.get_opt_state()[2] == ma._engine.get_opt_state()[2] == 20
    assert np.array_equal(mc._engine.get_flat(), ma._engine.get_flat())
    for s in (0, 1, 2):
        assert np.array_equal(mc._engine.get_opt_slot(s), ma._engine.get_opt_slot(s))
