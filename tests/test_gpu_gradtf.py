"""GPU tests of the gradient transform (k_gradtf.hip, nif_set_grad_transform) against the NumPy restatement of tests/gradtf_ref.py:
crafted gradients, a teacher-forced trajectory on the three kernel families of test_gpu_tail.py, the step's routes against each other,
a captured epoch against the eager one, the transform behind the all-reduce, and fit end to end.  Bars: centralisation and the clamps
bit-identical to the float32 restatement; norm stages within 2 ulp of it and within 1e-5 relative of the float64 one (a fixed-order
fp32 sum of non-negative squares with chains of a few dozen additions is off by far less).  Every test prints the worst value."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import gradtf_ref as G
from tests import opt_ref as R
from tests.test_gpu_parity import _cfg, _make
from tests.test_gpu_tail import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(a):
    return np.asarray(a, f32).view(np.int32)


def _put_grad(e, g, loss=0.5):
    from nif_amd._lib import check
    buf = np.concatenate([np.asarray(g, f32), [f32(loss)]]).astype(f32)
    check(e.lib.nif_h2d(e.ctx, C.c_void_p(e.grad_dev_ptr()), buf.ctypes.data_as(C.c_void_p), buf.nbytes))


def _get_grad(e):
    from nif_amd._lib import check
    out = np.empty((e.n_params + 1,), f32)
    check(e.lib.nif_d2h(e.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(e.grad_dev_ptr()), out.nbytes))
    return out


def _check_transform(got, g, layout, spec, what):
    """stages 1, 2, 5 alone: bit-identical; with a norm stage: 2 ulp of the float32 restatement, 1e-5 relative of the float64 one"""
    r32, per32, glob32 = G.transform32(g, layout, spec)
    stage = G.plan(spec)[1]
    worst = {"ulp": float(G.ulps(got, r32).max())}
    if stage == 0:
        assert np.array_equal(_bits(got), _bits(r32)), (what, worst)
    else:
        assert worst["ulp"] <= 2, (what, worst)
        r64 = G.transform64(g, layout, spec)[0]
        with np.errstate(all="ignore"):
            ok = np.isfinite(r64) & (np.abs(r64) >= 1e-30)       # (denormal results carry fewer bits: the 2-ulp bar covers them)
            rel = np.abs(got.astype(np.float64) - r64)[ok] / np.abs(r64[ok])
        worst["rel64"] = float(rel.max()) if rel.size else 0.0
        assert worst["rel64"] <= 1e-5, (what, worst)
    print("WORST", what, worst)
    return per32, glob32


# ---- 1. crafted gradients ----------------------------------------------------------------------------------------------------------
def _crafted(P, layout, rng):
    g = (rng.standard_normal(P) * 10.0 ** rng.uniform(-6, 1, P)).astype(f32)
    q = P // 8
    g[q:q + q // 2] = f32(1e-40) * np.sign(rng.standard_normal(q // 2)).astype(f32)        # denormals
    g[2 * q:2 * q + 16] = (rng.uniform(1e15, 2e15, 16) * np.sign(rng.standard_normal(16))).astype(f32)
    name, off, rows, cols = layout[3]
    g[off:off + rows * (cols or 1)] = 0                                                   # an all-zero tensor
    return g


SPECS = {
    "centralize": {"centralize": True},
    "clipvalue": {"clipvalue": 0.02},
    "clipnorm": {"clipnorm": "n_mid"},
    "global_clipnorm": {"global_clipnorm": "n/3"},
    "global_clipnorm_idle": {"global_clipnorm": "3n"},
    "gtcf_full": {"centralize": True, "gtcf": True, "clipnorm": "n/3", "clipvalue": "cv"},
    "gtcf_clipvalue_only": {"centralize": True, "gtcf": True, "clipvalue": 0.02},
    "gtcf_norm_idle": {"centralize": True, "gtcf": True, "clipnorm": "3n"},
}


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("case", sorted(SPECS))
def test_crafted_gradients(case, big):
    """measured over the 16 cases: 0 ulp against the float32 restatement everywhere (bars: bit-identical / 2 ulp); against float64
    1.6e-7 relative without centralisation, 6.8e-6 with it, where the subtraction of the mean cancels (bar 1e-5)"""
    m_, model, spec_, ws, x, y, sw = _make(CASES["small_nif_32x2"])
    e = m_._engine
    P, layout = e.n_params, e.layout()
    assert P % 4 != 0
    assert any(c > 0 and r == 1 for _, _, r, c in layout)           # rows == 1 matrices (latent_dim = 1, one input)
    g = _crafted(P, layout, np.random.default_rng(5))
    if not big:
        g[np.abs(g) > 1e10] = f32(0.25)
    base = {k: v for k, v in SPECS[case].items() if not isinstance(v, str)}
    pre = G.transform64(g, layout, {k: v for k, v in base.items() if k == "centralize"})
    n, per = pre[2], pre[1]
    sub = {"n/3": n / 3, "3n": 3 * n, "n_mid": float(np.median(per[per > 0])), "cv": n / 3 / 40}
    spec = {k: (float(f32(sub[v])) if isinstance(v, str) else v) for k, v in SPECS[case].items()}
    e.set_grad_transform(spec)
    _put_grad(e, g, 0.5)
    e.grad_transform_dev()
    out = _get_grad(e)
    assert _bits(out[P:])[0] == _bits([0.5])[0]                      # the loss slot: bit-unchanged
    got = out[:P]
    per32, glob32 = _check_transform(got, g, layout, spec, "%s big=%s" % (case, big))
    name, off, rows, cols = layout[3]
    assert np.all(_bits(got[off:off + rows * (cols or 1)]) == 0)     # norm 0: stays zero, no NaN
    assert np.all(np.isfinite(got))
    if spec.get("centralize"):
        for nm, off, rows, cols in layout:
            if cols > 0 and rows == 1:
                assert np.all(_bits(got[off:off + cols]) == 0), nm   # exactly 0.0, bitwise
    pn, gn = e.grad_norms()
    assert np.array_equal(_bits(pn), _bits(per32)) and _bits([gn])[0] == _bits([glob32])[0]
    e.set_grad_transform(None)


@pytest.mark.parametrize("kind", ["global_clipnorm", "gtcf", "clipnorm"])
def test_norm_just_below_and_just_above_the_threshold(kind):
    m_, model, spec_, ws, x, y, sw = _make(CASES["small_nif_32x2"])
    e = m_._engine
    P, layout = e.n_params, e.layout()
    g = np.random.default_rng(9).standard_normal(P).astype(f32)
    _, per, glob = G.transform32(g, layout, {})
    n = per[4] if kind == "clipnorm" else glob
    for c in (np.nextafter(n, f32(0)), n, np.nextafter(n, f32(np.inf))):
        spec = {"global_clipnorm": {"global_clipnorm": float(c)}, "gtcf": {"gtcf": True, "clipnorm": float(c)},
                "clipnorm": {"clipnorm": float(c)}}[kind]
        e.set_grad_transform(spec)
        _put_grad(e, g)
        e.grad_transform_dev()
        _check_transform(_get_grad(e)[:P], g, layout, spec, "%s c=%r n=%r" % (kind, c, n))
    e.set_grad_transform(None)


# ---- 2. teacher-forced trajectory ---------------------------------------------------------------------------------------------------
def _adam32(th, g, m, v, opt, t):
    """k_opt.hip adam_1 in float32: m += (g - m)(1 - b1); v = fma(g g - v, 1 - b2, v); theta -= lr_t m / (sqrt(v) + eps)"""
    th, g, m, v = (np.asarray(a, f32) for a in (th, g, m, v))
    b1, b2, eps = f32(opt.beta_1), f32(opt.beta_2), f32(opt.epsilon)
    bc1, bc2 = 1.0 - float(b1) ** t, 1.0 - float(b2) ** t
    lr = f32(float(f32(opt.learning_rate)) * np.sqrt(bc2) / bc1)
    with np.errstate(all="ignore"):
        m2 = m + (g - m) * (f32(1) - b1)
        v2 = ((g * g - v).astype(np.float64) * float(f32(1) - b2) + v.astype(np.float64)).astype(f32)
        th2 = th - lr * m2 / (np.sqrt(v2) + eps)
    return th2.astype(f32), m2.astype(f32), v2


def _variant(name):
    import nif_amd
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion, centralized_gradients_for_optimizer
    if name.startswith("adam"):
        return nif_amd.Adam(1e-3), name[5:]
    opt = Lion(learning_rate=1e-3) if name.startswith("lion") else AdaBeliefOptimizer()
    opt.get_gradients = centralized_gradients_for_optimizer(opt)
    return opt, "gtcf"


def _step(e, opt):
    e.adam_step_dev(opt.as_struct()) if hasattr(opt, "as_struct") else e.opt_step_dev(opt.as_opt())


@pytest.mark.parametrize("family", sorted(CASES))
@pytest.mark.parametrize("variant", ["adam_global_clipnorm", "adam_clipnorm", "adam_clipvalue", "lion_gtcf_clip", "adabelief_gtcf"])
def test_teacher_forced_trajectory(family, variant):
    """8 steps; each against the restated transform of this step's untransformed GPU gradient followed by the restated update from the
    GPU's previous state.  The constant of step k comes from step k - 1's norm (alternately below and above it), so clipping is
    active on some steps and idle on others.  Bars of tests/opt_ref.py's users: slots 2 ulp, Lion theta 2 ulp outside sign ties, the
    change of theta 1e-5 relative (+ 2 ulp of theta) for Adam and AdaBelief"""
    from nif_amd.optimizers import grad_transform_of
    opt, route = _variant(variant)
    m_, model, spec_, ws, x, y, sw = _make(CASES[family])
    e = m_._engine
    P, layout = e.n_params, e.layout()
    z = np.zeros((P,), f32)
    e.set_opt_state(z, z, 0)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    B = x.shape[0]
    active, worst = [], {"m": 0.0, "v": 0.0, "theta": 0.0, "dtheta_rel": 0.0}
    prev = None
    for k in range(8):
        e.set_grad_transform(None)
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
        _, g = e.grad_read()                                   # untransformed
        cen = route == "gtcf"
        _, per, glob = G.transform32(g, layout, {"centralize": cen})
        ref_n = float(np.median(per[per > 0])) if route == "clipnorm" else float(glob)
        top_n = float(per.max()) if route == "clipnorm" else ref_n     # (per tensor: idle means above EVERY tensor's norm)
        if prev is None:
            prev = (ref_n, top_n)
        c = float(f32(prev[0] * 0.5 if k % 2 == 0 else prev[1] * 4.0))
        prev = (ref_n, top_n)
        if route == "global_clipnorm":
            opt.global_clipnorm = c; on = glob > c
        elif route == "clipnorm":
            opt.clipnorm = c; on = bool(np.any(per > c))
        elif route == "clipvalue":
            opt.clipvalue = c = float(f32(np.abs(g).max() * (0.25 if k % 2 == 0 else 4.0))); on = bool(np.abs(g).max() > c)
        elif variant == "lion_gtcf_clip":
            opt.clipnorm, opt.clipvalue = c, float(f32(c / 20)); on = glob >= c
        else:
            on = k % 2 == 0                                    # centralise only: nothing to straddle
        active.append(bool(on))
        tf = grad_transform_of(opt)
        e.set_grad_transform(tf)
        th0 = e.get_flat(); m0, v0, t0 = e.get_opt_state()
        _step(e, opt)
        th1 = e.get_flat(); m1, v1, t1 = e.get_opt_state()
        assert t1 == t0 + 1
        gt = G.transform32(g, layout, tf)[0]
        got_g = _get_grad(e)[:P]                               # the buffer holds the transformed gradient after the step
        assert G.ulps(got_g, gt).max() <= 2
        if variant.startswith("lion"):
            th_r, m_r = R.lion(th0, gt, m0, opt, t1); v_r = v0
        elif variant.startswith("adabelief"):
            th_r, m_r, v_r, _ = R.adabelief(th0, gt, m0, v0, None, opt, t1)
        else:
            th_r, m_r, v_r = _adam32(th0, gt, m0, v0, opt, t1)
        # the slots from the GPU's own transformed gradient: 2 ulp; from the restated one they differ by what 2 ulp of g carry
        if variant.startswith("lion"):
            m_g = R.lion(th0, got_g, m0, opt, t1)[1]; v_g = v0
        elif variant.startswith("adabelief"):
            _, m_g, v_g, _ = R.adabelief(th0, got_g, m0, v0, None, opt, t1)
        else:
            _, m_g, v_g = _adam32(th0, got_g, m0, v0, opt, t1)
        worst["m"] = max(worst["m"], float(R.ulps(m1, m_g).max()))
        worst["v"] = max(worst["v"], float(R.ulps(v1, v_g).max()))
        assert worst["m"] <= 2 and worst["v"] <= 2, (family, variant, k, worst)
        with np.errstate(all="ignore"):
            assert np.max(np.abs(m1.astype(np.float64) - m_r) / np.maximum(np.abs(m_r), 1e-30)) <= 1e-5 or R.ulps(m1, m_r).max() <= 8
        if variant.startswith("lion"):
            cc, big = R.lion_c(got_g, m0, opt)
            amb = np.abs(cc) <= 4 * np.spacing(big.astype(f32)).astype(np.float64)
            th_g = R.lion(th0, got_g, m0, opt, t1)[0]
            u = R.ulps(th1, th_g)
            worst["theta"] = max(worst["theta"], float(u[~amb].max()))
            assert worst["theta"] <= 2, (family, variant, k, worst)
        else:
            d_gpu = th1.astype(np.float64) - th0
            d_ref = th_r.astype(np.float64) - th0
            err = np.abs(d_gpu - d_ref) - 2 * np.spacing(np.abs(th_r)).astype(np.float64)
            rel = float(np.max(np.maximum(err, 0) / np.maximum(np.abs(d_ref), 1e-30)))
            worst["dtheta_rel"] = max(worst["dtheta_rel"], rel)
            assert rel <= 1e-5, (family, variant, k, worst)
    print("WORST", family, variant, worst, "clipping active on steps", [i for i, a in enumerate(active) if a])
    assert any(active) and not all(active), active
    e.set_grad_transform(None)


# ---- 3. routes agree ---------------------------------------------------------------------------------------------------------------
def _three_steps(name, tf, options=(), never_set=False):
    import nif_amd
    m_, model, spec_, ws, x, y, sw = _make(CASES[name])
    e = m_._engine
    for k, v in options:
        e.set_option(k, v)
    if not never_set:
        e.set_grad_transform(tf)
    adam = nif_amd.Adam(1e-3).as_struct()
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    for _ in range(3):
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, x.shape[0], x.shape[0])
        e.adam_step_dev(adam)
    mm, vv, step = e.get_opt_state()
    return e.get_flat(), mm, vv, _get_grad(e), e


@pytest.mark.parametrize("name", sorted(CASES))
def test_routes_agree_bit_for_bit(name):
    """fuse_tail 1 vs 0 on every family -- on k_small's step (small_step 1) and on the tile kernels' (small_step 0) for the small net;
    k_small and the tile kernels themselves sum the gradient in different orders (3e-5 apart, test_gpu_parity.py), so small_step 1 is
    not compared with small_step 0 -- and transform off against a context that never had one"""
    probe = _three_steps(name, None)
    n = float(np.sqrt(np.sum(probe[3][:-1].astype(np.float64) ** 2)))
    tf = {"global_clipnorm": n / 2}
    a = _three_steps(name, tf, [("fuse_tail", 1)])
    b = _three_steps(name, tf, [("fuse_tail", 0)])
    for i in range(4):
        assert np.array_equal(_bits(a[i]), _bits(b[i])), (name, "fuse_tail", i)
    assert not np.array_equal(a[0], probe[0])                 # (the clip did change the trajectory)
    if name == "small_nif_32x2":      # the same pair on the tile kernels (small_step 0), whose reduction is deferred and fused as well
        c = _three_steps(name, tf, [("small_step", 0), ("fuse_tail", 1)])
        d = _three_steps(name, tf, [("small_step", 0), ("fuse_tail", 0)])
        for i in range(4):
            assert np.array_equal(_bits(c[i]), _bits(d[i])), (name, "small_step 0: fuse_tail", i)
    # transform set and switched off again == never set (second context of the same process): the default path is untouched
    off = _three_steps(name, None)
    e = off[4]
    e.set_grad_transform(tf); e.set_grad_transform(None)
    never = _three_steps(name, None, never_set=True)
    for i in range(4):
        assert np.array_equal(_bits(off[i]), _bits(never[i])), (name, "off vs never", i)


# ---- 4. captured vs eager ------------------------------------------------------------------------------------------------------------
def test_captured_epoch_equals_eager_epoch_with_global_clipnorm():
    import nif_amd
    cs = {"input_dim": 1, "output_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    cp = {"input_dim": 1, "latent_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    x, y = O.synthetic_wave_batch(10000, seed=0)
    runs = {}
    for graph in (True, False):
        nif_amd.set_seed(4)
        m = nif_amd.NIF(cs, cp); model = m.build()
        model._graph_epochs = graph
        model.compile(nif_amd.Adam(1e-3, global_clipnorm=0.05), "mse")
        e = m._engine
        launches = []
        orig = e.graph_launch
        e.graph_launch = lambda gid, a: (launches.append(gid), orig(gid, a))
        h = model.fit(x, y, epochs=3, batch_size=512, shuffle=False, verbose=0)
        assert len(launches) == (3 if graph else 0)
        mm, vv, step = e.get_opt_state()
        assert step == 60
        runs[graph] = (np.array(h.history["loss"]), e.get_flat(), mm, vv, e.grad_norms()[1])
    for i, (a, b) in enumerate(zip(runs[True], runs[False])):
        assert np.array_equal(a, b), (i, a, b)
    assert runs[True][4] > 0.05                               # the clip was active at the last step
    # the same run without clipping differs
    nif_amd.set_seed(4)
    m = nif_amd.NIF(cs, cp); model = m.build(); model.compile(nif_amd.Adam(1e-3), "mse")
    model.fit(x, y, epochs=3, batch_size=512, shuffle=False, verbose=0)
    assert not np.array_equal(m._engine.get_flat(), runs[False][1])


# ---- 5. behind the all-reduce --------------------------------------------------------------------------------------------------------
_COMM_SCRIPT = r'''
import os, sys, ctypes as C, numpy as np
sys.path.insert(0, %(root)r)
import nif_amd
from nif_amd._lib import check
from tests import gradtf_ref as G
from tests.test_gpu_parity import _cfg
kind, cs, cp = _cfg("NIFMultiScale", 64, 2, 32, 2, 1, 1, 1, 1)
x, y = nif_amd.data.synthetic_wave_batch(2048, seed=1)
def make(l2=None, dev=0):
    nif_amd.set_seed(3)
    m = nif_amd.NIFMultiScale(cs, dict(cp, l2_reg=l2) if l2 else cp)
    if dev:
        from nif_amd.engine import Engine
        e = Engine(m._spec, device_id=dev); e.set_weights(m._init_weights)
        return m, e
    m.build()
    return m, m._engine
def run(e, comm, tf, steps=2):
    if comm:
        arr = (C.c_void_p * 1)(e.ctx); check(e.lib.nif_comm_init_all(arr, 1))
    e.set_grad_transform(tf)
    lion = nif_amd.optimizers.Lion(1e-3).as_opt()
    d_x, d_y = e.alloc(x.size), e.alloc(y.size); d_x.upload(x); d_y.upload(y)
    for _ in range(steps):
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, 2048, 2048)
        check(e.lib.nif_allreduce_grad(e.ctx))
        e.opt_step_dev(lion)
    return e.get_flat(), e.get_opt_slot(0)
tf = {"centralize": True, "gtcf": True, "clipnorm": 1e-3, "clipvalue": 1e-4}
a = run(make()[1], False, tf); b = run(make()[1], True, tf)
assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
# a zero-gradient step with an L2 regulariser: clipped on the regulariser term alone
l2 = 1e-2
m, e = make(l2)
n_pnet = m._n_pnet_params()
w0 = e.get_flat()
e.set_grad_transform({"global_clipnorm": 1e-3})
e.zero_grad()
e.opt_step_dev(nif_amd.optimizers.Lion(1e-3).as_opt())
out = np.empty((e.n_params + 1,), np.float32)
check(e.lib.nif_d2h(e.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(e.grad_dev_ptr()), out.nbytes))
g = np.zeros_like(w0); g[:n_pnet] = np.float32(2) * np.float32(l2) * w0[:n_pnet]
want64 = G.transform64(g, e.layout(), {"global_clipnorm": 1e-3})[0]
rel = np.abs(out[:-1] - want64).max() / np.abs(want64).max()
gn = e.grad_norms()[1]
print("zero-grad + L2: rel", rel, "norm", gn)
assert rel <= 1e-5 and abs(gn - np.sqrt(np.sum(g.astype(np.float64) ** 2))) <= 1e-5 * gn and gn > 1e-3
assert abs(np.sqrt(np.sum(out[:-1].astype(np.float64) ** 2)) - 1e-3) <= 1e-5 * 1e-3 and np.all(out[n_pnet:-1] == 0)
if e.lib.nif_device_count() >= 2 and %(two)d:
    (m0, e0), (m1, e1) = make(), make(dev=1)
    arr = (C.c_void_p * 2)(e0.ctx, e1.ctx); check(e0.lib.nif_comm_init_all(arr, 2))
    lion = nif_amd.optimizers.Lion(1e-3).as_opt()
    bufs = []
    for r, e_ in enumerate((e0, e1)):
        e_.set_grad_transform({"centralize": True, "gtcf": True, "clipnorm": 1e-3})
        d_x, d_y = e_.alloc(1024 * 2), e_.alloc(1024); d_x.upload(x[r * 1024:(r + 1) * 1024]); d_y.upload(y[r * 1024:(r + 1) * 1024])
        bufs.append((d_x, d_y))
    for _ in range(4):
        for e_, (d_x, d_y) in zip((e0, e1), bufs):
            e_.loss_grad_dev(d_x.at(0), d_y.at(0), None, 1024, 2048)
        check(e0.lib.nif_allreduce_grad_multi(arr, 2))
        for e_ in (e0, e1):
            e_.opt_step_dev(lion)
    assert np.array_equal(e0.get_flat().view(np.int32), e1.get_flat().view(np.int32))
    assert np.array_equal(e0.get_opt_slot(0).view(np.int32), e1.get_opt_slot(0).view(np.int32))
    print("TWO RANKS OK")
print("OK")
'''


def _run_child(two):
    r = subprocess.run([sys.executable, "-c", _COMM_SCRIPT % {"root": ROOT, "two": two}], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=300,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:]
    return r.stdout


def test_transform_sits_behind_the_all_reduce_world1():
    _run_child(0)


def test_two_ranks_stay_bit_identical():
    from nif_amd import _lib
    if _lib.load().nif_device_count() < 2:
        pytest.skip("one GPU visible")
    assert "TWO RANKS OK" in _run_child(1)


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["plain", "hessian"])
def test_fit_reports_the_norm_it_clipped_by(which):
    import nif_amd
    kind, cs, cp = _cfg("NIFMultiScale", 32, 2, 32, 2, 1, 2, 1, 1)
    nif_amd.set_seed(2)
    m = nif_amd.NIFMultiScale(cs, cp)
    model = m.build()
    rng = np.random.default_rng(0)
    B = 256
    x = rng.uniform(-1, 1, (B, 3)).astype(f32)
    y = rng.uniform(-1, 1, (B, 1)).astype(f32)
    c = 1e-2
    if which == "hessian":
        model = nif_amd.SobolevModel(nif_amd.HessianLayer(model, [0], [1, 2]))
        targets = [y, rng.uniform(-1, 1, (B, 1, 2)).astype(f32), rng.uniform(-1, 1, (B, 1, 2, 2)).astype(f32)]
        model.compile(nif_amd.Adam(1e-3, global_clipnorm=c), "mse", loss_weights=[1.0, 0.1, 0.01])
    else:
        targets = y
        model.compile(nif_amd.Adam(1e-3, global_clipnorm=c), "mse")
    e = m._engine
    seen = {}
    orig = e.adam_step_dev

    def step(adam):
        _, g = e.grad_read()                      # this step's untransformed gradient
        orig(adam)
        seen["g"], seen["norms"], seen["after"] = g, e.grad_norms(), _get_grad(e)[:-1]
    e.adam_step_dev = step
    model.fit(x, targets, epochs=1, batch_size=B, shuffle=False, verbose=0)
    layout = e.layout()
    _, per32, glob32 = G.transform32(seen["g"], layout, {})
    n64 = float(np.sqrt(np.sum(seen["g"].astype(np.float64) ** 2)))
    per, glob = seen["norms"]
    worst = {"norm_ulp": float(G.ulps([glob], [glob32]).max()), "norm_rel64": abs(glob - n64) / n64}
    print("WORST", which, worst, "norm", glob)
    assert worst["norm_ulp"] <= 2 and worst["norm_rel64"] <= 1e-5 and G.ulps(per, per32).max() <= 2
    after = float(np.sqrt(np.sum(seen["after"].astype(np.float64) ** 2)))
    assert after <= min(n64, c) * (1 + 1e-5)
    assert n64 > c                                # (clipping was active)
    e.adam_step_dev = orig
    # fit cleared the engine's transform: a later step is unclipped
    assert e.lib.nif_grad_transform_dev(e.ctx) == 0
