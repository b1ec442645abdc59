"""The L-BFGS closure in double precision on the device (nif_f64_*, k_f64.hip; TFPLBFGS / MSEClosure dtype="float64") against the
fp64 NumPy oracle.

Bars.  (a) FIXED: predictions, loss and every gradient tensor within 1e-10 relative L2 of oracle.loss_and_grad / oracle.forward.  One
float32 rounding is 6e-8, so this proves that no single-precision intermediate is anywhere on the path.  (b) TIGHT: the oracle has two
formulations of the same function, loss_and_grad (materialised [B, po] hypernetwork output) and planes_loss_and_grad (plane
formulation); their disagreement on the case's 'mse' evaluation -- the largest relative L2 difference over predictions, loss and the
gradient tensors -- is the oracle's own rounding spread for that configuration and batch.  The device has to stay within 100 x that
spread (floor 1e-13); 'mae' / 'huber' / 'log_cosh' take the bar of the 'mse' evaluation of the same configuration, batch and data.
The factor covers a different summation order (K blocks of 4, chunked batch) and a device math library whose sin / exp differ from
NumPy's in the last place, amplified through the cancelling dL/dz sums."""
import os

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests.cfgs import cfg_ms, cfg_nif

pytestmark = pytest.mark.gpu

CONFIGS = {
    "nif_swish": cfg_nif(),                                            # class NIF: swish, skip connections
    "nif_tanh_r2_so2": cfg_nif(n=20, r=2, so=2, si=2, act="tanh"),
    "ms_64x4": cfg_ms(n=64, L=4, nst=32, lst=2),                       # plain SIREN 64 x 4, SIREN ParameterNet
    "ms_res_32x2": cfg_ms(n=32, L=2, s_res=True),                      # resblock ShapeNet
    "ms_128x2": cfg_ms(n=128, L=2, nst=16),                            # 128 units
    "ms_30x2_nst30": cfg_ms(n=30, L=2, nst=30, lst=2),                 # 30 units: padding of the 16 x 16 tiles
    "ms_r3_si2_so2": cfg_ms(n=24, r=3, si=2, so=2, pi=2),              # latent_dim 3, si / so > 1
    "ms_pnet_shortcut": cfg_ms(n=16, nst=12, p_act="swish"),           # Dense + MLP_SimpleShortCut
    "ms_pnet_resnet_so2": cfg_ms(n=16, nst=12, p_act="swish", p_res=True, so=2),     # MLP_ResNet
    "ms_res_pnet_siren_res": cfg_ms(n=16, nst=12, s_res=True, p_res=True),           # SIREN_ResNet
}
# (configuration, batch, loss, sample weights, B_global or None): every configuration at 64 points with 'mse', and the other batch
# sizes / loss kinds / weights spread over them; 4099 points only where the oracle's [B, po] tensors stay small
CASES = [(name, 64, "mse", False, None) for name in CONFIGS] + [
    ("nif_swish", 4099, "mse", True, None),
    ("nif_swish", 7, "mae", False, None),
    ("nif_tanh_r2_so2", 257, "huber", True, None),
    ("nif_tanh_r2_so2", 4099, "log_cosh", False, None),
    ("ms_64x4", 257, "mse", True, 1000),                               # B_global != B_local
    ("ms_64x4", 7, "log_cosh", True, None),
    ("ms_res_32x2", 257, "mae", True, None),
    ("ms_res_32x2", 4099, "huber", False, None),
    ("ms_128x2", 7, "huber", True, None),
    ("ms_30x2_nst30", 257, "log_cosh", True, None),
    ("ms_30x2_nst30", 4099, "mse", False, None),
    ("ms_r3_si2_so2", 4099, "mae", True, None),
    ("ms_r3_si2_so2", 7, "mse", False, None),
    ("ms_pnet_shortcut", 257, "huber", False, None),
    ("ms_pnet_resnet_so2", 4099, "log_cosh", True, None),
    ("ms_res_pnet_siren_res", 257, "mae", False, None),
    ("ms_res_pnet_siren_res", 7, "huber", True, None),
]
WORST = {"ratio": 0.0, "case": None, "err": 0.0}


def _make(name, seed=0):
    import nif_amd
    kind, cs, cp = CONFIGS[name]
    nif_amd.set_seed(seed)
    m = getattr(nif_amd, kind)(cs, cp)
    model = m.build()
    return nif_amd, m, model, O.Spec(kind, cs, cp)


def _data(spec, B, seed, weights):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=(B, spec.pi + spec.si))            # float64, NOT representable in float32
    y = rng.uniform(-1.0, 1.0, size=(B, spec.so))
    sw = rng.uniform(0.5, 1.5, size=(B,)) if weights else None
    return x, y, sw


def _theta(model, seed):
    """a float64 point with bits below float32: the model's parameters, each moved by a relative 1e-9"""
    rng = np.random.default_rng(seed + 100)
    th = O.flatten([w.astype(np.float64) for w in model.get_weights()])
    return th * (1.0 + 1e-9 * rng.standard_normal(th.shape))


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a - b))


def _device_eval(e, theta, x, y, sw, bg, loss):
    d_x, d_y = e.alloc_f64(x.size), e.alloc_f64(y.size)
    d_sw = e.alloc_f64(sw.size) if sw is not None else None
    try:
        d_x.upload(x); d_y.upload(y)
        if d_sw is not None:
            d_sw.upload(sw)
        e.f64_set_flat(theta)
        e.set_loss(loss)
        e.f64_loss_grad_dev(d_x.at(0), d_y.at(0), d_sw.at(0) if d_sw is not None else None, x.shape[0], bg or x.shape[0])
        return e.f64_grad_read()
    finally:
        e.set_loss("mse")
        d_x.free(); d_y.free()
        if d_sw is not None:
            d_sw.free()


def _split(spec, flat):
    out, off = [], 0
    for nm, s in spec.param_shapes():
        k = int(np.prod(s))
        out.append((nm, flat[off:off + k])); off += k
    return out


@pytest.mark.parametrize("name,B,loss,weights,bg", CASES, ids=["%s-B%d-%s%s%s" % (c[0], c[1], c[2], "-sw" if c[3] else "", "-bg" if c[4] else "")
                                                               for c in CASES])
def test_closure_parity(name, B, loss, weights, bg):
    nif_amd, m, model, spec = _make(name)
    from nif_amd import _lib
    if B == 4099:
        assert B > _lib.F64_CHUNK_POINTS, "the 4099-point cases must span more than one chunk"
    e = m._engine
    x, y, sw = _data(spec, B, 7, weights)
    theta = _theta(model, 3)
    assert np.any(theta != theta.astype(np.float32).astype(np.float64))
    ws = O.unflatten(spec, theta)
    # the oracle's own spread on the 'mse' evaluation of this configuration, batch and data
    l_a, g_a = O.loss_and_grad(spec, ws, x, y, sw, batch_global=bg)
    l_b, g_b, u_b = O.planes_loss_and_grad(spec, ws, x, y, sw, batch_global=bg)
    u_ref = O.forward(spec, ws, x)
    spread = max([_rel(u_b, u_ref), abs(l_b - l_a) / abs(l_a)] + [_rel(b_, a_) for a_, b_ in zip(g_a, g_b)])
    bar = max(100.0 * spread, 1e-13)
    l_ref, g_ref = (l_a, g_a) if loss == "mse" else O.loss_and_grad(spec, ws, x, y, sw, batch_global=bg, loss=loss)
    l_dev, g_dev = _device_eval(e, theta, x, y, sw, bg, loss)
    u_dev = e.f64_forward(x)
    assert u_dev.dtype == np.float64 and g_dev.dtype == np.float64
    errs = {"predictions": _rel(u_dev, u_ref), "loss": abs(l_dev - l_ref) / abs(l_ref)}
    for (nm, gd), gr in zip(_split(spec, g_dev), g_ref):
        errs[nm] = _rel(gd, gr)
    worst = max(errs, key=errs.get)
    ratio = errs[worst] / max(spread, 1e-15)
    print("f64 parity %s B=%d %s: oracle spread %.2e, bar %.2e, worst %s %.2e (%.1f x spread)" % (name, B, loss, spread, bar, worst, errs[worst], ratio))
    if ratio > WORST["ratio"]:
        WORST.update(ratio=ratio, case="%s-B%d-%s" % (name, B, loss), err=errs[worst])
    print("f64 parity worst ratio so far: %.1f x (%s, %.2e)" % (WORST["ratio"], WORST["case"], WORST["err"]))
    for k, v in errs.items():
        assert v <= 1e-10, "%s: %s is %.3e from the fp64 oracle (fixed bar 1e-10)" % (name, k, v)
    for k, v in errs.items():
        assert v <= bar, "%s: %s is %.3e from the fp64 oracle, over 100 x the oracle's own spread %.2e" % (name, k, v, spread)


def test_bitwise_repeatability():
    nif_amd, m, model, spec = _make("ms_30x2_nst30")
    e = m._engine
    x, y, sw = _data(spec, 4099, 11, True)
    theta = _theta(model, 5)
    l1, g1 = _device_eval(e, theta, x, y, sw, None, "mse")
    l2, g2 = _device_eval(e, theta, x, y, sw, None, "mse")
    assert np.float64(l1).tobytes() == np.float64(l2).tobytes() and g1.tobytes() == g2.tobytes()
    model.compile(nif_amd.Adam(1e-3), loss="mse")                      # an unrelated float32 step in between
    model.fit(x.astype(np.float32), y.astype(np.float32), epochs=1, batch_size=512, verbose=0)
    l3, g3 = _device_eval(e, theta, x, y, sw, None, "mse")
    assert np.float64(l1).tobytes() == np.float64(l3).tobytes() and g1.tobytes() == g3.tobytes()


# Central difference of step h = 1e-5 along a random unit direction: truncation ~ h^2 f3 / 6 (f3: the third directional derivative)
# and rounding ~ 1e-16 f / (h |g.d|).  At these (initialised) weights f ~ 0.3 .. 1 and |g.d| ~ 3e-4 .. 1, so rounding stays below 1e-8
# and truncation below 1e-9 of g.d.  The SIREN case (omega_0 = 30) needs no smaller step: its hidden kernels are drawn with scale
# 1 / omega_0, which keeps the slopes of the phases O(1) (the fp64 oracle's own central difference at this h agrees with its gradient
# to 1e-9 on all three configurations).
H_FD = 1e-5


@pytest.mark.parametrize("name", ["nif_swish", "nif_tanh_r2_so2", "ms_30x2_nst30"])
def test_directional_derivative(name):
    h = H_FD
    nif_amd, m, model, spec = _make(name)
    x, y, _ = _data(spec, 257, 13, False)
    rng = np.random.default_rng(17)
    t64 = nif_amd.optimizers.TFPLBFGS(model, "mse", x, y, display_epoch=1 << 62, dtype="float64")
    theta = t64.position
    d = rng.standard_normal(theta.shape); d /= np.linalg.norm(d)

    def check(f):
        _, g = f(theta)
        fd = (f(theta + h * d)[0] - f(theta - h * d)[0]) / (2.0 * h)
        gd = float(g.dot(d))
        return abs(fd - gd) / abs(gd), fd, gd
    rel64, fd, gd = check(t64._f)
    print("directional derivative %s: float64 closure fd %.12e g.d %.12e rel %.2e" % (name, fd, gd, rel64))
    t32 = nif_amd.optimizers.TFPLBFGS(model, "mse", x, y, display_epoch=1 << 62)
    rel32, fd32, gd32 = check(t32._f)
    print("directional derivative %s: float32 closure fd %.12e g.d %.12e rel %.2e" % (name, fd32, gd32, rel32))
    assert rel64 <= 1e-7
    assert rel32 > 1e-7, "the float32 closure is not expected to resolve a central difference of step %g" % h


def _wave():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "traveling_wave.npz"))["data"]
    data, _, _ = O.standard_normalize(d.astype(np.float64))
    return np.ascontiguousarray(data[:, :2]), np.ascontiguousarray(data[:, 2:3])


def test_trajectory_against_the_oracle():
    import nif_amd
    from nif_amd.optimizers import LBFGSMinimizer, TFPLBFGS
    x, y = _wave()
    assert x.shape[0] == 2000
    kind, cs, cp = cfg_ms(n=16, L=2, nst=12, lst=2, p_act="swish")
    nif_amd.set_seed(1)
    model = nif_amd.NIFMultiScale(cs, cp).build()
    spec = O.Spec(kind, cs, cp)
    model.compile(nif_amd.Adam(1e-3), loss="mse")
    model.fit(x.astype(np.float32), y.astype(np.float32), epochs=5, batch_size=500, verbose=0)
    tuner = TFPLBFGS(model, "mse", x, y, display_epoch=1 << 62, dtype="float64")
    theta0 = tuner.position
    n_ref = [0]

    def f_ref(theta):
        n_ref[0] += 1
        loss, g = O.loss_and_grad(spec, O.unflatten(spec, theta), x, y)
        return float(loss), O.flatten(g)
    xd, sd, xr, sr = theta0.copy(), None, theta0.copy(), None
    md, mr = LBFGSMinimizer(tuner._f), LBFGSMinimizer(f_ref)
    for it in range(5):
        xd, fd, sd, dd = md.run_resumable(xd, 1, sd)
        xr, fr, sr, dr = mr.run_resumable(xr, 1, sr)
        print("trajectory iteration %d: device %.15e (%d evaluations), oracle %.15e (%d), rel %.2e"
              % (it + 1, fd, len(tuner.history["loss"]), fr, n_ref[0], abs(fd - fr) / abs(fr)))
        assert dd == 1 and dr == 1
        assert abs(fd - fr) <= 1e-9 * abs(fr)
        assert len(tuner.history["loss"]) == n_ref[0]


def test_surface_end_to_end():
    import nif_amd
    from nif_amd.optimizers import TFPLBFGS
    x, y = _wave()
    kind, cs, cp = cfg_ms(n=16, L=2, nst=12, lst=2, p_act="swish")
    nif_amd.set_seed(2)
    model = nif_amd.NIFMultiScale(cs, cp).build()
    spec = O.Spec(kind, cs, cp)
    model.compile(nif_amd.Adam(1e-3), loss="mse")
    model.fit(x.astype(np.float32), y.astype(np.float32), epochs=3, batch_size=500, verbose=0)
    l0 = model.evaluate(x.astype(np.float32), y.astype(np.float32))
    tuner = TFPLBFGS(model, "mse", x, y, display_epoch=1 << 62, dtype="float64")
    hist = tuner.minimize(rounds=2, max_iter=5)
    assert len(hist["loss"]) > 2 and np.all(np.isfinite(hist["loss"])) and len(hist["iteration"]) == len(hist["loss"])
    assert min(hist["loss"]) < l0
    pos = tuner.position
    assert pos.dtype == np.float64 and np.any(pos != pos.astype(np.float32).astype(np.float64))
    flat = O.flatten(model.get_weights())
    assert flat.dtype == np.float32 and np.array_equal(flat, pos.astype(np.float32))
    u = model.predict(x.astype(np.float32))
    u_ref = O.forward(spec, [w.astype(np.float64) for w in model.get_weights()], x.astype(np.float32).astype(np.float64))
    assert _rel(u, u_ref) < 1e-5
    t32 = TFPLBFGS(model, "mse", x.astype(np.float32), y.astype(np.float32), display_epoch=1 << 62)      # the float32 tuner still works
    h32 = t32.minimize(rounds=1, max_iter=3)
    assert len(h32["loss"]) >= 1 and np.all(np.isfinite(h32["loss"]))


def test_refusals_on_the_device():
    import nif_amd
    from tests.cfgs import cfg_ll
    _, cs, cp = cfg_ll()
    ll = nif_amd.NIFMultiScaleLastLayerParameterized(cs, cp)
    ll.build()
    with pytest.raises(nif_amd.NifError, match="NIFMultiScaleLastLayerParameterized"):
        ll._engine.f64_set_flat(np.zeros(ll._engine.n_params))
    _, cs, cp = cfg_ms()
    mp = nif_amd.NIFMultiScale(cs, cp, mixed_policy="mixed_bfloat16")
    mp.build()
    with pytest.raises(nif_amd.NifError, match="mixed policy"):
        mp._engine.f64_set_flat(np.zeros(mp._engine.n_params))
    ok = nif_amd.NIFMultiScale(cs, cp)
    ok.build()
    with pytest.raises(nif_amd.NifError, match="before nif_f64_set_params"):
        ok._engine.f64_forward(np.zeros((4, 2)))
