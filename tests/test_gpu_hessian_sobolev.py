"""The second-order Sobolev step on the GPU (nif_sobolev2_loss_grad_dev, k_sob<.., HESS>): SobolevModel(HessianLayer(...)) against
the fp64 autograd reference (tests/hess_ref.py), its summation properties, predict / fit through the public model, and training."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import hess_ref

pytestmark = pytest.mark.gpu


def _cfg(kind, n, L, nst, lst, r, si, so, pi, s_res=False):
    cs = {"input_dim": si, "output_dim": so, "units": n, "nlayers": L, "use_resblock": s_res,
          "connectivity": "last_layer" if kind == "LL" else "full", "omega_0": 30.0, "weight_init_factor": 0.01}
    cp = {"input_dim": pi, "latent_dim": r, "units": nst, "nlayers": lst, "activation": "sine", "use_resblock": False,
          "omega_0": 30.0}
    return ("NIFMultiScaleLastLayerParameterized" if kind == "LL" else "NIFMultiScale"), cs, cp


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def _build(cfg, seed=0):
    import nif_amd
    kind, cs, cp = cfg
    nif_amd.set_seed(seed)
    m = getattr(nif_amd, kind)(cs, cp)
    return m, m.build()


def _data(kind, cs, cp, ws, B, y_index, x_index, seed):
    """inputs, targets (random, d2ydx2 NOT symmetric, on the scale of the model's own derivatives) and sample weights"""
    rng = np.random.default_rng(seed)
    pi, si, so = cp["input_dim"], cs["input_dim"], cs["output_dim"]
    x = rng.uniform(-1, 1, size=(B, pi + si)).astype(np.float32)
    spec = O.Spec(kind, cs, cp)
    u, J, H = O.hessian_analytic(spec, [w.astype(np.float64) for w in ws], x.astype(np.float64), y_index, x_index)
    ny, nx = len(y_index), len(x_index)
    y = (u + np.std(u) * rng.standard_normal(u.shape)).astype(np.float32)
    g = (J + np.std(J) * rng.standard_normal((B, ny, nx))).astype(np.float32)
    t = (H + np.std(H) * rng.standard_normal((B, ny, nx, nx))).astype(np.float32)
    sw = rng.uniform(0.2, 2.0, size=(B,)).astype(np.float32)
    return x, y, g, t, sw


# name: (cfg, B, y_index, x_index (coordinate positions, pi added), loss, sample weights, loss_weights)
CASES = {
    "ms32x2_si1": (_cfg("MS", 32, 2, 16, 1, 1, 1, 1, 1), 7, [0], [0], "mse", False, (1.0, 0.5, 0.3)),
    "ms64x3_si2_shuffled": (_cfg("MS", 64, 3, 16, 1, 2, 2, 1, 1), 257, [0], [1, 0], "huber", True, (2.0, 0.7, 0.2)),
    "ms_res32x2_si3_subset": (_cfg("MS", 32, 2, 16, 1, 1, 3, 2, 1, s_res=True), 1031, [1], [2, 0], "mse", True, (1.5, 1.0, 0.5)),
    "ms_res64x2_si3_all": (_cfg("MS", 64, 2, 16, 1, 1, 3, 1, 1, s_res=True), 64, [0], [0, 2, 1], "mse", False, (1.0, 0.1, 0.05)),
    # 128 units, 6 matrices, latent_dim 5: one plane buffer in LDS
    "ms128x6_r5_onebuf": (_cfg("MS", 128, 6, 32, 2, 5, 2, 1, 1), 64, [0], [0, 1], "mse", True, (1.0, 0.3, 0.1)),
    "ll32x2_r3_so2": (_cfg("LL", 32, 2, 32, 1, 3, 2, 2, 1), 257, [0], [1, 0], "huber", True, (2.0, 0.5, 0.25)),
    "ll_res48x2_r4_si3": (_cfg("LL", 48, 2, 40, 2, 4, 3, 1, 2, s_res=True), 64, [0], [0, 1, 2], "mse", False, (1.0, 0.2, 0.1)),
}
MEASURED = {}


def _full_rows(t, so, y_index, tail):
    full = np.zeros((t.shape[0], so) + tail, dtype=np.float32)
    full[:, y_index] = t
    return full.reshape(t.shape[0], -1)


def _entry(e, x, y, g, t, sw, B, Bg, y_index, x_index, w):
    """nif_sobolev2_loss_grad_dev on device copies of host rows (targets in [so][nx] / [so][nx][nx] rows)"""
    from nif_amd.engine import DeviceArray
    so = y.shape[1]
    nx = len(x_index)
    gr, tr = _full_rows(g, so, y_index, (nx,)), _full_rows(t, so, y_index, (nx, nx))
    w0, w1, w2 = w
    swv = (w0 * (sw if sw is not None else np.ones((x.shape[0],), np.float32))).astype(np.float32)
    arrs = [DeviceArray(e, a.size) for a in (x, y, gr, tr, swv)]
    for d, a in zip(arrs, (x, y, gr, tr, swv)):
        d.upload(np.ascontiguousarray(a))
    try:
        e.sobolev2_loss_grad_dev(arrs[0].at(0), arrs[1].at(0), arrs[2].at(0), arrs[3].at(0), arrs[4].at(0), B, Bg, x_index,
                                 w1 / w0, w2 / w0, y_index)
        return e.grad_read()
    finally:
        for d in arrs:
            d.free()


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_matches_fp64_autograd(name):
    cfg, B, yi, xi_c, loss, use_sw, w = CASES[name]
    kind, cs, cp = cfg
    m, model = _build(cfg, seed=3)
    pi = cp["input_dim"]
    xi = [pi + c for c in xi_c]
    ws = model.get_weights()
    x, y, g, t, sw = _data(kind, cs, cp, ws, B, yi, xi, seed=11)
    sw = sw if use_sw else None
    e = m._engine
    e.set_loss(loss)
    lg, gg = _entry(e, x, y, g, t, sw, B, B, yi, xi, w)
    lr, gr, _, _, _ = hess_ref.sobolev2_loss_and_grad(kind, cs, cp, [a.astype(np.float64) for a in ws], x.astype(np.float64), y, g, t,
                                                     yi, xi, w, sw, loss)
    errs, off = [], 0
    for a in gr:
        errs.append(_rel(gg[off:off + a.size].reshape(a.shape), a) if np.linalg.norm(a) > 0 else float(np.abs(gg[off:off + a.size]).max()))
        off += a.size
    assert off == gg.size
    le = abs(lg - lr) / abs(lr)
    MEASURED[name] = (le, max(errs))
    print("%s: loss rel %.2e, worst gradient tensor rel %.2e" % (name, le, max(errs)))
    assert le <= 1e-4, (lg, lr)
    assert max(errs) <= 1e-3, errs


def test_repeat_bit_identical_and_half_batches_add_up():
    cfg, B, yi, xi_c, loss, _, w = CASES["ms64x3_si2_shuffled"]
    kind, cs, cp = cfg
    m, model = _build(cfg, seed=4)
    xi = [cp["input_dim"] + c for c in xi_c]
    x, y, g, t, sw = _data(kind, cs, cp, model.get_weights(), B, yi, xi, seed=5)
    e = m._engine
    e.set_loss(loss)
    l1, g1 = _entry(e, x, y, g, t, sw, B, B, yi, xi, w)
    l2, g2 = _entry(e, x, y, g, t, sw, B, B, yi, xi, w)
    assert l1 == l2 and np.array_equal(g1, g2)
    h = 128       # (a multiple of 32 points: both halves are whole tiles)
    la, ga = _entry(e, x[:h], y[:h], g[:h], t[:h], sw[:h], h, B, yi, xi, w)
    lb, gb = _entry(e, x[h:], y[h:], g[h:], t[h:], sw[h:], B - h, B, yi, xi, w)
    assert abs((la + lb) - l1) <= 1e-5 * abs(l1)
    assert _rel(ga.astype(np.float64) + gb, g1.astype(np.float64)) <= 1e-5


def test_predict_is_the_hessian_layer():
    import nif_amd
    cfg = _cfg("MS", 64, 3, 16, 1, 2, 2, 2, 1)
    m, model = _build(cfg, seed=6)
    x = np.random.default_rng(0).uniform(-1, 1, size=(300, 3)).astype(np.float32)
    for yi, xi in (([0, 1], [1, 2]), ([1], [2, 1])):
        sm = nif_amd.SobolevModel(nif_amd.HessianLayer(model, yi, xi))
        got = sm.predict(x)
        want = nif_amd.HessianLayer(model, yi, xi)(x)
        assert len(got) == 3
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


def test_fit_is_the_entry_plus_adam():
    import nif_amd
    cfg, B, yi, xi_c, loss, _, w = CASES["ms64x3_si2_shuffled"]
    kind, cs, cp = cfg
    xi = [cp["input_dim"] + c for c in xi_c]
    bs = 96
    res = []
    for how in ("fit", "loop"):
        m, model = _build(cfg, seed=8)
        x, y, g, t, sw = _data(kind, cs, cp, model.get_weights(), B, yi, xi, seed=9)
        sm = nif_amd.SobolevModel(nif_amd.HessianLayer(model, yi, xi))
        sm.compile(nif_amd.Adam(1e-3), loss, loss_weights=list(w))
        if how == "fit":
            h = sm.fit(x, [y, g, t], batch_size=bs, epochs=1, shuffle=False, sample_weight=sw, verbose=0)
            assert np.isfinite(h.history["loss"][0])
            ev = sm.evaluate(x, [y, g, t], sample_weight=sw)
            assert np.isfinite(ev)
        else:
            e = m._engine
            e.set_loss(loss)
            adam = nif_amd.Adam(1e-3).as_struct()
            for lo in range(0, B, bs):
                hi = min(B, lo + bs)
                _entry(e, x[lo:hi], y[lo:hi], g[lo:hi], t[lo:hi], sw[lo:hi], hi - lo, hi - lo, yi, xi, w)
                e.adam_step_dev(adam)
        res.append(np.concatenate([a.ravel() for a in model.get_weights()]))
    assert np.array_equal(res[0], res[1])


def test_evaluate_is_the_entry_loss():
    import nif_amd
    cfg, B, yi, xi_c, loss, _, w = CASES["ll32x2_r3_so2"]
    kind, cs, cp = cfg
    xi = [cp["input_dim"] + c for c in xi_c]
    m, model = _build(cfg, seed=2)
    x, y, g, t, sw = _data(kind, cs, cp, model.get_weights(), B, yi, xi, seed=3)
    sm = nif_amd.SobolevModel(nif_amd.HessianLayer(model, yi, xi))
    sm.compile(nif_amd.Adam(1e-3), loss, loss_weights=list(w))
    ev = sm.evaluate(x, [y, g, t], sample_weight=sw)
    lr = hess_ref.sobolev2_loss_and_grad(kind, cs, cp, [a.astype(np.float64) for a in model.get_weights()], x.astype(np.float64),
                                         y, g, t, yi, xi, w, sw, loss, want_grad=False)[0]
    assert abs(ev - lr) <= 1e-4 * abs(lr)


def test_not_capturable():
    import nif_amd
    from nif_amd import _lib
    cfg, B, yi, xi_c, loss, _, w = CASES["ms32x2_si1"]
    kind, cs, cp = cfg
    xi = [cp["input_dim"] + c for c in xi_c]
    m, model = _build(cfg)
    x, y, g, t, sw = _data(kind, cs, cp, model.get_weights(), B, yi, xi, seed=1)
    e = m._engine
    e.reserve(B, 3)
    _entry(e, x, y, g, t, sw, B, B, yi, xi, w)        # (workspaces sized and arrays in place before the capture)
    from nif_amd.engine import DeviceArray
    d = [DeviceArray(e, a.size) for a in (x, y, g, t)]
    for da, a in zip(d, (x, y, g, t)):
        da.upload(np.ascontiguousarray(a))
    e.sync()
    e.graph_begin()
    try:
        with pytest.raises(_lib.NifError, match="graph capture"):
            e.sobolev2_loss_grad_dev(d[0].at(0), d[1].at(0), d[2].at(0), d[3].at(0), None, B, B, xi, 1.0, 1.0, yi)
    finally:
        gid = e.graph_end()
        if gid is not None and gid >= 0:
            e.graph_destroy(gid)
    for da in d:
        da.free()


def test_training_lowers_the_hessian_term():
    """u = sin(2 x0) cos(3 x1) on [-1, 1]^2: analytic gradient and Hessian; 300 Adam steps of the three-output model"""
    import nif_amd
    cfg = _cfg("MS", 32, 2, 16, 1, 1, 2, 1, 1)
    kind, cs, cp = cfg
    cs = dict(cs, omega_0=3.0)
    cp = dict(cp, omega_0=3.0)
    nif_amd.set_seed(0)
    m = nif_amd.NIFMultiScale(cs, cp)
    model = m.build()
    rng = np.random.default_rng(0)
    B = 2048
    x = np.concatenate([rng.uniform(-1, 1, (B, 1)) * 0.0, rng.uniform(-1, 1, (B, 2))], axis=1)
    a, b = x[:, 1], x[:, 2]
    u = np.sin(2 * a) * np.cos(3 * b)
    J = np.stack([2 * np.cos(2 * a) * np.cos(3 * b), -3 * np.sin(2 * a) * np.sin(3 * b)], 1)[:, None, :]
    H = np.stack([np.stack([-4 * u, -6 * np.cos(2 * a) * np.sin(3 * b)], 1),
                  np.stack([-6 * np.cos(2 * a) * np.sin(3 * b), -9 * u], 1)], 1)[:, None, :, :]
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    x, u, J, H = f(x), f(u[:, None]), f(J), f(H)
    sm = nif_amd.SobolevModel(nif_amd.HessianLayer(model, [0], [1, 2]))
    sm.compile(nif_amd.Adam(1e-3), "mse", loss_weights=[1.0, 0.1, 0.01])

    def hess_term():
        _, _, Hp = sm.predict(x)
        return float(np.mean((Hp - H) ** 2))

    h0 = hess_term()
    sm.fit(x, [u, J, H], batch_size=B, epochs=300, shuffle=False, verbose=0)
    h1 = hess_term()
    print("Hessian term %.4e -> %.4e (%.1fx)" % (h0, h1, h0 / h1))
    assert h1 * 10.0 <= h0, (h0, h1)
