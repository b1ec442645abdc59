"""SobolevModel(HessianLayer(...)) without a GPU: the fp64 reference of the second-order step (tests/hess_ref.py) against the
oracle's analytic Hessian and central differences, and the model's host logic on an engine double (target layout, loss weights,
what v1 refuses)."""
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import hess_ref
from tests.doubles import OracleEngine


def _cfg(kind, n, L, r, si, so, pi, s_res=False):
    cs = {"input_dim": si, "output_dim": so, "units": n, "nlayers": L, "use_resblock": s_res,
          "connectivity": "last_layer" if kind == "NIFMultiScaleLastLayerParameterized" else "full", "omega_0": 30.0,
          "weight_init_factor": 0.01}
    cp = {"input_dim": pi, "latent_dim": r, "units": 8, "nlayers": 1, "activation": "sine", "use_resblock": False, "omega_0": 30.0}
    return kind, cs, cp


SMALL = {
    "ms_plain": _cfg("NIFMultiScale", 8, 2, 2, 3, 2, 1),
    "ms_res": _cfg("NIFMultiScale", 8, 2, 1, 2, 1, 1, s_res=True),
    "ll": _cfg("NIFMultiScaleLastLayerParameterized", 8, 2, 2, 2, 2, 1),
}


def _weights(kind, cs, cp, seed=0):
    o = O.Spec(kind, cs, cp)
    return o, [np.asarray(w, dtype=np.float64) for w in O.init_weights(o, np.random.default_rng(seed))]


def _problem(name, B=9, seed=0):
    kind, cs, cp = SMALL[name]
    o, ws = _weights(kind, cs, cp, seed)
    rng = np.random.default_rng(seed + 1)
    pi, si, so = cp["input_dim"], cs["input_dim"], cs["output_dim"]
    x = rng.uniform(-1, 1, size=(B, pi + si))
    yi = list(range(so))[::-1]
    xi = [pi + c for c in range(si)][::-1]
    ny, nx = len(yi), len(xi)
    y = rng.standard_normal((B, so))
    g = rng.standard_normal((B, ny, nx))
    t = rng.standard_normal((B, ny, nx, nx))       # not symmetric
    sw = rng.uniform(0.5, 1.5, size=(B,))
    return kind, cs, cp, o, ws, x, y, g, t, sw, yi, xi


@pytest.mark.parametrize("name", sorted(SMALL))
def test_reference_hessian_is_the_oracles(name):
    kind, cs, cp, o, ws, x, y, g, t, sw, yi, xi = _problem(name)
    _, _, u, J, H = hess_ref.sobolev2_loss_and_grad(kind, cs, cp, ws, x, y, g, t, yi, xi, want_grad=False)
    ur, Jr, Hr = O.hessian_analytic(o, ws, x, yi, xi)
    assert np.abs(u - ur).max() <= 1e-10 * max(1.0, np.abs(ur).max())
    assert np.abs(J - Jr).max() <= 1e-10 * max(1.0, np.abs(Jr).max())
    assert np.abs(H - Hr).max() <= 1e-10 * max(1.0, np.abs(Hr).max())


@pytest.mark.parametrize("name,loss", [("ms_plain", "mse"), ("ms_res", "huber"), ("ll", "log_cosh"), ("ms_plain", "mae")])
def test_reference_gradient_matches_central_differences(name, loss):
    kind, cs, cp, o, ws, x, y, g, t, sw, yi, xi = _problem(name, B=5)
    lw = (1.3, 0.4, 0.2)
    yi2, xi2 = yi[:1], xi[:2]
    g2, t2 = g[:, :1, :2], t[:, :1, :2, :2]
    L, grads, _, _, _ = hess_ref.sobolev2_loss_and_grad(kind, cs, cp, ws, x, y, g2, t2, yi2, xi2, lw, sw, loss)
    rng = np.random.default_rng(7)
    f = lambda w: hess_ref.sobolev2_loss_and_grad(kind, cs, cp, w, x, y, g2, t2, yi2, xi2, lw, sw, loss, want_grad=False)[0]
    for _ in range(3):
        d = [rng.standard_normal(w.shape) for w in ws]
        eps = 1e-6
        fd = (f([w + eps * v for w, v in zip(ws, d)]) - f([w - eps * v for w, v in zip(ws, d)])) / (2 * eps)
        an = sum(float(np.sum(gw * v)) for gw, v in zip(grads, d))
        assert abs(fd - an) <= 1e-5 * max(abs(an), 1e-8 * abs(L)), (fd, an)


class HessianEngine(OracleEngine):
    """the double with the three-output model's step: records what the model hands the engine, computes the step with hess_ref"""

    def __init__(self, kind, cs, cp, o, ws):
        OracleEngine.__init__(self, o, ws)
        self.kind, self.cs, self.cp = kind, cs, cp
        self.steps = []
        self.loss_name = "mse"

    def set_loss(self, name):
        self.loss_name = name

    def alloc(self, n):
        from tests.doubles import _HostArray
        return _HostArray(n)

    def sobolev2_loss_grad_dev(self, d_x, d_y, d_g, d_h, d_sw, b, bg, x_index, w_jac, w_hess, y_index=None):
        o = self.o
        ncol, so, nx = o.pi + o.si, o.so, len(x_index)
        take = lambda d, n: d[0][d[1]:d[1] + n].astype(np.float64)
        x = take(d_x, b * ncol).reshape(b, ncol)
        y = take(d_y, b * so).reshape(b, so)
        g = take(d_g, b * so * nx).reshape(b, so, nx)
        h = take(d_h, b * so * nx * nx).reshape(b, so, nx, nx)
        sw = None if d_sw is None else take(d_sw, b)
        self.steps.append(dict(x=x, y=y, g=g, h=h, sw=sw, b=b, bg=bg, x_index=list(x_index), w_jac=w_jac, w_hess=w_hess,
                               y_index=y_index))
        yi = list(range(so)) if y_index is None else list(y_index)
        L, grads, _, _, _ = hess_ref.sobolev2_loss_and_grad(self.kind, self.cs, self.cp, O.unflatten(o, self.theta), x, y,
                                                           g[:, yi], h[:, yi], yi, x_index, (1.0, w_jac, w_hess), sw,
                                                           self.loss_name)
        s = b / float(bg)
        self.grad_buf[:-1] = s * O.flatten(grads); self.grad_buf[-1] = s * L
        self.reg_applied = False

    def hessian(self, inputs, y_index, x_index):
        x = np.asarray(inputs, dtype=np.float64)
        u, J, H = O.hessian_analytic(self.o, O.unflatten(self.o, self.theta), x, list(y_index), list(x_index))
        return u.astype(np.float32), J.astype(np.float32), H.astype(np.float32)


def _double(name="ms_plain", policy="float32"):
    import nif_amd
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    kind, cs, cp = SMALL[name]
    o, ws = _weights(kind, cs, cp)
    eng = HessianEngine(kind, cs, cp, o, ws)
    owner = types.SimpleNamespace(_spec=Spec(kind, cs, cp), _engine=eng, mixed_policy_name=policy)
    return nif_amd, Model(owner, "full"), eng, kind, cs, cp


def test_three_output_model_builds_and_lays_out_targets():
    nif_amd, model, eng, kind, cs, cp = _double("ms_plain")
    pi = cp["input_dim"]
    yi, xi = [1], [pi + 2, pi]
    sm = nif_amd.SobolevModel(nif_amd.HessianLayer(model, yi, xi))
    assert sm.loss_weights == [1.0, 1.0, 1.0]
    sm.compile(nif_amd.Adam(1e-3), "mse", loss_weights=[2.0, 0.5, 0.25])
    rng = np.random.default_rng(3)
    B, so = 6, cs["output_dim"]
    x = rng.uniform(-1, 1, (B, pi + cs["input_dim"])).astype(np.float32)
    y = rng.standard_normal((B, so)).astype(np.float32)
    g = rng.standard_normal((B, 1, 2)).astype(np.float32)
    t = rng.standard_normal((B, 1, 2, 2)).astype(np.float32)
    sw = rng.uniform(0.5, 1.5, B).astype(np.float32)
    sm.fit(x, [y, g, t], batch_size=B, epochs=1, shuffle=False, sample_weight=sw, verbose=0)
    st = eng.steps[0]
    assert st["b"] == B and st["bg"] == B and st["x_index"] == xi and list(st["y_index"]) == yi
    assert st["w_jac"] == pytest.approx(0.25) and st["w_hess"] == pytest.approx(0.125)
    np.testing.assert_allclose(st["sw"], 2.0 * sw, rtol=1e-6)                # w0 rides on the sample weights
    assert st["h"].shape == (B, so, 2, 2)
    np.testing.assert_array_equal(st["h"][:, 1], t[:, 0])                     # [so][nx][nx] rows, the listed output in place
    np.testing.assert_array_equal(st["h"][:, 0], 0.0)
    np.testing.assert_array_equal(st["g"][:, 1], g[:, 0])
    # w0 = 1 and no sample weights: nothing rides on them
    sm.compile(nif_amd.Adam(1e-3), "mse", loss_weights=[1.0, 0.0, 3.0])
    sm.fit(x, [y, g, t], batch_size=B, epochs=1, shuffle=False, verbose=0)
    assert eng.steps[-1]["sw"] is None and eng.steps[-1]["w_hess"] == 3.0
    out = sm.predict(x)
    assert len(out) == 3 and out[2].shape == (B, 1, 2, 2)


def test_target_shapes_are_validated():
    nif_amd, model, eng, kind, cs, cp = _double("ms_plain")
    pi = cp["input_dim"]
    sm = nif_amd.SobolevModel(nif_amd.HessianLayer(model, [0, 1], [pi, pi + 1]))
    sm.compile(nif_amd.Adam(1e-3), "mse", loss_weights=[1.0, 1.0, 1.0])
    B = 4
    x = np.zeros((B, pi + cs["input_dim"]), np.float32)
    y, g = np.zeros((B, 2), np.float32), np.zeros((B, 2, 2), np.float32)
    with pytest.raises(ValueError, match="three outputs"):
        sm.fit(x, [y, g], epochs=1, verbose=0)
    with pytest.raises(ValueError, match="d2ydx2 must have shape"):
        sm.fit(x, [y, g, np.zeros((B, 2, 2, 3), np.float32)], epochs=1, verbose=0)


def test_loss_weights_and_metrics():
    nif_amd, model, eng, kind, cs, cp = _double("ms_plain")
    pi = cp["input_dim"]
    sm = nif_amd.SobolevModel(nif_amd.HessianLayer(model, [0], [pi]))
    for lw in ([1.0, 0.1], [0.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, -0.5], [1.0, 1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="loss_weights"):
            sm.compile(nif_amd.Adam(1e-3), "mse", loss_weights=lw)
    with pytest.raises(NotImplementedError, match="metrics"):
        sm.compile(nif_amd.Adam(1e-3), "mse", loss_weights=[1.0, 1.0, 1.0], metrics=["mae"])


def test_refused_cases_name_what_is_built():
    import nif_amd
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    built = "NIFMultiScale"
    # a parameter column
    nif_amd_, model, eng, kind, cs, cp = _double("ms_plain")
    with pytest.raises(NotImplementedError, match="parameter columns.*" + built):
        nif_amd.SobolevModel(nif_amd.HessianLayer(model, [0], [0, cp["input_dim"]]))
    # class NIF
    cs_n = {"input_dim": 1, "output_dim": 1, "units": 8, "nlayers": 2, "activation": "tanh"}
    cp_n = {"input_dim": 1, "latent_dim": 1, "units": 8, "nlayers": 1, "activation": "tanh"}
    m_nif = nif_amd.NIF(cs_n, cp_n).build()
    with pytest.raises(NotImplementedError, match="class NIF.*" + built):
        nif_amd.SobolevModel(nif_amd.HessianLayer(m_nif, [0], [1]))
    # mixed policies
    for pol in ("mixed_bfloat16", "mixed_float16"):
        _, model_p, _, _, _, cp_p = _double("ms_plain", policy=pol)
        with pytest.raises(NotImplementedError, match="mixed_policy.*" + built):
            nif_amd.SobolevModel(nif_amd.HessianLayer(model_p, [0], [cp_p["input_dim"]]))
    # neither a Jacobian nor a Hessian layer
    with pytest.raises(TypeError, match="JacobianLayer or a HessianLayer"):
        nif_amd.SobolevModel(model)
    # pruning and L-BFGS
    sm = nif_amd.SobolevModel(nif_amd.HessianLayer(model, [0], [cp["input_dim"]]))
    with pytest.raises(NotImplementedError, match="HessianLayer, three outputs"):
        nif_amd.sparsity.prune_low_magnitude(sm)
    x = np.zeros((4, cp["input_dim"] + cs["input_dim"]), np.float32)
    with pytest.raises(NotImplementedError, match="three-output"):
        nif_amd.optimizers.TFPLBFGS(sm, "mse", x, np.zeros((4, cs["output_dim"]), np.float32))
    with pytest.raises(NotImplementedError, match="three-output"):
        nif_amd.optimizers.LBFGSOptimizer(nif_amd.optimizers.MSEClosure(sm, x, np.zeros((4, cs["output_dim"]), np.float32)))


def test_evaluate_is_the_reference_loss_on_the_double():
    nif_amd, model, eng, kind, cs, cp = _double("ll")
    pi = cp["input_dim"]
    yi, xi = [0, 1], [pi + 1, pi]
    sm = nif_amd.SobolevModel(nif_amd.HessianLayer(model, yi, xi))
    sm.compile(nif_amd.Adam(1e-3), "huber", loss_weights=[1.5, 0.3, 0.2])
    _, _, _, o, ws, x, y, g, t, sw, _, _ = _problem("ll", B=7)
    f = lambda a: np.asarray(a, np.float32)
    x32, y32, g32, t32, sw32 = f(x), f(y), f(g), f(t), f(sw)
    eng.sobolev2_loss_and_grad = None      # (evaluate goes through the device entry of the double below)

    def s2(inputs, yv, gv, hv, x_index, w_jac, w_hess, sample_weight=None, want_grad=True, y_index=None):
        B = inputs.shape[0]
        so, nx = cs["output_dim"], len(x_index)
        arr = lambda a: (np.ascontiguousarray(a, np.float32).ravel(), 0)
        eng.sobolev2_loss_grad_dev(arr(inputs), arr(yv), arr(gv), arr(hv), None if sample_weight is None else arr(sample_weight),
                                   B, B, x_index, w_jac, w_hess, y_index)
        return float(eng.grad_buf[-1]), None
    eng.sobolev2_loss_and_grad = s2
    ev = sm.evaluate(x32, [y32, g32, t32], sample_weight=sw32)
    ref = hess_ref.sobolev2_loss_and_grad(kind, cs, cp, ws, x32.astype(np.float64), y32, g32, t32, yi, xi, (1.5, 0.3, 0.2),
                                         sw32, "huber", want_grad=False)[0]
    assert ev == pytest.approx(ref, rel=1e-6)
