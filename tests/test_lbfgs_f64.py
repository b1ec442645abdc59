"""Host logic of the L-BFGS fine-tuner's dtype keyword (TFPLBFGS / MSEClosure / LBFGSOptimizer) on an engine double whose f64_*
methods call the fp64 oracle: the default takes the old path unchanged; dtype="float64" sends every trial point and the data up
unrounded, keeps a float64 master vector between rounds and minimize() calls, and leaves the model its rounding."""
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests.cfgs import ALL_SMALL
from tests.doubles import OracleEngine


class _HostArray64(object):
    def __init__(self, n):
        self.buf = np.zeros((int(n),), dtype=np.float64)

    def at(self, off):
        return (self.buf, int(off))

    def upload(self, host, double_offset=0):
        h = np.asarray(host)
        assert h.dtype == np.float64, "the float64 closure uploads float64 arrays"
        self.buf[double_offset:double_offset + h.size] = h.ravel()

    def free(self):
        pass


class _F64Engine(OracleEngine):
    """OracleEngine plus what TFPLBFGS drives: the float32 parameter surface (set_flat rounds, like nif_set_params' float buffer)
    and the f64_* surface with a master vector of its own"""

    def __init__(self, name="ms_plain", mixed_policy="float32"):
        from nif_amd.spec import Spec
        kind, cs, cp = ALL_SMALL[name]
        o = O.Spec(kind, cs, cp)
        ws = [w.astype(np.float32) for w in O.init_weights(o, np.random.default_rng(0))]
        OracleEngine.__init__(self, o, ws)
        self.spec = Spec(kind, cs, cp, mixed_policy)
        self.master = None
        self.seen = []               # every vector f64_set_flat received
        self.loss_name = "mse"
        self.f64_buf = np.zeros((self.n_params + 1,))

    def _inputs(self, a):
        return np.ascontiguousarray(np.asarray(a, dtype=np.float32)[:, :self.o.pi + self.o.si])

    def _targets(self, y, n):
        return np.ascontiguousarray(y, dtype=np.float32).reshape(n, self.o.so)

    def _weights(self, sw, n):
        return None if sw is None else np.ascontiguousarray(sw, dtype=np.float32).reshape(n)

    def set_loss(self, name):
        self.loss_name = name

    def set_flat(self, th):
        assert np.asarray(th).dtype == np.float32
        self.theta = np.asarray(th, dtype=np.float32).astype(np.float64)

    def get_flat(self):
        return self.theta.astype(np.float32)

    def grad_read(self):
        loss, g = OracleEngine.grad_read(self)
        return float(np.float32(loss)), g.astype(np.float32)

    # ---- the double-precision surface
    def alloc_f64(self, n):
        return _HostArray64(n)

    def f64_set_flat(self, th):
        th = np.asarray(th)
        assert th.dtype == np.float64 and th.shape == (self.n_params,)
        self.master = th.copy()
        self.seen.append(th.copy())

    def f64_get_flat(self):
        return self.master.copy()

    def f64_loss_grad_dev(self, d_x, d_y, d_sw, b, bg):
        ncol = self.o.pi + self.o.si
        x = d_x[0][d_x[1]:d_x[1] + b * ncol].reshape(b, ncol)
        y = d_y[0][d_y[1]:d_y[1] + b * self.o.so].reshape(b, self.o.so)
        sw = None if d_sw is None else d_sw[0][d_sw[1]:d_sw[1] + b]
        assert x.dtype == np.float64 and y.dtype == np.float64
        loss, g = O.loss_and_grad(self.o, O.unflatten(self.o, self.master), x, y, sw, batch_global=bg, loss=self.loss_name)
        self.f64_buf[:-1] = O.flatten(g); self.f64_buf[-1] = loss

    def f64_grad_read(self):
        return float(self.f64_buf[-1]), self.f64_buf[:-1].copy()


def _model(eng, **attrs):
    from nif_amd.model import Model
    m = Model(types.SimpleNamespace(_spec=eng.spec, _engine=eng), "full")
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _data(n=40, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, size=(n, 2)), rng.uniform(-1, 1, size=(n, 1))      # float64, not representable in float32


def _sub_f32(a):
    return bool(np.any(a != a.astype(np.float32).astype(np.float64)))


def test_default_dtype_is_the_old_path():
    from nif_amd.optimizers import TFPLBFGS
    x, y = _data()
    hist = []
    for kw in ({}, {"dtype": "float32"}):
        eng = _F64Engine()
        t = TFPLBFGS(_model(eng), "mse", x, y, display_epoch=1 << 62, **kw)
        hist.append(t.minimize(rounds=2, max_iter=4))
        assert eng.seen == [] and eng.master is None          # nothing of the double surface is touched
        assert t.dtype == "float32"
    assert hist[0]["loss"] == hist[1]["loss"] and len(hist[0]["loss"]) > 2
    assert list(hist[0]["iteration"]) == list(hist[1]["iteration"])


def test_float64_points_data_and_master_vector():
    from nif_amd.optimizers import TFPLBFGS
    x, y = _data()
    sw = np.random.default_rng(2).uniform(0.5, 1.5, size=(40,))
    assert _sub_f32(x) and _sub_f32(y) and _sub_f32(sw)
    eng = _F64Engine()
    theta32 = eng.get_flat()
    t = TFPLBFGS(_model(eng), "mse", x, y, display_epoch=1 << 62, sample_weight=sw, dtype="float64")
    # float64 inputs, targets and weights are not rounded on their way to the engine
    assert np.array_equal(t._d_x.buf, x.ravel()) and np.array_equal(t._d_y.buf, y.ravel()) and np.array_equal(t._d_sw.buf, sw)
    # the master vector starts as the exact upcast of the float32 parameters
    assert t.position.dtype == np.float64 and np.array_equal(t.position, theta32.astype(np.float64))
    # a trial point with bits below float32 arrives intact, and loss / gradient come back as float64
    probe = t.position * (1.0 + 1e-10)
    assert _sub_f32(probe)
    loss, g = t._f(probe)
    assert np.array_equal(eng.seen[-1], probe) and g.dtype == np.float64
    l_ref, g_ref = O.loss_and_grad(eng.o, O.unflatten(eng.o, probe), x, y, sw)
    assert loss == l_ref and np.array_equal(g, O.flatten(g_ref))
    # rounds: the master vector survives between them -- round 2 starts at round 1's unrounded result
    eng.seen.clear()
    n0 = len(t.history["loss"])
    t.minimize(rounds=1, max_iter=3)
    p1 = t.position
    assert _sub_f32(p1) and np.array_equal(eng.master, p1)
    assert np.array_equal(eng.get_flat(), p1.astype(np.float32))          # the model holds the rounding
    k = len(eng.seen)
    t.minimize(rounds=1, max_iter=3)
    assert np.array_equal(eng.seen[k], p1), "round 2 must start from the float64 master vector, not from rounded parameters"
    p2 = t.position
    assert np.array_equal(eng.get_flat(), p2.astype(np.float32)) and t.history["loss"][-1] < t.history["loss"][n0]
    assert len(t.history["iteration"]) == len(t.history["loss"])


def test_display_epoch_prints_in_float64(capsys):
    from nif_amd.optimizers import TFPLBFGS
    x, y = _data()
    t = TFPLBFGS(_model(_F64Engine()), "mse", x, y, display_epoch=2, dtype="float64")
    t._f(t.position); t._f(t.position)
    assert "Epoch: 2 loss:" in capsys.readouterr().out


def test_lbfgs_optimizer_follows_its_closure():
    from nif_amd.optimizers import LBFGSOptimizer, MSEClosure
    x, y = _data()
    eng = _F64Engine()
    c = MSEClosure(_model(eng), x, y, dtype="float64")
    opt = LBFGSOptimizer(c, None, steps=2)
    l0 = c()
    opt.minimize()
    p1 = opt.position
    assert p1.dtype == np.float64 and _sub_f32(p1) and opt.epoch == 2 and opt.loss < l0
    assert np.array_equal(eng.master, p1) and np.array_equal(eng.get_flat(), p1.astype(np.float32))
    assert c() == opt.loss                                   # the closure evaluates at the master vector, not at its rounding
    opt.minimize()
    p2 = opt.position
    assert opt.epoch == 4 and opt.loss < l0 and not np.array_equal(p1, p2)
    assert np.array_equal(eng.get_flat(), p2.astype(np.float32))
    # one uninterrupted run of 4 iterations from the same start is the same run: the pairs and the point were carried in float64
    from nif_amd.optimizers import LBFGSMinimizer
    eng2 = _F64Engine()
    c2 = MSEClosure(_model(eng2), x, y, dtype="float64")
    xa, fa = LBFGSMinimizer(c2._t._f).run(c2._t.position, 4)
    assert np.array_equal(xa, p2) and fa == opt.loss


def test_refusals():
    from nif_amd.optimizers import MSEClosure, TFPLBFGS
    x, y = _data()
    with pytest.raises(ValueError, match="float16"):
        TFPLBFGS(_model(_F64Engine()), "mse", x, y, dtype="float16")
    with pytest.raises(ValueError, match="float16"):
        MSEClosure(_model(_F64Engine()), x, y, dtype="float16")
    ll = _F64Engine("ll_plain")
    with pytest.raises(NotImplementedError, match="NIFMultiScaleLastLayerParameterized is not built"):
        TFPLBFGS(_model(ll), "mse", np.zeros((4, 3)), np.zeros((4, 2)), dtype="float64")
    with pytest.raises(NotImplementedError, match="mixed_policy='mixed_bfloat16' is not built"):
        TFPLBFGS(_model(_F64Engine(mixed_policy="mixed_bfloat16")), "mse", x, y, dtype="float64")
    with pytest.raises(NotImplementedError, match="Sobolev model is not built"):
        TFPLBFGS(_model(_F64Engine(), _order=1), "mse", x, y, dtype="float64")
    # the existing refusals keep their place in front, and their texts
    with pytest.raises(NotImplementedError, match="pruned model"):
        TFPLBFGS(_model(_F64Engine(), _is_pruned=True), "mse", x, y, dtype="float64")
    with pytest.raises(NotImplementedError, match="three-output"):
        TFPLBFGS(_model(_F64Engine(), _order=2), "mse", x, y, dtype="float64")
    with pytest.raises(NotImplementedError, match="built losses"):
        TFPLBFGS(_model(_F64Engine()), "mape", x, y, dtype="float64")
