"""CPU tests of the gradient transform: the restatement of tests/gradtf_ref.py against torch's clipping utilities, the host logic of
the optimizers / Model.fit (the marker of centralized_gradients_for_optimizer, Adam's clip keywords, push and pop on the engine double)
and what nif_set_grad_transform refuses (the struct is judged before the context, so no device is needed)."""
import ctypes as C
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import gradtf_ref as G
from tests.cfgs import ALL_SMALL

f32 = np.float32


def _layout(name):
    kind, cs, cp = ALL_SMALL[name]
    out, off = [], 0
    for nm, sh in O.Spec(kind, cs, cp).param_shapes():
        sh = tuple(int(v) for v in sh)
        out.append((nm, off, sh[0], sh[1] if len(sh) == 2 else 0))
        off += int(np.prod(sh))
    return out, off


def _tensors(g, layout):
    import torch
    return [torch.tensor(G._tensor(g, d).copy()) for d in layout]


def _flat(ts):
    return np.concatenate([t.numpy().ravel() for t in ts])


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# ---- the float64 restatement against torch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_SMALL))
def test_restatement_agrees_with_torch(name):
    """both sides fp64; torch's clip_grad_norm_ multiplies by min(c / (n + 1e-6), 1): compared where the norm is at least 10x away
    from the threshold, with the 1e-6 put back explicitly"""
    import torch
    layout, P = _layout(name)
    rng = np.random.default_rng(len(name))
    g = rng.standard_normal(P) * 10.0 ** rng.uniform(-3, 1, P)
    assert any(d[3] > 0 and d[2] > 1 for d in layout) and any(d[3] == 0 for d in layout)
    # centralise: mean over dim 0 of every matrix
    got, _, _ = G.transform64(g, layout, {"centralize": True})
    want = _flat([t - t.mean(dim=0, keepdim=True) if t.dim() == 2 else t for t in _tensors(g, layout)])
    assert _rel(got, want) <= 1e-12
    for d in layout:
        if d[3] > 0:
            assert np.abs(G._tensor(got, d).sum(axis=0)).max() <= 1e-12 * np.abs(G._tensor(g, d)).sum(axis=0).max() + 1e-300
    # clip by value
    got, _, _ = G.transform64(g, layout, {"clipvalue": 0.05})
    ts = [torch.nn.Parameter(torch.zeros_like(t)) for t in _tensors(g, layout)]
    for p, t in zip(ts, _tensors(g, layout)):
        p.grad = t.clone()
    torch.nn.utils.clip_grad_value_(ts, 0.05)
    assert np.array_equal(got, _flat([p.grad for p in ts]))
    assert np.abs(got).max() == 0.05
    # global norm: clipping (c = n / 10) and idle (c = 10 n)
    n = float(np.sqrt(np.sum(g * g)))
    for c, active in ((n / 10, True), (10 * n, False)):
        for spec in ({"global_clipnorm": c}, {"gtcf": True, "clipnorm": c}):
            got, per, glob = G.transform64(g, layout, spec)
            assert abs(glob - n) <= 1e-12 * n
            for p, t in zip(ts, _tensors(g, layout)):
                p.grad = t.clone()
            total = float(torch.nn.utils.clip_grad_norm_(ts, c))
            assert abs(total - n) <= 1e-12 * n
            want = _flat([p.grad for p in ts])
            if active:
                want = want * ((n + 1e-6) / n)           # torch divides by n + 1e-6
            assert _rel(got, want) <= 1e-12, (spec, active)
            assert (abs(np.sqrt(np.sum(got * got)) - c) <= 1e-12 * c) if active else _rel(got, g) <= 1e-15
    # per-tensor norm: one threshold 10x below the smallest tensor norm, one 10x above the largest
    norms = np.array([np.sqrt(np.sum(G._tensor(g, d) ** 2)) for d in layout])
    for c, active in ((norms.min() / 10, True), (norms.max() * 10, False)):
        got, per, _ = G.transform64(g, layout, {"clipnorm": c})
        assert _rel(per, norms) <= 1e-12
        want = []
        for t, nt in zip(_tensors(g, layout), norms):
            p = torch.nn.Parameter(torch.zeros_like(t)); p.grad = t.clone()
            torch.nn.utils.clip_grad_norm_([p], c)
            want.append(p.grad.numpy().ravel() * ((nt + 1e-6) / nt if active else 1.0))
        assert _rel(got, np.concatenate(want)) <= 1e-12, active


def test_restatement_order_and_corner_cases():
    layout, P = _layout("ms_plain_r3_si2")
    rng = np.random.default_rng(3)
    g = rng.standard_normal(P)
    # gtcf: the norm is the centralised gradient's, the clamp comes behind the scaling
    cen, _, _ = G.transform64(g, layout, {"centralize": True})
    n = np.sqrt(np.sum(cen * cen))
    got, _, glob = G.transform64(g, layout, {"centralize": True, "gtcf": True, "clipnorm": n / 4, "clipvalue": 0.01})
    assert abs(glob - n) <= 1e-12 * n
    assert np.allclose(got, np.clip(cen * (n / 4) / n, -0.01, 0.01), rtol=1e-12, atol=0)
    # a matrix with one row is centralised to exactly zero; vectors are left alone
    one_row = [d for d in _layout("ms_plain")[0] if d[3] > 0 and d[2] == 1]
    assert one_row
    lay1, P1 = _layout("ms_plain")
    g1 = rng.standard_normal(P1)
    for fn, dt in ((G.transform64, np.float64), (G.transform32, f32)):
        out = fn(g1.astype(dt), lay1, {"centralize": True})[0]
        for d in lay1:
            if d[3] > 0 and d[2] == 1:
                assert np.all(G._tensor(out, d) == 0)
            if d[3] == 0:
                assert np.array_equal(G._tensor(out, d), G._tensor(g1.astype(dt), d))
    # a zero gradient stays zero under every norm stage; a non-finite global norm makes Keras' form NaN
    z = np.zeros(P)
    for spec in ({"clipnorm": 1.0}, {"global_clipnorm": 1.0}, {"gtcf": True, "clipnorm": 1.0}):
        for fn in (G.transform64, G.transform32):
            assert np.all(fn(z, layout, spec)[0] == 0), spec
    bad = g.copy(); bad[5] = np.inf
    assert np.all(np.isnan(G.transform64(bad, layout, {"global_clipnorm": 1.0})[0]))
    assert np.all(np.isnan(G.transform32(bad, layout, {"global_clipnorm": 1.0})[0]))
    with pytest.raises(AssertionError):
        G.plan({"clipnorm": 1.0, "clipvalue": 1.0})


@pytest.mark.parametrize("name", ["ms_plain_r3_si2", "ll_plain"])
def test_float32_sequence_is_close_to_the_meaning(name):
    """the bar of the GPU tests, derived there: a fixed-order fp32 sum of squares with chains of a few dozen additions"""
    layout, P = _layout(name)
    rng = np.random.default_rng(11)
    g = (rng.standard_normal(P) * 10.0 ** rng.uniform(-4, 1, P)).astype(f32)
    n = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    for spec in ({"global_clipnorm": n / 3}, {"clipnorm": n / 50}, {"centralize": True, "gtcf": True, "clipnorm": n / 3, "clipvalue": n / 30}):
        a, pa, ga = G.transform32(g, layout, spec)
        b, pb, gb = G.transform64(g, layout, spec)
        assert a.dtype == f32 and abs(float(ga) - gb) <= 1e-5 * gb
        if not spec.get("centralize"):
            assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)) <= 1e-5


# ---- host logic ----------------------------------------------------------------------------------------------------------------
def test_marker_is_recognised_on_all_three_optimizers():
    from nif_amd import optimizers as Opt
    for opt in (Opt.Adam(1e-3), Opt.Lion(), Opt.AdaBeliefOptimizer()):
        assert Opt.grad_transform_of(opt) is None
        opt.get_gradients = Opt.centralized_gradients_for_optimizer(opt)
        assert Opt.grad_transform_of(opt) == {"centralize": True, "gtcf": True, "clipnorm": 0.0, "clipvalue": 0.0}
        opt.clipnorm = 0
        assert Opt.grad_transform_of(opt)["clipnorm"] == 0.0          # 0 and a missing attribute both mean off
        opt.clipnorm, opt.clipvalue = 2.5, 0.5
        assert Opt.grad_transform_of(opt) == {"centralize": True, "gtcf": True, "clipnorm": 2.5, "clipvalue": 0.5}
        with pytest.raises(NotImplementedError, match="no symbolic loss"):
            opt.get_gradients(None, [])
    lion = Opt.Lion()
    lion.clipnorm = 1.0                     # attributes without the marker: nothing is transformed (Lion has no Keras route)
    assert Opt.grad_transform_of(lion) is None
    with pytest.raises(TypeError):
        Opt.centralized_gradients_for_optimizer("adam")
    assert Opt.Lion().get_config() == {"name": "lion", "learning_rate": 1e-4, "decay": 0.0, "beta_1": 0.9, "beta_2": 0.99, "wd": 0.0}


def test_adam_clip_keywords_follow_keras():
    import nif_amd
    from nif_amd import optimizers as Opt
    assert Opt.grad_transform_of(nif_amd.Adam(1e-3)) is None
    assert Opt.grad_transform_of(nif_amd.Adam(1e-3, clipnorm=1.0)) == {"clipnorm": 1.0, "clipvalue": 0.0, "global_clipnorm": 0.0}
    assert Opt.grad_transform_of(nif_amd.Adam(1e-3, global_clipnorm=2.0))["global_clipnorm"] == 2.0
    assert Opt.grad_transform_of(nif_amd.Adam(1e-3, clipvalue=0.5))["clipvalue"] == 0.5
    for kw in ({"clipnorm": 1.0, "clipvalue": 1.0}, {"clipnorm": 1.0, "global_clipnorm": 1.0}, {"clipvalue": 1.0, "global_clipnorm": 1.0}):
        with pytest.raises(ValueError, match="At most one"):
            nif_amd.Adam(1e-3, **kw)
    with pytest.raises(ValueError):
        nif_amd.Adam(1e-3, clipnorm=-1.0)
    a = nif_amd.Adam(1e-3, clipnorm=1.0)
    a.clipvalue = 1.0                         # two set after construction: refused when the transform is read
    with pytest.raises(ValueError):
        Opt.grad_transform_of(a)
    nif_amd.Adam(1e-3, amsgrad=False)         # any other unknown keyword keeps its behaviour (ignored)
    for cls in (Opt.Lion, Opt.AdaBeliefOptimizer):
        for key in ("clipnorm", "clipvalue", "global_clipnorm"):
            with pytest.raises(NotImplementedError, match="centralized_gradients_for_optimizer"):
                cls(**{key: 1.0})


def _double_model():
    import nif_amd
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    from tests.doubles import OracleEngine

    class Eng(OracleEngine):
        """the engine double + a record of set_grad_transform and of the transform in force at every update"""

        def __init__(self, *a):
            OracleEngine.__init__(self, *a)
            self.tf_now, self.tf_calls, self.tf_at_step = None, [], []

        def set_grad_transform(self, spec=None, **kw):
            self.tf_now = dict(spec or {}, **kw) or None
            self.tf_calls.append(self.tf_now)

        def adam_step_dev(self, adam):
            self.tf_at_step.append(self.tf_now)
            OracleEngine.adam_step_dev(self, adam)

    kind, cs, cp = ALL_SMALL["ms_plain"]
    o = O.Spec(kind, cs, cp)
    eng = Eng(o, O.init_weights(o, np.random.default_rng(0)))
    model = Model(types.SimpleNamespace(_spec=Spec(kind, cs, cp), _engine=eng), "full")
    rng = np.random.default_rng(1)
    return nif_amd, model, eng, rng.uniform(-1, 1, (40, 2)).astype(f32), rng.uniform(-1, 1, (40, 1)).astype(f32)


def test_fit_pushes_and_pops_the_transform():
    nif_amd, model, eng, x, y = _double_model()
    model.compile(nif_amd.Adam(1e-2, global_clipnorm=0.5), "mse")
    model.fit(x, y, epochs=2, batch_size=20, shuffle=False, verbose=0)
    want = {"clipnorm": 0.0, "clipvalue": 0.0, "global_clipnorm": 0.5}
    assert eng.tf_calls == [want, None] and eng.tf_at_step == [want] * 4 and eng.tf_now is None
    # the gtcf route; attributes are read at the start of every fit
    opt = nif_amd.Adam(1e-2)
    opt.get_gradients = nif_amd.optimizers.centralized_gradients_for_optimizer(opt)
    model.compile(opt, "mse")
    model.fit(x, y, epochs=1, batch_size=40, shuffle=False, verbose=0)
    opt.clipnorm = 3.0
    model.fit(x, y, epochs=1, batch_size=40, shuffle=False, verbose=0)
    assert eng.tf_calls[2:] == [{"centralize": True, "gtcf": True, "clipnorm": 0.0, "clipvalue": 0.0}, None,
                                {"centralize": True, "gtcf": True, "clipnorm": 3.0, "clipvalue": 0.0}, None]
    # an error inside fit still clears it; an optimizer without a transform never touches the engine's
    with pytest.raises(NotImplementedError):
        model.fit(x, y, epochs=1, batch_size=40, verbose=0, steps_per_epoch=0.5, class_weight={0: 1})
    with pytest.raises(ValueError):
        model.fit(x, y, epochs=1, batch_size=40, verbose=0, steps_per_epoch=0)
    assert eng.tf_now is None and eng.tf_calls[-1] is None
    n = len(eng.tf_calls)
    model.compile(nif_amd.Adam(1e-2), "mse")
    model.fit(x, y, epochs=1, batch_size=40, shuffle=False, verbose=0)
    assert len(eng.tf_calls) == n
    two = nif_amd.Adam(1e-2, clipnorm=1.0); two.clipvalue = 1.0
    with pytest.raises(ValueError):
        model.compile(two, "mse")


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_set_grad_transform_refuses_bad_structs():
    from nif_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.nif_grad_transform) == 32

    def rc_msg(**kw):
        t = _lib.nif_grad_transform()
        for k, v in kw.items():
            if k == "reserved":
                t.reserved[v] = 1
            else:
                setattr(t, k, v)
        rc = lib.nif_set_grad_transform(None, C.byref(t))
        return rc, lib.nif_last_error().decode()

    assert rc_msg(flags=4) == (-1, "nif_grad_transform: unknown flag bits")
    assert rc_msg(flags=-1)[1].endswith("unknown flag bits")
    for i in range(4):
        assert rc_msg(reserved=i) == (-1, "nif_grad_transform: reserved fields must be zero")
    for key in ("clipnorm", "clipvalue", "global_clipnorm"):
        rc, msg = rc_msg(**{key: -1.0})
        assert rc == -1 and "must be >= 0" in msg
        assert "must be >= 0" in rc_msg(**{key: float("nan")})[1]
    for a, b in (("clipnorm", "clipvalue"), ("clipnorm", "global_clipnorm"), ("clipvalue", "global_clipnorm")):
        rc, msg = rc_msg(**{a: 1.0, b: 1.0})
        assert rc == -1 and "only one of" in msg
    assert "NIF_GT_GTCF has no global_clipnorm" in rc_msg(flags=_lib.GT_GTCF, global_clipnorm=1.0)[1]
    # valid structs pass the check and stop at the missing context
    for kw in ({}, {"flags": 3, "clipnorm": 1.0, "clipvalue": 2.0}, {"flags": 1}, {"global_clipnorm": 1.0}):
        assert rc_msg(**kw) == (-1, "nif_set_grad_transform: null context")
    assert lib.nif_set_grad_transform(None, None) == -1
    assert lib.nif_grad_transform_dev(None) == -1 and lib.nif_grad_norms(None, None, 0, None) == -1
