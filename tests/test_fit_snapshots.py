"""Model.fit_snapshots without a GPU: the factored formulas of the snapshot-wise step (tests/snapfit_ref.py) equal the oracle on the
expanded table, the extension header include/nif_hip_snapfit.h, its ctypes table and struct mirror and the library's exports are
equal, both entries pass the door of the C-ABI, and the step plan, the calls, History and the refusals of Model.fit_snapshots are what
they say on an engine double whose step is the reference.  The device path is tests/test_gpu_fit_snapshots.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import snapfit_ref as R
from tests.cfgs import ALL_SMALL, cfg_ll, cfg_ms
from tests.doubles import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nif_hip_snapfit.h")
ENTRIES = ["nif_snapshot_loss_grad", "nif_snapshot_loss_grad_dev"]


# ---- the algebra -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("r,so", [(1, 1), (3, 1), (10, 1), (1, 3), (3, 3), (10, 3)])
def test_factored_step_equals_the_oracle_on_the_expanded_table(r, so, weighted, loss):
    kind, cs, cp = cfg_ll(r=r, so=so, si=2, pi=2)
    spec = O.Spec(kind, cs, cp)
    ws = O.init_weights(spec, np.random.default_rng(7))
    names = [nm for nm, _ in spec.param_shapes()]
    ws[names.index("pnet_last_w")] = ws[names.index("pnet_last_w")] * 30.0      # (weight_init_factor makes the r x r map ~0)
    T, M = 5, 7
    p, x, y, sw = [a.astype(np.float64) for a in R.problem(spec, T, M)]
    s = sw if weighted else None
    assert not weighted or (sw == 0).any()
    for bg in (None, 3 * T * M):
        l, g = R.loss_and_grad(spec, ws, p, x, y, s, batch_global=bg, loss=loss)
        lr_, gr = O.loss_and_grad(spec, ws, R.expanded_table(p, x), y.reshape(T * M, so), None if s is None else s.reshape(-1),
                                  batch_global=bg, loss=loss)
        assert abs(l - lr_) <= 1e-12 * abs(lr_)
        gf, grf = O.flatten(g), O.flatten(gr)
        assert gf.shape == grf.shape
        assert np.linalg.norm(gf - grf) <= 1e-12 * np.linalg.norm(grf)


def test_expanded_table_is_snapshot_major():
    p, x = np.array([[1.0], [2.0]]), np.array([[10.0, 11.0], [20.0, 21.0], [30.0, 31.0]])
    t = R.expanded_table(p, x)
    assert t.shape == (6, 3)
    assert t[:, 0].tolist() == [1, 1, 1, 2, 2, 2] and t[:, 1].tolist() == [10, 20, 30, 10, 20, 30]


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_snapfit_header_exports_and_ctypes_table_are_equal():
    from nif_amd import _lib
    names = sorted(set(re.findall(r"\b(nif_[a-z0-9_]+)\s*\(", _header())))
    assert names == ENTRIES == sorted(_lib.SNAPFIT_SIGNATURES)
    others = [_lib.SIGNATURES, _lib.SNAPSHOT_SIGNATURES, _lib.ENCODE_SIGNATURES, _lib.SNAPDERIV_SIGNATURES, _lib.SNAPPARAM_SIGNATURES,
              _lib.SNAPPARAM2_SIGNATURES]
    assert not any(set(names) & set(t) for t in others)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert hasattr(lib, nm), "the header declares %s but the library does not export it" % nm
    bound = _lib.load()
    for nm in names:
        assert getattr(bound, nm).argtypes == _lib.SNAPFIT_SIGNATURES[nm][1] == [ctypes.POINTER(_lib.nif_snapfit_args)]
        assert getattr(bound, nm).restype is ctypes.c_int


def test_struct_mirror_has_the_headers_fields_size_and_offsets():
    """the header's struct laid out by the x86-64 / LP64 rules (natural alignment: int32 4, int64 and pointers 8) against ctypes'"""
    from nif_amd import _lib
    txt = _header()
    body = re.search(r"typedef\s+struct\s+nif_snapfit_args\s*\{(.*?)\}\s*nif_snapfit_args\s*;", txt, flags=re.S).group(1)
    fields, off = [], 0
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        m = re.match(r"^(.*?)(\w+)\s*(?:\[(\d+)\])?$", decl)
        ctype, name, count = m.group(1).strip(), m.group(2), int(m.group(3) or 1)
        size = 8 if ctype.endswith("*") else {"int32_t": 4, "int64_t": 8}[ctype]
        off = (off + size - 1) // size * size
        fields.append((name, off, size * count))
        off += size * count
    total = (off + 7) // 8 * 8
    mirror = _lib.nif_snapfit_args
    assert [f[0] for f in mirror._fields_] == [f[0] for f in fields]
    for name, o, sz in fields:
        assert (getattr(mirror, name).offset, getattr(mirror, name).size) == (o, sz), name
    assert ctypes.sizeof(mirror) == total
    assert int(re.search(r"#define\s+NIF_SNAPFIT_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.NIF_SNAPFIT_ABI_VERSION
    assert [f[0] for f in fields][:3] == ["abi_version", "reserved0", "ctx"] and fields[-1][0] == "reserved"


def test_both_entries_pass_the_guard_in_their_own_body():
    """tests/test_entry_guard.py's rule for the entries whose context travels inside the struct: NIF_ENTER(<args>->ctx, NIF_FLUSH_TAIL)"""
    from tests.test_entry_guard import _exports
    exports = _exports()
    for nm in ENTRIES:
        assert nm in exports, "%s is no extern \"C\" definition" % nm
        first, body = exports[nm]
        assert re.match(r"^const nif_snapfit_args\s*\*\s*(\w+)$", first), first
        arg = first.split("*")[-1].strip()
        assert re.search(r"\bNIF_ENTER\s*\(\s*%s\s*->\s*ctx\s*,\s*NIF_FLUSH_TAIL\s*\)" % arg, body), nm


def test_the_kernel_file_is_built_and_uses_no_atomics():
    import __graft_entry__ as G
    assert "k_snapfit.hip" in G.SOURCES
    src = open(os.path.join(G.CSRC, "k_snapfit.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\batomic\w*\s*\(", code)


# ---- Model.fit_snapshots on an engine double ---------------------------------------------------------------------------------------
class SnapEngine(OracleEngine):
    """tests/doubles.py::OracleEngine with the snapshot-wise step: the reference's factored formulas on what the device pointers hold"""

    def __init__(self, *a, **k):
        OracleEngine.__init__(self, *a, **k)
        self.loss_name = "mse"
        self.seen = []          # per snapshot step: (p [T, pi], sw [T, M] or None) as the call saw them

    def set_loss(self, name):
        self.loss_name = name

    def snapshot_loss_grad_dev(self, d_p, t, d_x, m, d_y, d_sw, batch_global=0):
        o = self.o
        take = lambda d, n, shape: d[0][d[1]:d[1] + n].reshape(shape).astype(np.float64)
        p, x = take(d_p, t * o.pi, (t, o.pi)), take(d_x, m * o.si, (m, o.si))
        y = take(d_y, t * m * o.so, (t, m, o.so))
        sw = None if d_sw is None else take(d_sw, t * m, (t, m))
        loss, grads = R.loss_and_grad(o, O.unflatten(o, self.theta), p, x, y, sw, batch_global=batch_global or t * m, loss=self.loss_name)
        self.grad_buf[:-1] = O.flatten(grads); self.grad_buf[-1] = loss
        self.reg_applied = False
        self.calls.append(("snapshot_loss_grad", int(t), int(m), int(batch_global)))
        self.seen.append((p.copy(), None if sw is None else sw.copy()))


def _double(cfg=None, T=10, M=6, seed=1):
    import nif_amd
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    kind, cs, cp = cfg or ALL_SMALL["ll_plain"]
    o = O.Spec(kind, cs, cp)
    eng = SnapEngine(o, O.init_weights(o, np.random.default_rng(0)))
    model = Model(types.SimpleNamespace(_spec=Spec(kind, cs, cp), _engine=eng), "full")
    p, x, u, sw = R.problem(o, T, M, seed=seed)
    return nif_amd, model, eng, o, p, x, u, sw


def _steps(eng):
    return [c for c in eng.calls if c[0] == "snapshot_loss_grad"]


def test_step_plan_shapes_and_batch_global_without_shuffle():
    nif_amd, model, eng, o, p, x, u, sw = _double()
    model.compile(nif_amd.Adam(1e-3), "mse")
    h = model.fit_snapshots(x, u, p, epochs=2, snapshots_per_step=4, shuffle=False)
    assert _steps(eng) == [("snapshot_loss_grad", t, 6, t * 6) for t in (4, 4, 2)] * 2
    assert not [c for c in eng.calls if c[0] in ("gather", "loss_grad", "reserve")]
    assert eng.t == 6 and h.epoch == [0, 1] and len(h.history["loss"]) == 2 and list(h.history) == ["loss"]
    # the steps are in order, and each saw its own snapshots' rows of p
    assert np.array_equal(np.vstack([s[0] for s in eng.seen[:3]]), p.astype(np.float64))
    assert all(s[1] is None for s in eng.seen)
    assert model.history is h


def test_history_is_the_weighted_mean_of_the_step_losses_of_the_reference():
    nif_amd, model, eng, o, p, x, u, sw = _double()
    model.compile(nif_amd.Adam(1e-3), "mse")
    th = eng.theta.copy()
    h = model.fit_snapshots(x, u, p, sample_weight=sw, epochs=1, snapshots_per_step=4, shuffle=False)
    ref = SnapEngine(o, O.unflatten(o, th))
    tot = 0.0
    adam = model.optimizer.as_struct()
    for t0, ts in ((0, 4), (4, 4), (8, 2)):
        l, g = R.loss_and_grad(o, O.unflatten(o, ref.theta), p[t0:t0 + ts], x, u[t0:t0 + ts], sw[t0:t0 + ts])
        ref.grad_buf[:-1] = O.flatten(g); ref.grad_buf[-1] = l
        ref.adam_step_dev(adam)
        tot += ts * 6 * l
    assert abs(h.history["loss"][0] - tot / 60.0) <= 1e-12 * abs(tot / 60.0)
    assert np.array_equal(eng.theta, ref.theta)


def test_a_shuffled_epoch_is_one_permutation_of_the_snapshots_gathered_on_the_device():
    nif_amd, model, eng, o, p, x, u, sw = _double()
    model.compile(nif_amd.Adam(1e-3), "mse")
    model._shuffle_seed = 3
    model.fit_snapshots(x, u, p, sample_weight=sw, epochs=2, snapshots_per_step=4, shuffle=True)
    gathers = [c for c in eng.calls if c[0] == "gather"]
    assert gathers == [("gather", 10, o.pi), ("gather", 10, 6 * o.so), ("gather", 10, 6)] * 2      # p, u as [T][M so], sw as [T][M]
    assert [c[1] for c in _steps(eng)] == [4, 4, 2, 4, 4, 2]
    rng = np.random.default_rng(3)
    for ep in range(2):
        perm = rng.permutation(10)
        seen_p = np.vstack([s[0] for s in eng.seen[3 * ep:3 * ep + 3]])
        seen_w = np.vstack([s[1] for s in eng.seen[3 * ep:3 * ep + 3]])
        assert np.array_equal(seen_p, p[perm].astype(np.float64)) and np.array_equal(seen_w, sw[perm].astype(np.float64))


@pytest.mark.parametrize("form", ["TM", "M", "T"])
def test_the_three_sample_weight_forms_broadcast_to_T_by_M(form):
    nif_amd, model, eng, o, p, x, u, sw = _double()
    model.compile(nif_amd.Adam(1e-3), "mse")
    rng = np.random.default_rng(5)
    w = {"TM": sw, "M": rng.uniform(0.5, 1.5, size=6).astype(np.float32), "T": rng.uniform(0.5, 1.5, size=10).astype(np.float32)}[form]
    full = {"TM": sw, "M": np.tile(w[None, :], (10, 1)) if form == "M" else None, "T": np.tile(w[:, None], (1, 6)) if form == "T" else None}[form]
    model.fit_snapshots(x, u, p, sample_weight=w, epochs=1, shuffle=False)
    assert _steps(eng) == [("snapshot_loss_grad", 10, 6, 60)]      # snapshots_per_step=None: all T
    assert np.array_equal(eng.seen[0][1], full.astype(np.float64))


def test_the_losses_of_compile_reach_the_step():
    for loss in R.LOSSES:
        nif_amd, model, eng, o, p, x, u, sw = _double()
        model.compile(nif_amd.Adam(1e-3), loss)
        th = O.unflatten(o, eng.theta.copy())
        h = model.fit_snapshots(x, u, p, epochs=1, shuffle=False)
        l, _ = R.loss_and_grad(o, th, p, x, u, loss=loss)
        assert abs(h.history["loss"][0] - l) <= 1e-12 * abs(l)
        assert eng.loss_name == "mse"       # (popped behind the call: the engine is shared)


def test_callbacks_initial_epoch_and_stop_training():
    nif_amd, model, eng, o, p, x, u, sw = _double()
    model.compile(nif_amd.Adam(1e-2), "mse")
    log = []

    class CB(object):
        def set_model(self, m): log.append("set_model")
        def on_train_begin(self, logs): log.append("begin")
        def on_epoch_begin(self, ep, logs): log.append(("eb", ep))
        def on_epoch_end(self, ep, logs):
            log.append(("ee", ep, sorted(logs)))
            logs["extra"] = 1.0
            if ep == 2:
                model.stop_training = True
        def on_train_end(self, logs): log.append("end")
    h = model.fit_snapshots(x, u, p, epochs=5, initial_epoch=1, shuffle=False, callbacks=[CB()])
    assert log == ["set_model", "begin", ("eb", 1), ("ee", 1, ["loss"]), ("eb", 2), ("ee", 2, ["loss"]), "end"]
    assert h.epoch == [1, 2] and h.history["extra"] == [1.0, 1.0]
    assert eng.t == 2


def test_empty_inputs_run_no_step():
    nif_amd, model, eng, o, p, x, u, sw = _double()
    model.compile(nif_amd.Adam(1e-3), "mse")
    h = model.fit_snapshots(x, u[:0], p[:0], epochs=1)
    assert _steps(eng) == [] and h.history["loss"] == [0.0]
    h = model.fit_snapshots(x[:0], u[:, :0], p, epochs=1)
    assert _steps(eng) == [] and h.history["loss"] == [0.0]


def test_refusals_and_their_messages():
    nif_amd, model, eng, o, p, x, u, sw = _double()
    with pytest.raises(RuntimeError, match="compile"):
        model.fit_snapshots(x, u, p)
    model.compile(nif_amd.Adam(1e-3), "mse")
    with pytest.raises(ValueError, match=r"u must have shape \(T=10, M=6, so_dim=2\)"):
        model.fit_snapshots(x, u[:, :5], p)
    with pytest.raises(ValueError, match=r"x must have shape \(M, si_dim=2\)"):
        model.fit_snapshots(x[:, :1], u, p)
    with pytest.raises(ValueError, match=r"p must have shape \(T, pi_dim=1\)"):
        model.fit_snapshots(x, u, np.zeros((10, 3), dtype=np.float32))
    with pytest.raises(ValueError, match=r"sample_weight must have shape \(T, M\), \(M,\) or \(T,\)"):
        model.fit_snapshots(x, u, p, sample_weight=np.ones(7))
    with pytest.raises(ValueError, match="snapshots_per_step"):
        model.fit_snapshots(x, u, p, snapshots_per_step=0)
    model.compile(nif_amd.Adam(1e-3), "mse", metrics=["mse"])
    with pytest.raises(NotImplementedError, match=r"metrics"):
        model.fit_snapshots(x, u, p)
    model.compile(nif_amd.Adam(1e-3), "mse")
    model._jac_reg = 0.1
    with pytest.raises(NotImplementedError, match="activity or latent-Jacobian regulariser"):
        model.fit_snapshots(x, u, p)
    model._jac_reg = 0.0
    assert eng.calls == []
    # the hypernetwork classes stay refused
    nif_amd, hyper, heng, ho, hp, hx, hu, _ = _double2(cfg_ms(r=3, si=2, pi=1, so=2))
    hyper.compile(nif_amd.Adam(1e-3), "mse")
    with pytest.raises(NotImplementedError, match="NIFMultiScaleLastLayerParameterized.*per-snapshot weight-gradient kernel"):
        hyper.fit_snapshots(hx, hu, hp)
    assert heng.calls == []


def _double2(cfg):
    """a double of another class (the step is never reached)"""
    import nif_amd
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    kind, cs, cp = cfg
    o = O.Spec(kind, cs, cp)
    eng = SnapEngine(o, O.init_weights(o, np.random.default_rng(0)))
    model = Model(types.SimpleNamespace(_spec=Spec(kind, cs, cp), _engine=eng), "full")
    rng = np.random.default_rng(2)
    return (nif_amd, model, eng, o, rng.uniform(-1, 1, size=(4, o.pi)).astype(np.float32), rng.uniform(-1, 1, size=(5, o.si)).astype(np.float32),
            rng.uniform(-1, 1, size=(4, 5, o.so)).astype(np.float32), None)


def test_more_than_one_rank_is_refused(monkeypatch):
    from nif_amd import distributed as dist
    nif_amd, model, eng, o, p, x, u, sw = _double()
    model.compile(nif_amd.Adam(1e-3), "mse")
    monkeypatch.setattr(dist, "get", lambda: types.SimpleNamespace(world=2))
    with pytest.raises(NotImplementedError, match=r"one GPU \(world = 2\)"):
        model.fit_snapshots(x, u, p)
    assert eng.calls == []


def test_a_mixed_policy_is_refused():
    import nif_amd
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    kind, cs, cp = ALL_SMALL["ll_plain"]
    o = O.Spec(kind, cs, cp)
    eng = SnapEngine(o, O.init_weights(o, np.random.default_rng(0)))
    model = Model(types.SimpleNamespace(_spec=Spec(kind, cs, cp, "mixed_bfloat16"), _engine=eng), "full")
    model.compile(nif_amd.Adam(1e-3), "mse")
    p, x, u, _ = R.problem(o, 3, 4)
    with pytest.raises(NotImplementedError, match="mixed_bfloat16 policy"):
        model.fit_snapshots(x, u, p)


def test_the_sobolev_model_refuses_the_call():
    from nif_amd.model import Model, SobolevModel
    assert SobolevModel.fit_snapshots is not Model.fit_snapshots
    sm = SobolevModel.__new__(SobolevModel)
    with pytest.raises(NotImplementedError, match="SobolevModel.fit_snapshots"):
        sm.fit_snapshots(None, None, None)


def test_fit_records_the_same_calls_as_before():
    """fit() on the expanded table: the calls it made before the step tail was shared, and the update fit_snapshots makes"""
    nif_amd, model, eng, o, p, x, u, sw = _double()
    model.compile(nif_amd.Adam(1e-3), "mse")
    table, y = R.expanded_table(p, x).astype(np.float32), u.reshape(60, o.so)
    th = eng.theta.copy()
    h = model.fit(table, y, epochs=2, batch_size=24, shuffle=False, verbose=0)
    assert eng.calls == [("reserve", 24)] + [("loss_grad", 24, 24), ("loss_grad", 24, 24), ("loss_grad", 12, 12)] * 2
    eng.calls = []
    h2 = model.fit(table, y, epochs=1, batch_size=24, shuffle=True, verbose=0)
    assert eng.calls == [("reserve", 24), ("gather", 60, 3), ("gather", 60, 2), ("loss_grad", 24, 24), ("loss_grad", 24, 24),
                         ("loss_grad", 12, 12)]
    assert eng.t == 9 and len(h.history["loss"]) == 2 and len(h2.history["loss"]) == 1
    # the same snapshots per batch: the two calls walk the same trajectory
    nif_amd, m2, eng2, o, p, x, u, sw = _double()
    assert np.array_equal(eng2.theta, th)
    m2.compile(nif_amd.Adam(1e-3), "mse")
    hs = m2.fit_snapshots(x, u, p, epochs=2, snapshots_per_step=4, shuffle=False)
    assert np.allclose(hs.history["loss"], h.history["loss"], rtol=1e-9, atol=0)
