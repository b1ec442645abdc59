"""Model.predict_snapshot_parameter_derivatives without a GPU: the fifth extension header, its ctypes table and struct mirror and the
library's exports are equal, both entries pass the door of the C-ABI, and the host side (argument checks, result shapes, the chunk
plan) does what it says on an engine double.  The device path is tests/test_gpu_snapshot_param_derivatives.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests.cfgs import cfg_ll, cfg_ms, cfg_nif
from tests.doubles import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nif_hip_snapparam.h")
ENTRIES = ["nif_snapshot_param_derivatives", "nif_snapshot_param_derivatives_dev"]
FIELDS = ["abi_version", "rows_are_latent", "ctx", "rows", "drows", "nd", "np", "p_idx", "T", "x", "offsets_host", "M", "y_idx", "ny",
          "u", "dudp"]


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_exports_and_ctypes_table_are_equal():
    from nif_amd import _lib
    names = sorted(set(re.findall(r"\b(nif_[a-z0-9_]+)\s*\(", _header())))
    assert names == ENTRIES == sorted(_lib.SNAPPARAM_SIGNATURES)
    assert not set(names) & (set(_lib.SIGNATURES) | set(_lib.SNAPSHOT_SIGNATURES) | set(_lib.ENCODE_SIGNATURES) | set(_lib.SNAPDERIV_SIGNATURES))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert hasattr(lib, nm), "the header declares %s but the library does not export it" % nm
    bound = _lib.load()
    for nm in names:
        assert getattr(bound, nm).argtypes == _lib.SNAPPARAM_SIGNATURES[nm][1] == [ctypes.POINTER(_lib.nif_snapparam_args)]
        assert getattr(bound, nm).restype is ctypes.c_int


def test_struct_mirror_has_the_headers_fields_size_and_offsets():
    """the header's struct laid out by the x86-64 / LP64 rules (natural alignment: int32 4, int64 and pointers 8) against ctypes'"""
    from nif_amd import _lib
    txt = _header()
    body = re.search(r"typedef\s+struct\s+nif_snapparam_args\s*\{(.*?)\}\s*nif_snapparam_args\s*;", txt, flags=re.S).group(1)
    fields, off = [], 0
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        m = re.match(r"^(.*?)(\w+)\s*(?:\[(\d+)\])?$", decl)
        ctype, name, count = m.group(1).strip(), m.group(2), int(m.group(3) or 1)
        size = 8 if ctype.endswith("*") else {"int32_t": 4, "int64_t": 8}[ctype]
        assert off % size == 0, "%s would sit behind implicit padding: state it as a reserved field" % name
        fields.append((name, off, size * count))
        off += size * count
    assert off % 8 == 0
    mirror = _lib.nif_snapparam_args
    assert [f[0] for f in mirror._fields_] == [f[0] for f in fields]
    for name, o, sz in fields:
        assert (getattr(mirror, name).offset, getattr(mirror, name).size) == (o, sz), name
    assert ctypes.sizeof(mirror) == off
    assert int(re.search(r"#define\s+NIF_SNAPPARAM_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.NIF_SNAPPARAM_ABI_VERSION
    # the fields the interface names, in its order; everything else is reserved
    assert [f[0] for f in fields if not f[0].startswith("reserved")] == FIELDS
    assert fields[-1][0] == "reserved" and fields[-1][2] == 32


def test_both_entries_pass_the_guard_in_their_own_body():
    """tests/test_entry_guard.py's rule for the entries whose context travels inside the struct: NIF_ENTER(<args>->ctx, NIF_FLUSH_TAIL);
    the struct pointer is the FIRST (and only) parameter, so neither entry joins the context-first set of the older tables"""
    from tests.test_entry_guard import _exports
    exports = _exports()
    for nm in ENTRIES:
        assert nm in exports, "%s is no extern \"C\" definition" % nm
        first, body = exports[nm]
        assert re.match(r"^const nif_snapparam_args\s*\*\s*(\w+)$", first), first
        arg = first.split("*")[-1].strip()
        assert re.search(r"\bNIF_ENTER\s*\(\s*%s\s*->\s*ctx\s*,\s*NIF_FLUSH_TAIL\s*\)" % arg, body), nm


# ---- the host side on an engine double ---------------------------------------------------------------------------------------------
class SnapParamEngine(OracleEngine):
    """tests/doubles.py's engine with the three calls predict_snapshot_parameter_derivatives makes.  p rows: the fp64 oracle's
    derivative layer on the expanded table, parameter columns; latent rows: a stand-in that depends on the row, its directions and the
    points (the device path is tested on the GPU).  Every call is recorded with the points it was asked for."""

    def __init__(self, kind, cs, cp, seed=0):
        ospec = O.Spec(kind, cs, cp)
        OracleEngine.__init__(self, ospec, O.init_weights(ospec, np.random.default_rng(seed), dtype=np.float32))
        self.ws = O.unflatten(ospec, self.theta)
        self.freed = 0
        self.asked = []      # (snapshot's row [and directions] as bytes, point as bytes) of every point an engine call was asked for

    def snapshot_mesh(self, x):
        self.calls.append(("mesh", np.shape(x)))
        owner = self

        class Mesh(object):
            def __init__(self, a):
                self.x = np.array(a, dtype=np.float32)

            def free(self):
                owner.freed += 1

        return Mesh(x)

    def _one(self, row, drow, x, yi, pi_):
        s = self.o
        key = np.asarray(row, np.float32).tobytes() + (b"" if drow is None else np.asarray(drow, np.float32).tobytes())
        for pt in x:
            self.asked.append((key, np.asarray(pt, np.float32).tobytes()))
        if drow is not None:
            u = np.outer(np.sin(x.sum(axis=1)), np.ones(s.so)) * float(np.sum(row))
            d = u[:, :1, None] * np.sum(drow, axis=1)[None, None, :] + np.zeros((x.shape[0], len(yi), drow.shape[0]))
        else:
            tab = np.hstack([np.tile(row, (x.shape[0], 1)), x]).astype(np.float64)
            u, d, _ = O.hessian_analytic(s, self.ws, tab, yi, list(pi_))
        return np.asarray(u, dtype=np.float32), np.asarray(d, dtype=np.float32)

    def snapshot_param_derivatives(self, rows, drows, mesh, lo, hi, y_index, p_index):
        self.calls.append(("shared", np.shape(rows)[0], lo, hi, tuple(y_index), None if p_index is None else tuple(p_index),
                           None if drows is None else np.shape(drows)))
        parts = [self._one(r, None if drows is None else drows[t], mesh.x[lo:hi], y_index, p_index) for t, r in enumerate(rows)]
        return tuple(np.stack([p[i] for p in parts]) for i in range(2))

    def snapshot_param_derivatives_ragged(self, rows, drows, xs, y_index, p_index):
        assert len(xs) == np.shape(rows)[0] and (drows is None or np.shape(drows)[0] == len(xs))
        self.calls.append(("ragged", [a.shape[0] for a in xs], tuple(y_index), None if p_index is None else tuple(p_index),
                           None if drows is None else np.shape(drows)))
        parts = [self._one(r, None if drows is None else drows[t], a, y_index, p_index) for t, (r, a) in enumerate(zip(rows, xs))]
        return tuple(np.concatenate([p[i] for p in parts], axis=0) for i in range(2))


def _model(cfg, role="full"):
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    kind, cs, cp = cfg
    eng = SnapParamEngine(kind, cs, cp)
    owner = types.SimpleNamespace(_engine=eng, _spec=Spec(kind, cs, cp, "float32"))
    return Model(owner, role), eng, eng.o


CFGS = {"nif": cfg_nif(r=2, so=2, si=2, pi=2, act="tanh"), "ms": cfg_ms(r=3, si=2, pi=2), "ll": cfg_ll()}
RAGGED = [1, 7, 0, 40, 13]
ND = 4


def _inputs(spec, seed=1):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, size=(len(RAGGED), spec.pi)).astype(np.float32)
    lat = rng.uniform(-1, 1, size=(len(RAGGED), spec.r)).astype(np.float32)
    dl = rng.uniform(-1, 1, size=(len(RAGGED), ND, spec.r)).astype(np.float32)
    xs = [rng.uniform(-1, 1, size=(m, spec.si)).astype(np.float32) for m in RAGGED]
    return p, lat, dl, xs


def test_argument_checks():
    m, eng, spec = _model(CFGS["ms"])
    p, lat, dl, xs = _inputs(spec)
    T = len(RAGGED)
    f = m.predict_snapshot_parameter_derivatives
    bad = [
        dict(),                                              # neither p nor latent
        dict(p=p, latent=lat, dlatent=dl),                   # both
        dict(p=p, latent=lat),
        dict(latent=lat),                                    # latent without dlatent
        dict(dlatent=dl),                                    # dlatent without latent
        dict(p=p, dlatent=dl),
        dict(latent=lat, dlatent=dl, p_index=[0]),           # p_index with latent
        dict(p=lat),                                         # [T, r] where [T, pi] belongs
        dict(latent=p, dlatent=dl),
        dict(p=p[0]),
        dict(latent=lat, dlatent=dl[:, 0]),                  # wrong shapes of dlatent
        dict(latent=lat, dlatent=dl[:-1]),
        dict(latent=lat, dlatent=dl[:, :, :-1]),
        dict(latent=lat, dlatent=dl[:, :0]),                 # no direction
        dict(latent=lat, dlatent=np.zeros((T, 17, spec.r), np.float32)),      # more than 16 directions
        dict(p=p, p_index=[spec.pi]),                        # a parameter column out of range
        dict(p=p, p_index=[-1]),
        dict(p=p, p_index=[0, 0]),                           # repeated
        dict(p=p, p_index=[]),
        dict(p=p, y_index=[spec.so]),
        dict(p=p, y_index=[-1]),
        dict(p=p, y_index=[]),
        dict(p=p, y_index=[0] * 17),                         # more than 16 entries
        dict(latent=lat, dlatent=dl, y_index=[0] * 17),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            f(xs[3], **kw)
    with pytest.raises(ValueError):
        f(np.zeros((4, spec.si + 1), np.float32), p=p)
    with pytest.raises(ValueError):
        f(xs[:-1], p=p)                                      # T meshes for T rows
    with pytest.raises(ValueError):
        f(xs[:-1], latent=lat, dlatent=dl)
    assert eng.calls == []
    with pytest.raises(ValueError) as ei:
        f(xs[3], p=p, latent=lat, dlatent=dl)
    assert "exactly one of p [T, pi] and latent [T, r]" in str(ei.value)          # worded like predict_snapshots'


def test_more_than_16_parameter_columns_refuse():
    m, eng, spec = _model(cfg_ms(r=3, si=2, pi=17))
    p = np.zeros((2, 17), np.float32)
    x = np.zeros((3, 2), np.float32)
    with pytest.raises(ValueError):
        m.predict_snapshot_parameter_derivatives(x, p=p)                          # the default is every column: 17
    with pytest.raises(ValueError):
        m.predict_snapshot_parameter_derivatives(x, p=p, p_index=list(range(17)))
    assert eng.calls == []
    assert m.predict_snapshot_parameter_derivatives(x, p=p, p_index=list(range(16)))[1].shape == (2, 3, spec.so, 16)


@pytest.mark.parametrize("role", ["p_to_lr", "p_to_w", "lr_to_w", "x_to_u_given_w", "x_to_phi"])
def test_sub_model_views_refuse(role):
    m, eng, spec = _model(CFGS["ll"], role)
    p, lat, dl, xs = _inputs(spec)
    with pytest.raises(ValueError):
        m.predict_snapshot_parameter_derivatives(xs[3], p=p)
    with pytest.raises(ValueError):
        m.predict_snapshot_parameter_derivatives(xs[3], latent=lat, dlatent=dl)
    assert eng.calls == []


@pytest.mark.parametrize("name", sorted(CFGS))
def test_shapes_and_equality_with_the_layer_on_the_expanded_table(name):
    m, eng, spec = _model(CFGS[name])
    p, lat, dl, xs = _inputs(spec)
    T, so, pi = len(RAGGED), spec.so, spec.pi
    shared = m.predict_snapshot_parameter_derivatives(xs[3], p=p)
    ragged = m.predict_snapshot_parameter_derivatives(xs, p=p)
    assert isinstance(shared, tuple) and isinstance(ragged, tuple) and len(shared) == len(ragged) == 2
    for out, lst, tail in zip(shared, ragged, [(so,), (so, pi)]):                 # the defaults: every output, every parameter column
        assert out.shape == (T, RAGGED[3]) + tail and out.dtype == np.float32
        assert isinstance(lst, list) and [a.shape for a in lst] == [(n,) + tail for n in RAGGED]
        assert all(a.dtype == np.float32 for a in lst)
    for t in range(T):
        for x, got in ((xs[3], [o[t] for o in shared]), (xs[t], [o[t] for o in ragged])):
            if not x.shape[0]:
                continue
            tab = np.hstack([np.tile(p[t], (x.shape[0], 1)), x]).astype(np.float64)
            want = O.hessian_analytic(spec, eng.ws, tab, list(range(so)), list(range(pi)))[:2]
            for g, w in zip(got, want):
                assert np.array_equal(g, w.astype(np.float32))
    # indices: one column, outputs reversed with a repeat -- passed on as given, shapes follow
    yi, pi_ = [so - 1, 0, so - 1], [pi - 1]
    eng.calls.clear()
    sub = m.predict_snapshot_parameter_derivatives(tuple(xs), p=p, p_index=pi_, y_index=yi)
    assert eng.calls == [("ragged", [n for n in RAGGED if n], tuple(yi), tuple(pi_), None)]
    assert sub[1][3].shape == (40, 3, 1) and sub[0][3].shape == (40, so)
    assert np.array_equal(sub[1][3], ragged[1][3][:, yi][:, :, pi_])
    # latent rows reach the engine as latents, each with its own directions
    eng.calls.clear()
    u, d = m.predict_snapshot_parameter_derivatives(xs[3], latent=lat, dlatent=dl)
    assert eng.calls == [("mesh", (40, spec.si)), ("shared", T, 0, 40, tuple(range(so)), None, (T, ND, spec.r))]
    assert u.shape == (T, 40, so) and d.shape == (T, 40, so, ND) and u.dtype == d.dtype == np.float32
    lu, ld = m.predict_snapshot_parameter_derivatives(xs, latent=lat, dlatent=dl, y_index=[0])
    assert [a.shape for a in lu] == [(n, so) for n in RAGGED] and [a.shape for a in ld] == [(n, 1, ND) for n in RAGGED]
    assert np.array_equal(ld[3], d[3][:, :1])                                     # snapshot 3 has the shared mesh's points


def test_empty_meshes_and_no_snapshots():
    m, eng, spec = _model(CFGS["ms"])
    p, lat, dl, xs = _inputs(spec)
    so, pi = spec.so, spec.pi
    u, d = m.predict_snapshot_parameter_derivatives(np.empty((0, spec.si), np.float32), p=p)
    assert u.shape == (len(RAGGED), 0, so) and d.shape == (len(RAGGED), 0, so, pi)
    assert m.predict_snapshot_parameter_derivatives(xs[3], p=p[:0])[1].shape == (0, RAGGED[3], so, pi)
    assert m.predict_snapshot_parameter_derivatives([], p=p[:0]) == ([], [])
    assert m.predict_snapshot_parameter_derivatives(xs[3], latent=lat[:0], dlatent=dl[:0])[1].shape == (0, RAGGED[3], so, ND)
    out = m.predict_snapshot_parameter_derivatives([xs[2]] * 2, latent=lat[:2], dlatent=dl[:2])
    assert [a.shape for a in out[1]] == [(0, so, ND)] * 2
    assert eng.calls == []


def _per_point(spec, ny, nd):
    """bytes a point holds on the device (Model.predict_snapshot_parameter_derivatives' estimate): operands, u, the latent and the
    direction tiles of a launch group, the kernels' rows over every output and the gathered results (last-layer class: and phi)"""
    ll = spec.kind == "NIFMultiScaleLastLayerParameterized"
    return 4 * (spec.pi + spec.si + spec.so + spec.r * (1 + min(nd, 3)) + (ny + spec.so) * nd + (spec.so * spec.r if ll else 0))


@pytest.mark.parametrize("given", ["p", "latent"])
def test_chunking_changes_neither_the_result_nor_what_the_engine_is_asked_for_in_total(given, monkeypatch):
    from nif_amd.model import Model
    m, eng, spec = _model(CFGS["ms"])
    p, lat, dl, xs = _inputs(spec)
    kw = dict(p=p) if given == "p" else dict(latent=lat, dlatent=dl)
    nd = spec.pi if given == "p" else ND
    tag = (tuple(range(spec.so)), tuple(range(spec.pi)), None) if given == "p" else (tuple(range(spec.so)), None, (5, ND, spec.r))
    f = m.predict_snapshot_parameter_derivatives
    whole_s = f(xs[3], **kw)
    assert eng.calls == [("mesh", (40, spec.si)), ("shared", 5, 0, 40) + tag] and eng.freed == 1
    asked_s = sorted(eng.asked)
    eng.calls.clear(); eng.asked.clear()
    whole_r = f(xs, **kw)
    assert [c[:2] for c in eng.calls] == [("ragged", [n for n in RAGGED if n])]
    asked_r = sorted(eng.asked)
    assert len(asked_s) == 5 * 40 and len(asked_r) == sum(RAGGED)
    # a budget of 16 points: the mesh itself is cut, one snapshot at a time, still one upload; the 40-point snapshot of the list is
    # cut at 16 and 32.  Every snapshot travels with its own directions
    monkeypatch.setattr(Model, "_SNAPSHOT_CHUNK_BYTES", 16 * _per_point(spec, spec.so, nd))
    eng.calls.clear(); eng.asked.clear()
    parts_s = f(xs[3], **kw)
    assert [c for c in eng.calls if c[0] == "mesh"] == [("mesh", (40, spec.si))] and eng.freed == 2
    assert [c[1:4] for c in eng.calls if c[0] == "shared"] == [(1, lo, min(40, lo + 16)) for lo in (0, 16, 32) for _ in range(5)]
    assert sorted(eng.asked) == asked_s
    eng.calls.clear(); eng.asked.clear()
    parts_r = f(xs, **kw)
    assert [c[1] for c in eng.calls] == [[1, 7], [16], [16], [8], [13]]
    assert sorted(eng.asked) == asked_r
    for a, b in zip(parts_s, whole_s):
        assert np.array_equal(a, b)
    for la, lb in zip(parts_r, whole_r):
        for a, b in zip(la, lb):
            assert np.array_equal(a, b)
    # batch_size only raises the points per chunk
    eng.calls.clear()
    f(xs[3], batch_size=200, **kw)
    assert [c[:4] for c in eng.calls] == [("mesh", (40, spec.si)), ("shared", 5, 0, 40)]

    def broken(*a):
        raise RuntimeError("device")
    eng.snapshot_param_derivatives = broken
    freed = eng.freed
    with pytest.raises(RuntimeError):
        f(xs[3], **kw)
    assert eng.freed == freed + 1                                # the mesh is freed behind a failure too


def test_the_shared_chunk_planner_still_hands_plain_rows_to_the_older_calls():
    """_snapshot_run's `extra` is optional: without it the calls get rows, not a pair"""
    m, eng, spec = _model(CFGS["ms"])
    p, lat, dl, xs = _inputs(spec)
    seen = []
    outs = m._snapshot_run("t", xs[3], p, None, None, 4, [(1,)],
                           lambda rows, il, mesh, lo, hi: (seen.append(type(rows)) or np.zeros((rows.shape[0], hi - lo, 1), np.float32),), None)
    assert seen == [np.ndarray] and outs[0].shape == (5, 40, 1)
