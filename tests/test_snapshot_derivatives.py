"""Model.predict_snapshot_derivatives without a GPU: the fourth extension header, its ctypes table and struct mirror and the library's
exports are equal, both entries pass the door of the C-ABI, and the host side (argument checks, result shapes, the chunk plan) does
what it says on an engine double.  The device path is tests/test_gpu_snapshot_derivatives.py."""
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
HEADER = os.path.join(ROOT, "include", "nif_hip_snapderiv.h")
ENTRIES = ["nif_snapshot_derivatives", "nif_snapshot_derivatives_dev"]
FIELDS = ["abi_version", "order", "ctx", "rows", "rows_are_latent", "T", "x", "offsets_host", "M", "y_idx", "ny", "x_idx", "nx", "u",
          "dudx", "d2udx2"]


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_exports_and_ctypes_table_are_equal():
    from nif_amd import _lib
    names = sorted(set(re.findall(r"\b(nif_[a-z0-9_]+)\s*\(", _header())))
    assert names == ENTRIES == sorted(_lib.SNAPDERIV_SIGNATURES)
    assert not set(names) & (set(_lib.SIGNATURES) | set(_lib.SNAPSHOT_SIGNATURES) | set(_lib.ENCODE_SIGNATURES))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert hasattr(lib, nm), "the header declares %s but the library does not export it" % nm
    bound = _lib.load()
    for nm in names:
        assert getattr(bound, nm).argtypes == _lib.SNAPDERIV_SIGNATURES[nm][1] == [ctypes.POINTER(_lib.nif_snapderiv_args)]
        assert getattr(bound, nm).restype is ctypes.c_int


def test_struct_mirror_has_the_headers_fields_size_and_offsets():
    """the header's struct laid out by the x86-64 / LP64 rules (natural alignment: int32 4, int64 and pointers 8) against ctypes'"""
    from nif_amd import _lib
    txt = _header()
    body = re.search(r"typedef\s+struct\s+nif_snapderiv_args\s*\{(.*?)\}\s*nif_snapderiv_args\s*;", txt, flags=re.S).group(1)
    fields, off = [], 0
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        m = re.match(r"^(.*?)(\w+)\s*(?:\[(\d+)\])?$", decl)
        ctype, name, count = m.group(1).strip(), m.group(2), int(m.group(3) or 1)
        size = 8 if ctype.endswith("*") else {"int32_t": 4, "int64_t": 8}[ctype]
        assert off % size == 0, "%s would sit behind implicit padding: state it as a reserved field" % name
        fields.append((name, off, size * count))
        off += size * count
    assert off % 8 == 0
    mirror = _lib.nif_snapderiv_args
    assert [f[0] for f in mirror._fields_] == [f[0] for f in fields]
    for name, o, sz in fields:
        assert (getattr(mirror, name).offset, getattr(mirror, name).size) == (o, sz), name
    assert ctypes.sizeof(mirror) == off
    assert int(re.search(r"#define\s+NIF_SNAPDERIV_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.NIF_SNAPDERIV_ABI_VERSION
    # the fields the interface names, in its order; everything else is reserved
    assert [f[0] for f in fields if not f[0].startswith("reserved")] == FIELDS
    assert fields[-1][0] == "reserved" and fields[-1][2] == 32


def test_both_entries_pass_the_guard_in_their_own_body():
    """tests/test_entry_guard.py's rule for the entries whose context travels inside the struct: NIF_ENTER(<args>->ctx, NIF_FLUSH_TAIL)"""
    from tests.test_entry_guard import _exports
    exports = _exports()
    for nm in ENTRIES:
        assert nm in exports, "%s is no extern \"C\" definition" % nm
        first, body = exports[nm]
        assert re.match(r"^const nif_snapderiv_args\s*\*\s*(\w+)$", first), first
        arg = first.split("*")[-1].strip()
        assert re.search(r"\bNIF_ENTER\s*\(\s*%s\s*->\s*ctx\s*,\s*NIF_FLUSH_TAIL\s*\)" % arg, body), nm


# ---- the host side on an engine double ---------------------------------------------------------------------------------------------
class SnapDerivEngine(OracleEngine):
    """tests/doubles.py's engine with the three calls predict_snapshot_derivatives makes.  p rows: the fp64 oracle's HessianLayer on the
    expanded table; latent rows: a stand-in that depends on the row and the points (the device path is tested on the GPU).  Every
    call is recorded with the points it was asked for."""

    def __init__(self, kind, cs, cp, seed=0):
        ospec = O.Spec(kind, cs, cp)
        OracleEngine.__init__(self, ospec, O.init_weights(ospec, np.random.default_rng(seed), dtype=np.float32))
        self.ws = O.unflatten(ospec, self.theta)
        self.freed = 0
        self.asked = []      # (snapshot's row as bytes, point as bytes) of every point an engine call was asked for

    def snapshot_mesh(self, x):
        self.calls.append(("mesh", np.shape(x)))
        owner = self

        class Mesh(object):
            def __init__(self, a):
                self.x = np.array(a, dtype=np.float32)

            def free(self):
                owner.freed += 1

        return Mesh(x)

    def _one(self, row, is_latent, x, yi, xi, order):
        s = self.o
        for pt in x:
            self.asked.append((np.asarray(row, np.float32).tobytes(), np.asarray(pt, np.float32).tobytes()))
        if is_latent:
            u = np.outer(np.sin(x.sum(axis=1)), np.ones(s.so)) * float(np.sum(row))
            d = np.zeros((x.shape[0], len(yi), len(xi))) + u[:, :1, None]
            h = np.zeros((x.shape[0], len(yi), len(xi), len(xi))) + u[:, :1, None, None]
        else:
            tab = np.hstack([np.tile(row, (x.shape[0], 1)), x]).astype(np.float64)
            u, d, h = O.hessian_analytic(s, self.ws, tab, yi, [s.pi + j for j in xi])
        outs = (u, d, h) if order == 2 else (u, d)
        return tuple(np.asarray(o, dtype=np.float32) for o in outs)

    def snapshot_derivatives(self, rows, is_latent, mesh, lo, hi, y_index, x_index, order):
        self.calls.append(("shared", np.shape(rows)[0], lo, hi, tuple(y_index), tuple(x_index), order))
        parts = [self._one(r, is_latent, mesh.x[lo:hi], y_index, x_index, order) for r in rows]
        return tuple(np.stack([p[i] for p in parts]) for i in range(len(parts[0])))

    def snapshot_derivatives_ragged(self, rows, is_latent, xs, y_index, x_index, order):
        assert len(xs) == np.shape(rows)[0]
        self.calls.append(("ragged", [a.shape[0] for a in xs], tuple(y_index), tuple(x_index), order))
        parts = [self._one(r, is_latent, a, y_index, x_index, order) for r, a in zip(rows, xs)]
        return tuple(np.concatenate([p[i] for p in parts], axis=0) for i in range(len(parts[0])))


def _model(cfg, role="full"):
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    kind, cs, cp = cfg
    eng = SnapDerivEngine(kind, cs, cp)
    owner = types.SimpleNamespace(_engine=eng, _spec=Spec(kind, cs, cp, "float32"))
    return Model(owner, role), eng, eng.o


CFGS = {"nif": cfg_nif(r=2, so=2, si=2, pi=2, act="tanh"), "ms": cfg_ms(r=3, si=2, pi=1), "ll": cfg_ll()}
RAGGED = [1, 7, 0, 40, 13]


def _inputs(spec, seed=1):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, size=(len(RAGGED), spec.pi)).astype(np.float32)
    lat = rng.uniform(-1, 1, size=(len(RAGGED), spec.r)).astype(np.float32)
    xs = [rng.uniform(-1, 1, size=(m, spec.si)).astype(np.float32) for m in RAGGED]
    return p, lat, xs


def test_argument_checks():
    m, eng, spec = _model(CFGS["ms"])
    p, lat, xs = _inputs(spec)
    f = m.predict_snapshot_derivatives
    bad = [
        dict(),                                          # neither p nor latent
        dict(p=p, latent=lat),                           # both
        dict(p=lat),                                     # [T, r] where [T, pi] belongs
        dict(latent=p),
        dict(p=p[0]),
        dict(p=p, x_index=[spec.si]),                    # a coordinate index out of range
        dict(p=p, x_index=[-1]),
        dict(p=p, x_index=[0, 0]),                       # repeated
        dict(p=p, x_index=[]),
        dict(p=p, y_index=[spec.so]),
        dict(p=p, y_index=[0] * 17),                     # more than 16 entries
        dict(p=p, order=3),
        dict(p=p, order=0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            f(xs[3], **kw)
    with pytest.raises(ValueError):
        f(np.zeros((4, spec.si + 1), np.float32), p=p)
    with pytest.raises(ValueError):
        f(xs[:-1], p=p)                                  # T meshes for T rows
    assert eng.calls == []
    with pytest.raises(ValueError) as ei:
        f(xs[3], p=p, latent=lat)
    assert "exactly one of p [T, pi] and latent [T, r]" in str(ei.value)          # worded like predict_snapshots'


@pytest.mark.parametrize("role", ["p_to_lr", "p_to_w", "lr_to_w", "x_to_u_given_w", "x_to_phi"])
def test_sub_model_views_refuse(role):
    m, eng, spec = _model(CFGS["ll"], role)
    p, lat, xs = _inputs(spec)
    with pytest.raises(ValueError):
        m.predict_snapshot_derivatives(xs[3], p=p)


@pytest.mark.parametrize("name", sorted(CFGS))
@pytest.mark.parametrize("order", [1, 2])
def test_shapes_and_equality_with_the_hessian_on_the_expanded_table(name, order):
    m, eng, spec = _model(CFGS[name])
    p, lat, xs = _inputs(spec)
    T, so, si = len(RAGGED), spec.so, spec.si
    shared = m.predict_snapshot_derivatives(xs[3], p=p, order=order)
    ragged = m.predict_snapshot_derivatives(xs, p=p, order=order)
    assert isinstance(shared, tuple) and isinstance(ragged, tuple) and len(shared) == len(ragged) == order + 1
    tails = [(so,), (so, si), (so, si, si)][:order + 1]                           # the defaults: every output, every coordinate
    for out, lst, tail in zip(shared, ragged, tails):
        assert out.shape == (T, RAGGED[3]) + tail and out.dtype == np.float32
        assert isinstance(lst, list) and [a.shape for a in lst] == [(n,) + tail for n in RAGGED]
        assert all(a.dtype == np.float32 for a in lst)
    xi_all = [spec.pi + j for j in range(si)]
    for t in range(T):
        for x, got in ((xs[3], [o[t] for o in shared]), (xs[t], [o[t] for o in ragged])):
            if not x.shape[0]:
                continue
            tab = np.hstack([np.tile(p[t], (x.shape[0], 1)), x]).astype(np.float64)
            want = O.hessian_analytic(spec, eng.ws, tab, list(range(so)), xi_all)
            for g, w in zip(got, want):
                assert np.array_equal(g, w.astype(np.float32))
    # indices: a subset in non-natural order, outputs reversed with a repeat -- passed on as given, shapes follow
    yi, xi = [so - 1, 0, so - 1], [si - 1, 0]
    eng.calls.clear()
    sub = m.predict_snapshot_derivatives(tuple(xs), p=p, x_index=xi, y_index=yi, order=order)
    assert eng.calls == [("ragged", [n for n in RAGGED if n], tuple(yi), tuple(xi), order)]
    assert sub[1][3].shape == (40, 3, 2) and sub[0][3].shape == (40, so)
    assert np.array_equal(sub[1][3], ragged[1][3][:, yi][:, :, xi])
    if order == 2:
        assert np.array_equal(sub[2][3], ragged[2][3][:, yi][:, :, xi][:, :, :, xi])
    # latent rows reach the engine as latents
    eng.calls.clear()
    out = m.predict_snapshot_derivatives(xs[3], latent=lat, order=order)
    assert eng.calls[0] == ("mesh", (40, si)) and eng.calls[1][:2] == ("shared", T)
    assert out[0].shape == (T, 40, so)


def test_empty_meshes_and_no_snapshots():
    m, eng, spec = _model(CFGS["ms"])
    p, lat, xs = _inputs(spec)
    so, si = spec.so, spec.si
    u, d, h = m.predict_snapshot_derivatives(np.empty((0, si), np.float32), p=p, order=2)
    assert u.shape == (len(RAGGED), 0, so) and d.shape == (len(RAGGED), 0, so, si) and h.shape == (len(RAGGED), 0, so, si, si)
    assert m.predict_snapshot_derivatives(xs[3], p=p[:0])[1].shape == (0, RAGGED[3], so, si)
    assert m.predict_snapshot_derivatives([], p=p[:0]) == ([], [])
    out = m.predict_snapshot_derivatives([xs[2]] * 2, p=p[:2], order=2)
    assert [a.shape for a in out[2]] == [(0, so, si, si)] * 2
    assert eng.calls == []


@pytest.mark.parametrize("order", [1, 2])
def test_chunking_changes_neither_the_result_nor_what_the_engine_is_asked_for_in_total(order, monkeypatch):
    from nif_amd.model import Model
    m, eng, spec = _model(CFGS["ms"])
    p, lat, xs = _inputs(spec)
    whole_s = m.predict_snapshot_derivatives(xs[3], p=p, order=order)
    assert eng.calls == [("mesh", (40, spec.si)), ("shared", 5, 0, 40, (0,), (0, 1), order)] and eng.freed == 1
    asked_s = sorted(eng.asked)
    eng.calls.clear(); eng.asked.clear()
    whole_r = m.predict_snapshot_derivatives(xs, p=p, order=order)
    assert eng.calls == [("ragged", [n for n in RAGGED if n], (0,), (0, 1), order)]
    asked_r = sorted(eng.asked)
    assert len(asked_s) == 5 * 40 and len(asked_r) == sum(RAGGED)
    # a budget of 16 points: the mesh itself is cut, one snapshot at a time, still one upload; the 40-point snapshot of the list is
    # cut at 16 and 32
    monkeypatch.setattr(Model, "_SNAPSHOT_CHUNK_BYTES", 16 * _per_point(spec, spec.so, spec.si))
    eng.calls.clear(); eng.asked.clear()
    parts_s = m.predict_snapshot_derivatives(xs[3], p=p, order=order)
    assert [c for c in eng.calls if c[0] == "mesh"] == [("mesh", (40, spec.si))] and eng.freed == 2
    assert [c[1:4] for c in eng.calls if c[0] == "shared"] == [(1, lo, min(40, lo + 16)) for lo in (0, 16, 32) for _ in range(5)]
    assert sorted(eng.asked) == asked_s
    eng.calls.clear(); eng.asked.clear()
    parts_r = m.predict_snapshot_derivatives(xs, p=p, order=order)
    assert [c[1] for c in eng.calls] == [[1, 7], [16], [16], [8], [13]]
    assert sorted(eng.asked) == asked_r
    for a, b in zip(parts_s, whole_s):
        assert np.array_equal(a, b)
    for la, lb in zip(parts_r, whole_r):
        for a, b in zip(la, lb):
            assert np.array_equal(a, b)
    # batch_size only raises the points per chunk
    eng.calls.clear()
    m.predict_snapshot_derivatives(xs[3], p=p, order=order, batch_size=200)
    assert [c[:4] for c in eng.calls] == [("mesh", (40, spec.si)), ("shared", 5, 0, 40)]

    def broken(*a):
        raise RuntimeError("device")
    eng.snapshot_derivatives = broken
    freed = eng.freed
    with pytest.raises(RuntimeError):
        m.predict_snapshot_derivatives(xs[3], p=p, order=order)
    assert eng.freed == freed + 1                                # the mesh is freed behind a failure too


def _per_point(spec, ny, nx):
    """bytes a point holds on the device (Model.predict_snapshot_derivatives' estimate): operands, u, the latent, the kernels' rows over
    every output (last-layer class: over the so * r rows of phi, and phi itself) and the gathered results"""
    ll = spec.kind == "NIFMultiScaleLastLayerParameterized"
    krows = spec.so * (spec.r if ll else 1)
    return 4 * (spec.pi + spec.si + spec.so + spec.r + krows + (ny + krows) * (nx + nx * nx))
