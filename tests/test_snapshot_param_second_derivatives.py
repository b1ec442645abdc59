"""Model.predict_snapshot_parameter_derivatives(order=2) without a GPU: the sixth extension header, its ctypes table and struct mirror
and the library's exports are equal, both entries pass the door of the C-ABI, the host side (argument checks, result shapes, the chunk
plan, order=1 untouched) does what it says on an engine double, and the fp64 reference of the latent route (tests/snapparam2_ref.py)
agrees with oracle.nif_oracle.hessian_analytic's parameter blocks.  The device path is
tests/test_gpu_snapshot_param_second_derivatives.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests.cfgs import cfg_ll, cfg_ms, cfg_nif
from tests.snapparam2_ref import latent_second, pnet_directions
from tests.test_snapshot_param_derivatives import SnapParamEngine, _per_point

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nif_hip_snapparam2.h")
ENTRIES = ["nif_snapshot_param_second_derivatives", "nif_snapshot_param_second_derivatives_dev"]
FIELDS = ["abi_version", "rows_are_latent", "ctx", "rows", "drows", "ddrows", "nd", "np", "p_idx", "T", "x", "offsets_host", "M", "y_idx",
          "ny", "nxc", "x_idx", "u", "dudp", "d2udp2", "dudx", "d2udpdx"]


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_exports_and_ctypes_table_are_equal():
    from nif_amd import _lib
    names = sorted(set(re.findall(r"\b(nif_[a-z0-9_]+)\s*\(", _header())))
    assert names == ENTRIES == sorted(_lib.SNAPPARAM2_SIGNATURES)
    older = (set(_lib.SIGNATURES) | set(_lib.SNAPSHOT_SIGNATURES) | set(_lib.ENCODE_SIGNATURES) | set(_lib.SNAPDERIV_SIGNATURES) |
             set(_lib.SNAPPARAM_SIGNATURES))
    assert not set(names) & older
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert hasattr(lib, nm), "the header declares %s but the library does not export it" % nm
    bound = _lib.load()
    for nm in names:
        assert getattr(bound, nm).argtypes == _lib.SNAPPARAM2_SIGNATURES[nm][1] == [ctypes.POINTER(_lib.nif_snapparam2_args)]
        assert getattr(bound, nm).restype is ctypes.c_int


def test_struct_mirror_has_the_headers_fields_size_and_offsets():
    """the header's struct laid out by the x86-64 / LP64 rules (natural alignment: int32 4, int64 and pointers 8) against ctypes'"""
    from nif_amd import _lib
    txt = _header()
    body = re.search(r"typedef\s+struct\s+nif_snapparam2_args\s*\{(.*?)\}\s*nif_snapparam2_args\s*;", txt, flags=re.S).group(1)
    fields, off = [], 0
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        m = re.match(r"^(.*?)(\w+)\s*(?:\[(\d+)\])?$", decl)
        ctype, name, count = m.group(1).strip(), m.group(2), int(m.group(3) or 1)
        size = 8 if ctype.endswith("*") else {"int32_t": 4, "int64_t": 8}[ctype]
        assert off % size == 0, "%s would sit behind implicit padding: state it as a reserved field" % name
        fields.append((name, off, size * count))
        off += size * count
    assert off % 8 == 0
    mirror = _lib.nif_snapparam2_args
    assert [f[0] for f in mirror._fields_] == [f[0] for f in fields]
    for name, o, sz in fields:
        assert (getattr(mirror, name).offset, getattr(mirror, name).size) == (o, sz), name
    assert ctypes.sizeof(mirror) == off
    assert int(re.search(r"#define\s+NIF_SNAPPARAM2_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.NIF_SNAPPARAM2_ABI_VERSION == 1
    # the fields the interface names, in its order; everything else is reserved
    assert [f[0] for f in fields if not f[0].startswith("reserved")] == FIELDS
    assert fields[-1][0] == "reserved" and fields[-1][2] == 32


def test_both_entries_pass_the_guard_in_their_own_body():
    """tests/test_entry_guard.py's rule for the entries whose context travels inside the struct: NIF_ENTER(<args>->ctx, NIF_FLUSH_TAIL);
    the struct pointer is the FIRST (and only) parameter"""
    from tests.test_entry_guard import _exports
    exports = _exports()
    for nm in ENTRIES:
        assert nm in exports, "%s is no extern \"C\" definition" % nm
        first, body = exports[nm]
        assert re.match(r"^const nif_snapparam2_args\s*\*\s*(\w+)$", first), first
        arg = first.split("*")[-1].strip()
        assert re.search(r"\bNIF_ENTER\s*\(\s*%s\s*->\s*ctx\s*,\s*NIF_FLUSH_TAIL\s*\)" % arg, body), nm


# ---- the host side on an engine double ---------------------------------------------------------------------------------------------
class SnapParam2Engine(SnapParamEngine):
    """the first-order file's double with the two second-order calls.  p rows: the fp64 oracle's HessianLayer on the expanded table,
    its parameter and mixed blocks; latent rows: tests/snapparam2_ref.latent_second.  Every call is recorded."""

    def _two(self, row, drow, ddrow, x, yi, pi_, xi):
        s = self.o
        key = np.asarray(row, np.float32).tobytes() + (b"" if drow is None else np.asarray(drow, np.float32).tobytes())
        for pt in x:
            self.asked.append((key, np.asarray(pt, np.float32).tobytes()))
        yi, xi = list(yi), list(xi)
        if drow is not None:
            u, J, H, Jx, Hx = latent_second(s, self.ws, row, drow, ddrow, x, xi)
            outs = [u, J[:, yi], H[:, yi], Jx[:, yi], Hx[:, yi]]
        else:
            nd = len(pi_)
            tab = np.hstack([np.tile(row, (x.shape[0], 1)), x]).astype(np.float64)
            u, J, H = O.hessian_analytic(s, self.ws, tab, yi, list(pi_) + [s.pi + j for j in xi])
            outs = [u, J[:, :, :nd], H[:, :, :nd, :nd], J[:, :, nd:], H[:, :, :nd, nd:]]
        return [np.asarray(o, dtype=np.float32) for o in (outs if xi else outs[:3])]

    @staticmethod
    def _tag(drows, ddrows, p_index, x_index):
        return (None if p_index is None else tuple(p_index), None if drows is None else np.shape(drows),
                None if ddrows is None else np.shape(ddrows), tuple(x_index))

    def snapshot_param_second_derivatives(self, rows, drows, ddrows, mesh, lo, hi, y_index, p_index, x_index):
        self.calls.append(("shared2", np.shape(rows)[0], lo, hi, tuple(y_index)) + self._tag(drows, ddrows, p_index, x_index))
        parts = [self._two(r, None if drows is None else drows[t], None if ddrows is None else ddrows[t], mesh.x[lo:hi], y_index, p_index, x_index)
                 for t, r in enumerate(rows)]
        return tuple(np.stack([p[i] for p in parts]) for i in range(len(parts[0])))

    def snapshot_param_second_derivatives_ragged(self, rows, drows, ddrows, xs, y_index, p_index, x_index):
        assert len(xs) == np.shape(rows)[0] and (drows is None or np.shape(drows)[0] == len(xs))
        assert ddrows is None or np.shape(ddrows)[0] == len(xs)
        self.calls.append(("ragged2", [a.shape[0] for a in xs], tuple(y_index)) + self._tag(drows, ddrows, p_index, x_index))
        parts = [self._two(r, None if drows is None else drows[t], None if ddrows is None else ddrows[t], a, y_index, p_index, x_index)
                 for t, (r, a) in enumerate(zip(rows, xs))]
        return tuple(np.concatenate([p[i] for p in parts], axis=0) for i in range(len(parts[0])))


def _model(cfg, role="full"):
    import types
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    kind, cs, cp = cfg
    eng = SnapParam2Engine(kind, cs, cp)
    owner = types.SimpleNamespace(_engine=eng, _spec=Spec(kind, cs, cp, "float32"))
    return Model(owner, role), eng, eng.o


CFGS = {"nif": cfg_nif(r=2, so=2, si=2, pi=2, act="tanh"), "ms": cfg_ms(r=3, si=2, pi=2), "ll": cfg_ll()}
RAGGED = [1, 7, 0, 40, 13]
ND = 3


def _inputs(spec, seed=1):
    rng = np.random.default_rng(seed)
    T = len(RAGGED)
    p = rng.uniform(-1, 1, size=(T, spec.pi)).astype(np.float32)
    lat = rng.uniform(-1, 1, size=(T, spec.r)).astype(np.float32)
    dl = rng.uniform(-1, 1, size=(T, ND, spec.r)).astype(np.float32)
    d2 = rng.uniform(-1, 1, size=(T, ND, ND, spec.r)).astype(np.float32)
    d2 = (d2 + d2.transpose(0, 2, 1, 3)).astype(np.float32)                      # a + a^T: symmetric bit for bit
    xs = [rng.uniform(-1, 1, size=(m, spec.si)).astype(np.float32) for m in RAGGED]
    return p, lat, dl, d2, xs


def test_argument_checks():
    m, eng, spec = _model(CFGS["ms"])
    p, lat, dl, d2, xs = _inputs(spec)
    T = len(RAGGED)
    f = m.predict_snapshot_parameter_derivatives
    skew = d2.copy()
    skew[1, 0, 2, 0] = np.nextafter(skew[1, 0, 2, 0], np.float32(9))           # one ulp off its mirror image
    bad = [
        dict(p=p, order=0), dict(p=p, order=3), dict(p=p, order="2"),          # order
        dict(p=p, order=1, x_index=[0]),                                         # x_index / d2latent belong to order=2
        dict(p=p, x_index=[0]),
        dict(latent=lat, dlatent=dl, d2latent=d2),
        dict(latent=lat, dlatent=dl, order=1, d2latent=d2),
        dict(p=p, order=2, d2latent=d2),                                         # d2latent with p
        dict(latent=lat, dlatent=np.zeros((T, 9, spec.r), np.float32), order=2),      # more than 8 directions
        dict(latent=lat, dlatent=dl, order=2, d2latent=skew),                    # not symmetric
        dict(latent=lat, dlatent=dl, order=2, d2latent=d2[:, :2]),               # wrong shapes
        dict(latent=lat, dlatent=dl, order=2, d2latent=d2[:-1]),
        dict(latent=lat, dlatent=dl, order=2, d2latent=d2[..., :-1]),
        dict(p=p, order=2, x_index=[spec.si]),                                   # a coordinate out of range
        dict(p=p, order=2, x_index=[-1]),
        dict(p=p, order=2, x_index=[0, 0]),                                      # repeated
        dict(p=p, order=2, x_index=[]),
        dict(latent=lat, dlatent=dl, order=2, x_index=[0, 1, 0]),
        dict(order=2),                                                           # the first-order checks still hold
        dict(p=p, latent=lat, dlatent=dl, order=2),
        dict(latent=lat, order=2),
        dict(p=p, order=2, p_index=[0, 0]),
        dict(p=p, order=2, y_index=[spec.so]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            f(xs[3], **kw)
    assert eng.calls == []


def test_more_than_8_parameter_columns_refuse_at_order_2_only():
    m, eng, spec = _model(cfg_ms(r=3, si=2, pi=9))
    p = np.zeros((2, 9), np.float32)
    x = np.zeros((3, 2), np.float32)
    with pytest.raises(ValueError):
        m.predict_snapshot_parameter_derivatives(x, p=p, order=2)                # the default is every column: 9
    assert eng.calls == []
    assert m.predict_snapshot_parameter_derivatives(x, p=p)[1].shape == (2, 3, spec.so, 9)
    out = m.predict_snapshot_parameter_derivatives(x, p=p, order=2, p_index=list(range(8)))
    assert out[2].shape == (2, 3, spec.so, 8, 8)


@pytest.mark.parametrize("role", ["p_to_lr", "p_to_w", "lr_to_w", "x_to_u_given_w", "x_to_phi"])
def test_sub_model_views_refuse(role):
    m, eng, spec = _model(CFGS["ll"], role)
    p, lat, dl, d2, xs = _inputs(spec)
    with pytest.raises(ValueError):
        m.predict_snapshot_parameter_derivatives(xs[3], p=p, order=2)
    assert eng.calls == []


@pytest.mark.parametrize("name", sorted(CFGS))
def test_shapes_and_equality_with_the_layer_on_the_expanded_table(name):
    m, eng, spec = _model(CFGS[name])
    p, lat, dl, d2, xs = _inputs(spec)
    T, so, pi, si = len(RAGGED), spec.so, spec.pi, spec.si
    f = m.predict_snapshot_parameter_derivatives
    for xi in (None, [si - 1, 0]):
        nx = 0 if xi is None else len(xi)
        kw = dict(order=2) if xi is None else dict(order=2, x_index=xi)
        tails = [(so,), (so, pi), (so, pi, pi)] + ([(so, nx), (so, pi, nx)] if nx else [])
        shared = f(xs[3], p=p, **kw)
        ragged = f(xs, p=p, **kw)
        assert isinstance(shared, tuple) and isinstance(ragged, tuple) and len(shared) == len(ragged) == len(tails)
        for out, lst, tail in zip(shared, ragged, tails):
            assert out.shape == (T, RAGGED[3]) + tail and out.dtype == np.float32
            assert isinstance(lst, list) and [a.shape for a in lst] == [(n,) + tail for n in RAGGED]
        cols = list(range(pi)) + [pi + j for j in (xi or [])]
        for t in range(T):
            for x, got in ((xs[3], [o[t] for o in shared]), (xs[t], [o[t] for o in ragged])):
                if not x.shape[0]:
                    continue
                tab = np.hstack([np.tile(p[t], (x.shape[0], 1)), x]).astype(np.float64)
                u, J, H = O.hessian_analytic(spec, eng.ws, tab, list(range(so)), cols)
                want = [u, J[:, :, :pi], H[:, :, :pi, :pi]] + ([J[:, :, pi:], H[:, :, :pi, pi:]] if nx else [])
                for g, w in zip(got, want):
                    assert np.array_equal(g, w.astype(np.float32))
    # latent rows reach the engine as latents, each with its own directions and second directions
    eng.calls.clear()
    out = f(xs[3], latent=lat, dlatent=dl, d2latent=d2, order=2, x_index=[0])
    assert eng.calls == [("mesh", (40, si)), ("shared2", T, 0, 40, tuple(range(so)), None, (T, ND, spec.r), (T, ND, ND, spec.r), (0,))]
    assert [o.shape for o in out] == [(T, 40, so), (T, 40, so, ND), (T, 40, so, ND, ND), (T, 40, so, 1), (T, 40, so, ND, 1)]
    eng.calls.clear()
    lo = f(xs, latent=lat, dlatent=dl, order=2, y_index=[0])
    assert eng.calls == [("ragged2", [n for n in RAGGED if n], (0,), None, (T - 1, ND, spec.r), None, ())]
    assert [a.shape for a in lo[2]] == [(n, 1, ND, ND) for n in RAGGED] and len(lo) == 3
    # the snapshot that has the shared mesh's points, without d2latent: the d2latent term is what differs
    only = f(xs[3], latent=lat, dlatent=dl, order=2, y_index=[0])
    assert np.array_equal(lo[2][3], only[2][3])


def test_empty_meshes_and_no_snapshots():
    m, eng, spec = _model(CFGS["ms"])
    p, lat, dl, d2, xs = _inputs(spec)
    so, pi = spec.so, spec.pi
    f = m.predict_snapshot_parameter_derivatives
    out = f(np.empty((0, spec.si), np.float32), p=p, order=2, x_index=[1])
    assert [o.shape for o in out] == [(5, 0, so), (5, 0, so, pi), (5, 0, so, pi, pi), (5, 0, so, 1), (5, 0, so, pi, 1)]
    assert f(xs[3], p=p[:0], order=2)[2].shape == (0, RAGGED[3], so, pi, pi)
    assert f([], p=p[:0], order=2) == ([], [], [])
    out = f([xs[2]] * 2, latent=lat[:2], dlatent=dl[:2], d2latent=d2[:2], order=2)
    assert [a.shape for a in out[2]] == [(0, so, ND, ND)] * 2
    assert eng.calls == []


def _per_point2(spec, ny, nd, nx):
    """the first order's bytes per point and the new rows: the pair and mixed results over every output, the gathered ones and the
    first-order coordinate rows"""
    return _per_point(spec, ny, nd) + 4 * (ny + spec.so) * (nd * nd + nd * nx + nx)


@pytest.mark.parametrize("given", ["p", "latent"])
def test_chunking_changes_neither_the_result_nor_what_the_engine_is_asked_for_in_total(given, monkeypatch):
    from nif_amd.model import Model
    m, eng, spec = _model(CFGS["ms"])
    p, lat, dl, d2, xs = _inputs(spec)
    kw = dict(p=p, order=2, x_index=[0]) if given == "p" else dict(latent=lat, dlatent=dl, d2latent=d2, order=2, x_index=[0])
    nd = spec.pi if given == "p" else ND
    f = m.predict_snapshot_parameter_derivatives
    whole_s = f(xs[3], **kw)
    assert [c[:4] for c in eng.calls] == [("mesh", (40, spec.si)), ("shared2", 5, 0, 40)] and eng.freed == 1
    asked_s = sorted(eng.asked)
    eng.calls.clear(); eng.asked.clear()
    whole_r = f(xs, **kw)
    assert [c[:2] for c in eng.calls] == [("ragged2", [n for n in RAGGED if n])]
    asked_r = sorted(eng.asked)
    assert len(asked_s) == 5 * 40 and len(asked_r) == sum(RAGGED)
    # a budget of 16 points: the planner's per_point count has grown by the new rows
    monkeypatch.setattr(Model, "_SNAPSHOT_CHUNK_BYTES", 16 * _per_point2(spec, spec.so, nd, 1))
    eng.calls.clear(); eng.asked.clear()
    parts_s = f(xs[3], **kw)
    assert [c for c in eng.calls if c[0] == "mesh"] == [("mesh", (40, spec.si))] and eng.freed == 2
    assert [c[1:4] for c in eng.calls if c[0] == "shared2"] == [(1, lo, min(40, lo + 16)) for lo in (0, 16, 32) for _ in range(5)]
    assert sorted(eng.asked) == asked_s
    eng.calls.clear(); eng.asked.clear()
    parts_r = f(xs, **kw)
    assert [c[1] for c in eng.calls] == [[1, 7], [16], [16], [8], [13]]
    if given == "latent":                       # every snapshot travels with its own directions and second directions
        assert [c[4] for c in eng.calls] == [(2, ND, spec.r), (1, ND, spec.r), (1, ND, spec.r), (1, ND, spec.r), (1, ND, spec.r)]
        assert [c[5] for c in eng.calls] == [(2, ND, ND, spec.r)] + [(1, ND, ND, spec.r)] * 4
    assert sorted(eng.asked) == asked_r
    assert len(parts_s) == len(whole_s) == 5
    for a, b in zip(parts_s, whole_s):
        assert np.array_equal(a, b)
    for la, lb in zip(parts_r, whole_r):
        for a, b in zip(la, lb):
            assert np.array_equal(a, b)

    def broken(*a):
        raise RuntimeError("device")
    eng.snapshot_param_second_derivatives = broken
    freed = eng.freed
    with pytest.raises(RuntimeError):
        f(xs[3], **kw)
    assert eng.freed == freed + 1                                # the mesh is freed behind a failure too


def test_order_1_makes_the_engine_calls_it_made_before():
    m, eng, spec = _model(CFGS["ms"])
    p, lat, dl, d2, xs = _inputs(spec)
    so, pi = spec.so, spec.pi
    f = m.predict_snapshot_parameter_derivatives
    for kw in (dict(), dict(order=1)):
        eng.calls.clear()
        a = f(xs[3], p=p, **kw)
        b = f(xs, p=p, p_index=[1], y_index=[0], **kw)
        c = f(xs[3], latent=lat, dlatent=dl, **kw)
        assert eng.calls == [
            ("mesh", (40, spec.si)), ("shared", 5, 0, 40, tuple(range(so)), tuple(range(pi)), None),
            ("ragged", [n for n in RAGGED if n], (0,), (1,), None),
            ("mesh", (40, spec.si)), ("shared", 5, 0, 40, tuple(range(so)), None, (5, ND, spec.r))]
        assert len(a) == len(b) == len(c) == 2
    # u and dudp of the order=2 call are what the order=1 call returns (on the double: the same oracle)
    two = f(xs[3], p=p, order=2)
    assert np.array_equal(two[0], a[0]) and np.array_equal(two[1], a[1])
    assert np.array_equal(two[2], two[2].transpose(0, 1, 2, 4, 3))


# ---- the fp64 reference of the latent route against the oracle ---------------------------------------------------------------------
# Measured (x86-64, glibc, numpy + torch float64): the worst relative L2 distance over the blocks and the snapshots is 1.32e-15 on "ms"
# (5.3e-16 on "nif", 3.9e-16 on "ll"): sums of float64 products taken in two different orders.  The bar is ten times the worst, so
# that another platform's libm does not trip it.
REF_MEASURED, REF_BAR = 1.32e-15, 1.32e-14


@pytest.mark.parametrize("name", sorted(CFGS))
def test_the_latent_reference_with_the_oracles_pnet_tangents_is_the_oracles_parameter_blocks(name):
    """latent_second at z(p) along dz/dp with d2latent = d2z/dp2 (oracle.nif_oracle.pnet_tangents2) is hessian_analytic's J and H on
    the parameter columns and its mixed block, by the chain rule"""
    kind, cs, cp = CFGS[name]
    spec = O.Spec(kind, cs, cp)
    ws = [np.asarray(w, dtype=np.float64) for w in O.init_weights(spec, np.random.default_rng(0), dtype=np.float32)]
    if kind != O.KIND_NIF:      # (weight_init_factor 0.01 leaves the latent next to no say in the field: a usable scale)
        i = [nm for nm, _ in spec.param_shapes()].index("pnet_last_w")
        ws[i] = ws[i] * (30.0 if kind == O.KIND_LL else 2.0)
    rng = np.random.default_rng(3)
    T, M = 3, 17
    p = rng.uniform(-1, 1, size=(T, spec.pi))
    x = rng.uniform(-1, 1, size=(M, spec.si))
    cols, xi = list(range(spec.pi)), list(range(spec.si))
    z, dz, ddz = pnet_directions(spec, ws, p, cols)
    worst = 0.0
    for t in range(T):
        tab = np.hstack([np.tile(p[t], (M, 1)), x])
        u, J, H = O.hessian_analytic(spec, ws, tab, list(range(spec.so)), cols + [spec.pi + j for j in xi])
        got = latent_second(spec, ws, z[t], dz[t], ddz[t], x, xi)
        want = [u, J[:, :, :spec.pi], H[:, :, :spec.pi, :spec.pi], J[:, :, spec.pi:], H[:, :, :spec.pi, spec.pi:]]
        for what, g, w in zip(("u", "dudp", "d2udp2", "dudx", "d2udpdx"), got, want):
            assert g.shape == w.shape
            rel = np.linalg.norm(g - w) / np.linalg.norm(w)
            print("%s snapshot %d %s: rel-L2 %.3e" % (name, t, what, rel))
            worst = max(worst, rel)
    print("%s: worst %.3e (measured %.1e, bar %.1e)" % (name, worst, REF_MEASURED, REF_BAR))
    assert worst < REF_BAR
