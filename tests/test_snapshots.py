"""Model.predict_snapshots on the host side: argument checks, result shapes, chunk planning and the one upload of a shared mesh, on an
engine double (oracle arithmetic + recorded calls).  The device path is tests/test_gpu_snapshots.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests.cfgs import cfg_ll, cfg_ms, cfg_nif


class DoubleEngine(object):
    """the three engine calls predict_snapshots makes, in fp64 oracle arithmetic; every call is recorded"""

    def __init__(self, kind, cs, cp, seed=0):
        self.ospec = O.Spec(kind, cs, cp)
        self.ws = [w.astype(np.float64) for w in O.init_weights(self.ospec, np.random.default_rng(seed), dtype=np.float32)]
        self.calls = []
        self.freed = 0

    def forward(self, x):
        return O.forward(self.ospec, self.ws, np.asarray(x, dtype=np.float64)).astype(np.float32)

    def _field(self, row, is_latent, x):
        s = self.ospec
        x = np.asarray(x, dtype=np.float64)
        if not is_latent:
            return self.forward(np.hstack([np.tile(row, (x.shape[0], 1)), x]))
        lat = np.tile(np.asarray(row, dtype=np.float64), (x.shape[0], 1))
        if s.kind == "NIFMultiScaleLastLayerParameterized":
            u = np.einsum("bsj,bj->bs", O.model_x_to_phi(s, self.ws, x), lat) + self.ws[-1]
        else:
            u = O.shapenet_given_w(s, x, O.model_lr_to_w(s, self.ws, lat))
        return u.astype(np.float32)

    def snapshot_mesh(self, x):
        self.calls.append(("mesh", np.shape(x)))
        owner = self

        class Mesh(object):
            def __init__(self, a):
                self.x = np.array(a, dtype=np.float32)

            def free(self):
                owner.freed += 1

        return Mesh(x)

    def forward_snapshots(self, rows, is_latent, mesh, lo, hi):
        self.calls.append(("shared", np.shape(rows)[0], lo, hi))
        return np.stack([self._field(r, is_latent, mesh.x[lo:hi]) for r in rows])

    def forward_snapshots_ragged(self, rows, is_latent, xs):
        assert len(xs) == np.shape(rows)[0]
        self.calls.append(("ragged", [a.shape[0] for a in xs]))
        return np.concatenate([self._field(r, is_latent, a) for r, a in zip(rows, xs)], axis=0)


def _model(cfg, role="full"):
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    kind, cs, cp = cfg
    eng = DoubleEngine(kind, cs, cp)
    owner = types.SimpleNamespace(_engine=eng, _spec=Spec(kind, cs, cp, "float32"))
    return Model(owner, role), eng, eng.ospec


CFGS = {"nif": cfg_nif(r=2, so=2, si=2, pi=2, act="tanh"), "ms": cfg_ms(r=3, si=2, pi=1), "ll": cfg_ll()}
RAGGED = [1, 7, 0, 40, 13]


def _inputs(spec, seed=1):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, size=(len(RAGGED), spec.pi)).astype(np.float32)
    lat = rng.uniform(-1, 1, size=(len(RAGGED), spec.r)).astype(np.float32)
    xs = [rng.uniform(-1, 1, size=(m, spec.si)).astype(np.float32) for m in RAGGED]
    return p, lat, xs


def test_exactly_one_of_p_and_latent_and_their_widths():
    m, eng, spec = _model(CFGS["ms"])
    p, lat, xs = _inputs(spec)
    with pytest.raises(ValueError):
        m.predict_snapshots(xs[3])
    with pytest.raises(ValueError):
        m.predict_snapshots(xs[3], p=p, latent=lat)
    with pytest.raises(ValueError):
        m.predict_snapshots(xs[3], p=lat)                       # [T, r] where [T, pi] belongs
    with pytest.raises(ValueError):
        m.predict_snapshots(xs[3], latent=p)
    with pytest.raises(ValueError):
        m.predict_snapshots(xs[3], p=p[0])                      # one row is still [1, pi]
    with pytest.raises(ValueError):
        m.predict_snapshots(np.zeros((4, spec.si + 1), np.float32), p=p)
    with pytest.raises(ValueError):
        m.predict_snapshots(xs[:-1], p=p)                       # T meshes for T rows
    with pytest.raises(ValueError):
        m.predict_snapshots(xs[:-1] + [np.zeros((3, spec.si + 1), np.float32)], p=p)
    assert eng.calls == []


@pytest.mark.parametrize("role", ["p_to_lr", "p_to_w", "lr_to_w", "x_to_u_given_w", "x_to_phi"])
def test_sub_model_views_refuse(role):
    m, eng, spec = _model(CFGS["ll"], role)
    p, lat, xs = _inputs(spec)
    with pytest.raises(ValueError):
        m.predict_snapshots(xs[3], p=p)


@pytest.mark.parametrize("name", sorted(CFGS))
@pytest.mark.parametrize("by", ["p", "latent"])
def test_shapes_and_equality_with_predict_on_the_expanded_table(name, by):
    m, eng, spec = _model(CFGS[name])
    p, lat, xs = _inputs(spec)
    kw = {"p": p} if by == "p" else {"latent": lat}
    shared = m.predict_snapshots(xs[3], **kw)
    assert shared.shape == (len(RAGGED), RAGGED[3], spec.so) and shared.dtype == np.float32
    ragged = m.predict_snapshots(xs, **kw)
    assert isinstance(ragged, list) and [a.shape for a in ragged] == [(n, spec.so) for n in RAGGED]
    assert all(a.dtype == np.float32 for a in ragged)
    assert m.predict_snapshots(tuple(xs), **kw)[1].shape == (7, spec.so)
    for t in range(len(RAGGED)):
        if by == "p":
            want_s = m.predict(np.hstack([np.tile(p[t], (RAGGED[3], 1)), xs[3]]))
            want_r = m.predict(np.hstack([np.tile(p[t], (RAGGED[t], 1)), xs[t]])) if RAGGED[t] else np.empty((0, spec.so), np.float32)
        else:
            want_s, want_r = eng._field(lat[t], True, xs[3]), eng._field(lat[t], True, xs[t])
        assert np.array_equal(shared[t], want_s)
        assert np.array_equal(ragged[t], want_r)


def test_empty_meshes_and_no_snapshots():
    m, eng, spec = _model(CFGS["ms"])
    p, lat, xs = _inputs(spec)
    assert m.predict_snapshots(np.empty((0, spec.si), np.float32), p=p).shape == (len(RAGGED), 0, spec.so)
    assert m.predict_snapshots(xs[3], p=p[:0]).shape == (0, RAGGED[3], spec.so)
    assert m.predict_snapshots([], p=p[:0]) == []
    out = m.predict_snapshots([xs[2]] * 2, p=p[:2])             # every mesh empty: nothing reaches the engine
    assert [a.shape for a in out] == [(0, spec.so)] * 2
    assert eng.calls == []


def test_shared_mesh_is_uploaded_once_and_freed_whatever_the_chunking(monkeypatch):
    from nif_amd.model import Model
    m, eng, spec = _model(CFGS["ms"])
    p, lat, xs = _inputs(spec)
    whole = m.predict_snapshots(xs[3], p=p)
    assert eng.calls == [("mesh", (40, spec.si)), ("shared", 5, 0, 40)] and eng.freed == 1
    per_point = 4 * (spec.pi + spec.si + spec.so + spec.r)
    # 100 points per chunk: two snapshots of the 40-point mesh at a time
    eng.calls.clear()
    monkeypatch.setattr(Model, "_SNAPSHOT_CHUNK_BYTES", 100 * per_point)
    assert np.array_equal(m.predict_snapshots(xs[3], p=p), whole)
    assert eng.calls == [("mesh", (40, spec.si)), ("shared", 2, 0, 40), ("shared", 2, 0, 40), ("shared", 1, 0, 40)]
    # 16 points per chunk: the mesh itself is cut, one snapshot at a time, still one upload
    eng.calls.clear()
    monkeypatch.setattr(Model, "_SNAPSHOT_CHUNK_BYTES", 16 * per_point)
    assert np.array_equal(m.predict_snapshots(xs[3], p=p), whole)
    assert [c for c in eng.calls if c[0] == "mesh"] == [("mesh", (40, spec.si))]
    assert [c[2:] for c in eng.calls if c[0] == "shared"] == [(lo, min(40, lo + 16)) for lo in (0, 16, 32) for _ in range(5)]
    assert all(c[1] == 1 for c in eng.calls if c[0] == "shared") and eng.freed == 3
    # batch_size only raises the points per chunk
    eng.calls.clear()
    assert np.array_equal(m.predict_snapshots(xs[3], p=p, batch_size=200), whole)
    assert eng.calls == [("mesh", (40, spec.si)), ("shared", 5, 0, 40)]

    def broken(*a):
        raise RuntimeError("device")
    eng.forward_snapshots = broken
    with pytest.raises(RuntimeError):
        m.predict_snapshots(xs[3], p=p)
    assert eng.freed == 5                                        # freed behind a failure too


def test_ragged_meshes_split_into_bounded_chunks(monkeypatch):
    from nif_amd.model import Model
    m, eng, spec = _model(CFGS["ll"])
    p, lat, xs = _inputs(spec)
    whole = m.predict_snapshots(xs, latent=lat)
    assert eng.calls == [("ragged", [n for n in RAGGED if n])]               # an empty mesh has no piece
    per_point = 4 * (spec.pi + spec.si + spec.so + spec.r * (1 + spec.so))
    eng.calls.clear()
    monkeypatch.setattr(Model, "_SNAPSHOT_CHUNK_BYTES", 16 * per_point)
    parts = m.predict_snapshots(xs, latent=lat)
    # 1 + 7 fit one chunk; the 40-point snapshot is cut at 16 and 32; its tail travels alone, since 13 more would overflow
    assert eng.calls == [("ragged", [1, 7]), ("ragged", [16]), ("ragged", [16]), ("ragged", [8]), ("ragged", [13])]
    assert all(sum(c[1]) <= 16 for c in eng.calls)
    for a, b in zip(parts, whole):
        assert np.array_equal(a, b)


def test_snapshot_header_exports_and_ctypes_table_are_equal():
    """include/nif_hip_snapshots.h is to SNAPSHOT_SIGNATURES what include/nif_hip.h is to SIGNATURES (tests/test_abi.py)"""
    from nif_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "nif_hip_snapshots.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(nif_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["nif_forward_snapshots", "nif_forward_snapshots_dev"] == sorted(_lib.SNAPSHOT_SIGNATURES)
    assert not set(names) & set(_lib.SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert hasattr(lib, nm), "the header declares %s but the library does not export it" % nm
    bound = _lib.load()
    for nm in names:
        assert getattr(bound, nm).argtypes == _lib.SNAPSHOT_SIGNATURES[nm][1]
