"""Model.encode_snapshots without a GPU: the float64 references agree with each other (tests/encode_ref.py), the third extension header,
its ctypes table and struct mirror and the library's exports are equal, both entries pass the door of the C-ABI, and the
Levenberg-Marquardt loop of nif_amd/encode.py does what it says on an engine double whose normal equations come from the reference.
The device path is tests/test_gpu_encode.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import encode_ref as R
from tests.cfgs import cfg_ll, cfg_ms, cfg_nif

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nif_hip_encode.h")
ENTRIES = ["nif_snapshot_normal_eq", "nif_snapshot_normal_eq_dev"]

CFGS = {"nif": cfg_nif(r=2, so=2, si=2, pi=2, act="tanh"), "ms": cfg_ms(r=3, si=2, pi=1), "ll": cfg_ll()}


def _gpu_nets():
    """the nets of tests/test_gpu_encode.py (the references must hold on them too)"""
    return {name: R.net_cfg(name) for name in R.NETS}


def _all_nets():
    nets = dict(("cpu_" + k, v) for k, v in CFGS.items())
    nets.update(_gpu_nets())
    return nets


# ---- the references ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_all_nets()))
def test_central_differences_and_autograd_agree_on_the_latent_jacobian(name):
    kind, cs, cp = _all_nets()[name]
    eng = R.RefEngine(kind, cs, cp)
    spec, ws = eng.ospec, eng.ws
    rng = np.random.default_rng(3)
    z = rng.uniform(-1, 1, size=spec.r)
    x = rng.uniform(-1, 1, size=(9, spec.si))
    u_t, j_t = R.field_and_jac(spec, ws, z, x)
    u_o = R.field(spec, ws, z, x)
    j_f = R.jac_fd(spec, ws, z, x)
    assert j_t.shape == (9, spec.so, spec.r)
    assert np.linalg.norm(u_t - u_o) <= 1e-12 * np.linalg.norm(u_o)
    err = np.linalg.norm(j_f - j_t) / np.linalg.norm(j_t)
    print("%s: |J_fd - J_autograd| / |J| = %.3g" % (name, err))
    assert err <= 1e-7


def test_gram_holds_the_normal_equations():
    kind, cs, cp = CFGS["ms"]
    eng = R.RefEngine(kind, cs, cp)
    spec, r = eng.ospec, eng.ospec.r
    rng = np.random.default_rng(4)
    x, y, w = rng.uniform(-1, 1, size=(11, spec.si)), rng.uniform(-1, 1, size=(11, spec.so)), rng.uniform(0.5, 1.5, size=11)
    z = rng.uniform(-1, 1, size=(1, r))
    S = R.normal_eq(spec, eng.ws, z, [x], [y], [w])[0]
    u, J = R.field_and_jac(spec, eng.ws, z[0], x)
    Jm, e = J.reshape(-1, r), (u - y).reshape(-1)
    W = np.repeat(w, spec.so)
    assert np.allclose(S[:r, :r], Jm.T @ (W[:, None] * Jm), rtol=1e-13, atol=0)
    assert np.allclose(S[:r, r], Jm.T @ (W * e), rtol=1e-12, atol=1e-15)
    assert np.isclose(S[r, r], np.sum(W * e * e), rtol=1e-13)
    assert np.array_equal(S, S.T)


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_encode_header_exports_and_ctypes_table_are_equal():
    from nif_amd import _lib
    names = sorted(set(re.findall(r"\b(nif_[a-z0-9_]+)\s*\(", _header())))
    assert names == ENTRIES == sorted(_lib.ENCODE_SIGNATURES)
    assert not set(names) & (set(_lib.SIGNATURES) | set(_lib.SNAPSHOT_SIGNATURES))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert hasattr(lib, nm), "the header declares %s but the library does not export it" % nm
    bound = _lib.load()
    for nm in names:
        assert getattr(bound, nm).argtypes == _lib.ENCODE_SIGNATURES[nm][1] == [ctypes.POINTER(_lib.nif_encode_args)]
        assert getattr(bound, nm).restype is ctypes.c_int


def test_struct_mirror_has_the_headers_fields_size_and_offsets():
    """the header's struct laid out by the x86-64 / LP64 rules (natural alignment: int32 4, int64 and pointers 8) against ctypes'"""
    from nif_amd import _lib
    txt = _header()
    body = re.search(r"typedef\s+struct\s+nif_encode_args\s*\{(.*?)\}\s*nif_encode_args\s*;", txt, flags=re.S).group(1)
    fields, off = [], 0
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        m = re.match(r"^(.*?)(\w+)\s*(?:\[(\d+)\])?$", decl)
        ctype, name, count = m.group(1).strip(), m.group(2), int(m.group(3) or 1)
        size = 8 if ctype.endswith("*") else {"int32_t": 4, "int64_t": 8}[ctype]
        off = (off + size - 1) // size * size
        fields.append((name, off, size * count))
        off += size * count
    total = (off + 7) // 8 * 8
    mirror = _lib.nif_encode_args
    assert [f[0] for f in mirror._fields_] == [f[0] for f in fields]
    for name, o, sz in fields:
        assert (getattr(mirror, name).offset, getattr(mirror, name).size) == (o, sz), name
    assert ctypes.sizeof(mirror) == total
    assert int(re.search(r"#define\s+NIF_ENCODE_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.NIF_ENCODE_ABI_VERSION
    assert [f[0] for f in fields][:2] == ["abi_version", "reserved0"] and fields[-1][0] == "reserved"


def test_both_entries_pass_the_guard_in_their_own_body():
    """tests/test_entry_guard.py's rule for the entries whose context travels inside the struct: NIF_ENTER(<args>->ctx, NIF_FLUSH_TAIL)"""
    from tests.test_entry_guard import _exports
    exports = _exports()
    for nm in ENTRIES:
        assert nm in exports, "%s is no extern \"C\" definition" % nm
        first, body = exports[nm]
        assert re.match(r"^const nif_encode_args\s*\*\s*(\w+)$", first), first
        arg = first.split("*")[-1].strip()
        assert re.search(r"\bNIF_ENTER\s*\(\s*%s\s*->\s*ctx\s*,\s*NIF_FLUSH_TAIL\s*\)" % arg, body), nm


# ---- the Levenberg-Marquardt loop on the engine double -----------------------------------------------------------------------------
def _model(cfg, role="full"):
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    kind, cs, cp = cfg
    eng = R.RefEngine(kind, cs, cp)
    owner = types.SimpleNamespace(_engine=eng, _spec=Spec(kind, cs, cp, "float32"))
    return Model(owner, role), eng, eng.ospec


COUNTS = [12, 7, 0, 40, 33]
DELTA = 0.02


def _problem(name, seed=5, counts=COUNTS, delta=DELTA):
    """fields of known latents z* on ragged meshes, and the perturbed start z* + delta"""
    m, eng, spec = _model(CFGS[name])
    rng = np.random.default_rng(seed)
    T = len(counts)
    zs = rng.uniform(-1, 1, size=(T, spec.r)).astype(np.float32)
    xs = [rng.uniform(-1, 1, size=(n, spec.si)).astype(np.float32) for n in counts]
    us = [R.field(spec, eng.ws, zs[t], xs[t]).astype(np.float32) for t in range(T)]
    z0 = (zs + delta * rng.uniform(-1, 1, size=zs.shape)).astype(np.float32)
    return m, eng, spec, zs, xs, us, z0


def _recovery_bound(spec, ws, z, x, u):
    """how far the least-squares latent of float32 samples may sit from z*: the samples carry a rounding eta, |eta| <= 2^-24 |u|, the
    minimiser moves by A^-1 J^T eta, |.| <= |A^-1|_2 sqrt(tr A) |eta|; the float32 latent itself adds 2^-24 |z|.  Ten times that"""
    _, J = R.field_and_jac(spec, ws, z, x)
    Jm = J.reshape(-1, spec.r)
    A = Jm.T @ Jm
    return 10 * (np.linalg.norm(np.linalg.inv(A), 2) * np.sqrt(np.trace(A)) * 2.0 ** -24 * np.linalg.norm(u) + 2.0 ** -24 * np.linalg.norm(z))


@pytest.mark.parametrize("name", sorted(CFGS))
def test_recovers_the_latents_of_exact_fields(name):
    m, eng, spec, zs, xs, us, z0 = _problem(name)
    res = m.encode_snapshots(xs, us, latent0=z0)
    assert res.latent.shape == zs.shape and res.latent.dtype == np.float32
    assert res.converged.all(), (res.converged, res.iterations)
    calls = [c for c in eng.calls if c[0] == "normal_eq"]
    assert len(calls) <= 20 + 1
    assert eng.calls[0] == ("samples", COUNTS) and eng.freed == 1
    for t, n in enumerate(COUNTS):
        if n == 0:
            continue
        err, bound = np.linalg.norm(res.latent[t].astype(np.float64) - zs[t]), _recovery_bound(spec, eng.ws, zs[t], xs[t], us[t])
        print("%s snapshot %d: |z - z*| = %.3g (bound %.3g), %d iterations, mse %.3g" % (name, t, err, bound, res.iterations[t], res.loss[t]))
        assert err <= bound
        c_ref = R.normal_eq(spec, eng.ws, res.latent[t:t + 1], [xs[t]], [us[t]])[0, -1, -1]
        assert np.isclose(res.loss[t], c_ref / (n * spec.so), rtol=1e-12, atol=0)
    # the shared-mesh form is the same problem per snapshot
    xsh = xs[3]
    ush = np.stack([R.field(spec, eng.ws, zs[t], xsh).astype(np.float32) for t in range(len(COUNTS))])
    eng.calls.clear()
    sh = m.encode_snapshots(xsh, ush, latent0=z0)
    assert eng.calls[0] == ("samples", [40] * len(COUNTS))
    assert sh.converged.all() and np.array_equal(sh.latent[3], res.latent[3])
    for t in range(len(COUNTS)):
        assert np.linalg.norm(sh.latent[t].astype(np.float64) - zs[t]) <= _recovery_bound(spec, eng.ws, zs[t], xsh, ush[t])


def test_a_converged_snapshot_is_frozen_while_the_others_go_on():
    m, eng, spec, zs, xs, us, z0 = _problem("ms")
    z0[1] = zs[1]                                     # snapshot 1 starts at its solution
    res = m.encode_snapshots(xs, us, latent0=z0)
    assert res.converged.all()
    assert res.iterations[1] < res.iterations.max()
    lats = [c[1] for c in eng.calls if c[0] == "normal_eq"]
    assert len(lats) == res.iterations.max() + 1
    for t in range(len(COUNTS)):                      # once a snapshot has stopped, every later call carries its final latent
        for k in range(int(res.iterations[t]) + 1, len(lats)):
            assert np.array_equal(lats[k][t], res.latent[t]), (t, k)


def test_an_empty_snapshot_keeps_its_latent():
    m, eng, spec, zs, xs, us, z0 = _problem("ll")
    res = m.encode_snapshots(xs, us, latent0=z0)
    assert np.array_equal(res.latent[2], z0[2]) and res.loss[2] == 0.0 and res.iterations[2] == 0 and res.converged[2]
    # nothing but empty snapshots: no engine call at all
    eng.calls.clear()
    none = m.encode_snapshots([xs[2]] * 2, [us[2]] * 2, latent0=z0[:2])
    assert np.array_equal(none.latent, z0[:2]) and eng.calls == [] and none.converged.all()
    assert m.encode_snapshots([], [], latent0=z0[:0]).latent.shape == (0, spec.r)


def test_fewer_samples_than_latent_dimensions():
    """two samples of a scalar field for r = 3: A has rank <= 2.  The damping makes every step solvable; the fit reaches the samples
    (any latent on the solution set does) and the loop stops by its own criteria"""
    m, eng, spec, zs, xs, us, z0 = _problem("ms", counts=[2, 1, 40], delta=0.005)
    assert spec.r == 3 and spec.so == 1
    A = R.normal_eq(spec, eng.ws, z0, xs, us)[:, :3, :3]
    assert np.linalg.matrix_rank(A[0]) <= 2 and np.linalg.matrix_rank(A[1]) <= 1
    res = m.encode_snapshots(xs, us, latent0=z0)
    assert res.converged.all(), (res.converged, res.iterations)
    assert np.isfinite(res.latent).all()
    for t in range(2):
        scale = float(np.mean(us[t].astype(np.float64) ** 2))
        print("rank-deficient snapshot %d: mse %.3g of a field of mean square %.3g, %d iterations" % (t, res.loss[t], scale, res.iterations[t]))
        assert res.loss[t] <= 1e-12 * scale           # float32 latents: residual ~ 2^-24 |u| |du/dz| |z| per sample, squared
    assert len([c for c in eng.calls if c[0] == "normal_eq"]) <= 21


def test_exactly_one_of_latent0_and_p0_and_the_argument_shapes():
    m, eng, spec, zs, xs, us, z0 = _problem("ms")
    p0 = np.random.default_rng(6).uniform(-1, 1, size=(len(COUNTS), spec.pi)).astype(np.float32)
    with pytest.raises(ValueError):
        m.encode_snapshots(xs, us)
    with pytest.raises(ValueError):
        m.encode_snapshots(xs, us, latent0=z0, p0=p0)
    with pytest.raises(ValueError):
        m.encode_snapshots(xs, us, latent0=p0)                  # [T, pi] where [T, r] belongs
    with pytest.raises(ValueError):
        m.encode_snapshots(xs[:-1], us[:-1], latent0=z0)
    with pytest.raises(ValueError):
        m.encode_snapshots(xs, us[:-1] + [us[0]], latent0=z0)    # a snapshot's samples and coordinates differ in length
    with pytest.raises(ValueError):
        m.encode_snapshots(xs[3], np.zeros((len(COUNTS), 39, spec.so), np.float32), latent0=z0)
    with pytest.raises(ValueError):
        m.encode_snapshots(xs, us, latent0=z0, sample_weight=[np.ones(3)] * len(COUNTS))
    assert eng.calls == []
    with pytest.raises(ValueError):
        _model(CFGS["ms"], "p_to_lr")[0].encode_snapshots(xs, us, latent0=z0)
    # p0 goes through the ParameterNet once and is the same run as latent0 = its latents
    a = m.encode_snapshots(xs, us, p0=p0, max_iter=2)
    assert eng.calls[0] == ("p_to_lr", len(COUNTS))
    b = m.encode_snapshots(xs, us, latent0=eng.p_to_lr(p0), max_iter=2)
    assert np.array_equal(a.latent, b.latent) and np.array_equal(a.loss, b.loss)


@pytest.mark.parametrize("max_iter", [0, 1, 3, 20])
def test_at_most_max_iter_plus_one_device_calls(max_iter):
    m, eng, spec, zs, xs, us, z0 = _problem("nif")
    res = m.encode_snapshots(xs, us, latent0=z0, max_iter=max_iter)
    calls = len([c for c in eng.calls if c[0] == "normal_eq"])
    assert 1 <= calls <= max_iter + 1
    assert res.iterations.max() <= max_iter
    if max_iter == 0:
        assert np.array_equal(res.latent, z0) and not res.converged[0]
        c0 = R.normal_eq(spec, eng.ws, z0, xs, us)[:, -1, -1]
        assert np.allclose(res.loss, c0 / np.maximum(np.array(COUNTS) * spec.so, 1), rtol=1e-12, atol=0)


def test_weights_enter_the_normal_equations_and_zero_weight_removes_a_sample():
    m, eng, spec, zs, xs, us, z0 = _problem("ms")
    us_bad = [u.copy() for u in us]
    us_bad[3][5] += 3.0                                # one corrupted sample ...
    w = [np.ones(n, np.float32) for n in COUNTS]
    w[3][5] = 0.0                                      # ... that weighs nothing
    res = m.encode_snapshots(xs, us_bad, latent0=z0, sample_weight=w)
    assert res.converged.all()
    assert np.linalg.norm(res.latent[3].astype(np.float64) - zs[3]) <= _recovery_bound(spec, eng.ws, zs[3], np.delete(xs[3], 5, 0), np.delete(us[3], 5, 0))
