"""Model.select_sensors without a GPU: the float64 reference of the greedy pivoted QR (tests/sensors_ref.py) picks the pivots of
SciPy's LAPACK pivoted QR on every case of the GPU tests, the conditions under which those cases compare pivots hold on the oracle's
phi, the extension header include/nif_hip_sensors.h, its ctypes table and struct mirror and the library's exports are equal, both
entries pass the door of the C-ABI, and the defaults, the rank cut, the (point, component) split and the refusals of
Model.select_sensors are what they say on an engine double fed by the reference.  The device path is tests/test_gpu_select_sensors.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import sensors_ref as R
from tests.cfgs import ALL_SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nif_hip_sensors.h")
ENTRIES = ["nif_select_sensors", "nif_select_sensors_dev"]

_refs = {}


def _ref(name):
    """(case, phi, mask, reference result) on the oracle's phi, computed once"""
    if name not in _refs:
        case = R.DEFICIENT if name == "deficient" else R.CASES[name]
        phi = R.oracle_phi(case)
        mask = R.mesh(case)[1]
        _refs[name] = (case, phi, mask, R.select(phi, case.K, mask))
    return _refs[name]


ALL_CASES = sorted(R.CASES) + ["deficient"]


# ---- the reference -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_reference_pivots_are_scipys(name):
    """scipy.linalg.qr(Phi^T, pivoting=True): LAPACK's geqp3 down-dates the column norms instead of recomputing them, so the two can
    differ only at a near-tie -- which the cases exclude -- or past the rank"""
    sl = pytest.importorskip("scipy.linalg")
    case, phi, mask, ref = _ref(name)
    rows = phi.reshape(-1, phi.shape[2])
    idx = np.arange(rows.shape[0]) if mask is None else np.flatnonzero(np.repeat(mask, phi.shape[1]))
    _, _, perm = sl.qr(rows[idx].T, mode="economic", pivoting=True)
    upto = R.DEFICIENT_RANK if name == "deficient" else min(case.K, idx.size)
    assert idx[perm[:upto]].tolist() == ref.pivots[:upto].tolist()


@pytest.mark.parametrize("name", ALL_CASES)
def test_the_conditions_of_the_gpu_cases_hold_on_the_oracles_phi(name):
    case, phi, mask, ref = _ref(name)
    if name == "deficient":
        ok, gap, rel = R.conditions_hold(ref, R.DEFICIENT_RANK)
        assert ref.rel[R.DEFICIENT_RANK - 1] >= R.REL_MIN and ref.rel[R.DEFICIENT_RANK] < R.RANK_DROP
    else:
        assert (ref.pivots >= 0).all()
        ok, gap, rel = R.conditions_hold(ref)
    print("%s: min gap %.2e, min d_k / d_0 %.3f" % (name, gap, rel))
    assert ok, (gap, rel)


def test_reference_on_a_matrix_with_known_pivots():
    """rows 3 e0, 2 e1, (1, 1, 0), e2 twice: norms, projections, the lowest row at a tie, zero rows never chosen"""
    phi = np.array([[0, 0, 0], [3, 0, 0], [1, 1, 0], [0, 2, 0], [0, 0, 1], [0, 0, 1]], dtype=np.float64)[:, None, :]
    ref = R.select(phi, 3)
    assert ref.pivots.tolist() == [1, 3, 4] and np.allclose(ref.diag, [3, 2, 1])
    assert np.allclose(ref.gap, [1 - 4 / 9.0, 1 - 1 / 4.0, 0.0])
    masked = R.select(phi, 3, mask=[1, 0, 1, 1, 0, 0])
    assert masked.pivots.tolist() == [3, 2, -1] and np.allclose(masked.diag, [2, 1, 0])
    two = R.select(phi.reshape(3, 2, 3), 3, mask=[0, 1, 1])      # so = 2: the mask is per point
    assert two.pivots.tolist() == [3, 2, 4]


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_sensors_header_exports_and_ctypes_table_are_equal():
    from nif_amd import _lib
    names = sorted(set(re.findall(r"\b(nif_[a-z0-9_]+)\s*\(", _header())))
    assert names == ENTRIES == sorted(_lib.SENSORS_SIGNATURES)
    others = [_lib.SIGNATURES, _lib.SNAPSHOT_SIGNATURES, _lib.ENCODE_SIGNATURES, _lib.SNAPDERIV_SIGNATURES, _lib.SNAPPARAM_SIGNATURES,
              _lib.SNAPPARAM2_SIGNATURES, _lib.SNAPFIT_SIGNATURES]
    assert not any(set(names) & set(t) for t in others)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert hasattr(lib, nm), "the header declares %s but the library does not export it" % nm
    bound = _lib.load()
    for nm in names:
        assert getattr(bound, nm).argtypes == _lib.SENSORS_SIGNATURES[nm][1] == [ctypes.POINTER(_lib.nif_sensors_args)]
        assert getattr(bound, nm).restype is ctypes.c_int


def test_struct_mirror_has_the_headers_fields_size_and_offsets():
    """the header's struct laid out by the x86-64 / LP64 rules (natural alignment: int32 4, int64 and pointers 8) against ctypes'"""
    from nif_amd import _lib
    txt = _header()
    body = re.search(r"typedef\s+struct\s+nif_sensors_args\s*\{(.*?)\}\s*nif_sensors_args\s*;", txt, flags=re.S).group(1)
    fields, off = [], 0
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        m = re.match(r"^(.*?)(\w+)\s*(?:\[(\d+)\])?$", decl)
        ctype, name, count = m.group(1).strip(), m.group(2), int(m.group(3) or 1)
        size = 8 if ctype.endswith("*") else {"int32_t": 4, "int64_t": 8}[ctype]
        off = (off + size - 1) // size * size
        fields.append((name, off, size * count))
        off += size * count
    total = (off + 7) // 8 * 8
    mirror = _lib.nif_sensors_args
    assert [f[0] for f in mirror._fields_] == [f[0] for f in fields]
    assert [f[0] for f in fields] == ["abi_version", "reserved0", "ctx", "x", "M", "mask", "K", "pivots_out", "diag_out", "reserved"]
    for name, o, sz in fields:
        assert (getattr(mirror, name).offset, getattr(mirror, name).size) == (o, sz), name
    assert ctypes.sizeof(mirror) == total
    assert int(re.search(r"#define\s+NIF_SENSORS_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.NIF_SENSORS_ABI_VERSION == 1


def test_both_entries_pass_the_guard_in_their_own_body():
    """tests/test_entry_guard.py's rule for the entries whose context travels inside the struct: NIF_ENTER(<args>->ctx, NIF_FLUSH_TAIL)"""
    from tests.test_entry_guard import _exports
    exports = _exports()
    for nm in ENTRIES:
        assert nm in exports, "%s is no extern \"C\" definition" % nm
        first, body = exports[nm]
        assert re.match(r"^const nif_sensors_args\s*\*\s*(\w+)$", first), first
        arg = first.split("*")[-1].strip()
        assert re.search(r"\bNIF_ENTER\s*\(\s*%s\s*->\s*ctx\s*,\s*NIF_FLUSH_TAIL\s*\)" % arg, body), nm


def test_the_kernel_file_is_built_and_uses_no_atomics():
    import __graft_entry__ as G
    assert "k_sensors.hip" in G.SOURCES
    src = open(os.path.join(G.CSRC, "k_sensors.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\batomic\w*\s*\(", code)


def test_the_older_headers_and_the_core_table_do_not_know_the_entries():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "nif_hip_sensors.h":
            assert "nif_select_sensors" not in open(os.path.join(ROOT, "include", h)).read(), h


# ---- Model.select_sensors on an engine double ----------------------------------------------------------------------------------------
class SensorEngine(object):
    """Engine.select_sensors by the reference on the oracle's phi: (pivots [K] int64, diag [K] float32)"""

    def __init__(self, spec, ws):
        self.o, self.ws, self.calls = spec, ws, []

    def select_sensors(self, x, n_sensors, mask=None):
        self.calls.append((x.shape, x.dtype, int(n_sensors), None if mask is None else (mask.dtype, mask.copy())))
        ref = R.select(O.snet_phi(self.o, self.ws, x.astype(np.float64)), int(n_sensors), mask)
        return ref.pivots, ref.diag.astype(np.float32)


def _double(case, role="full"):
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    spec, ws = R.weights(case)
    eng = SensorEngine(spec, [w.astype(np.float64) for w in ws])
    model = Model(types.SimpleNamespace(_spec=Spec(*case.net), _engine=eng), role)
    return model, eng, spec


def test_defaults_and_the_split_of_a_row_index():
    case, phi, mask, ref = _ref("r10_so3_m33")
    model, eng, spec = _double(case)
    x = R.mesh(case)[0]
    res = model.select_sensors(x)
    assert eng.calls == [((33, 2), np.float32, 10, None)]      # n_sensors defaults to r
    assert type(res).__name__ == "SensorResult" and res._fields == ("point", "component", "x", "diag", "rank")
    assert res.rank == 10 and res.point.dtype == np.int64 and res.component.dtype == np.int64 and res.diag.dtype == np.float32
    assert (res.point * 3 + res.component).tolist() == ref.pivots.tolist()
    assert set(res.component.tolist()) <= {0, 1, 2} and len(set(res.component.tolist())) > 1
    assert np.array_equal(res.x, x[res.point]) and np.allclose(res.diag, ref.diag, rtol=1e-6)
    few = model.select_sensors(x, n_sensors=4)
    assert few.rank == 4 and (few.point * 3 + few.component).tolist() == ref.pivots[:4].tolist()
    # a column vector of coordinates for si = 1
    c1 = R.CASES["r1_so1_m1"]
    m1 = _double(c1)[0]
    assert m1.select_sensors(R.mesh(c1)[0][:, 0]).point.tolist() == [0]


def test_the_rtol_cut_and_rank():
    case, phi, mask, ref = _ref("deficient")
    model, eng, spec = _double(case)
    x = R.mesh(case)[0]
    res = model.select_sensors(x)      # default rtol: r float32 epsilons
    assert res.rank == R.DEFICIENT_RANK == len(res.point) == len(res.component) == len(res.diag) == res.x.shape[0]
    assert res.point.tolist() == ref.pivots[:res.rank].tolist()
    found = int((ref.pivots >= 0).sum())
    assert found > R.DEFICIENT_RANK and model.select_sensors(x, rtol=0).rank == found      # every step that found a row: rounding included
    cut = int(np.argmax(ref.rel <= 0.3))
    assert 0 < cut < R.DEFICIENT_RANK and model.select_sensors(x, rtol=0.3).rank == cut
    with pytest.raises(ValueError, match="rtol"):
        model.select_sensors(x, rtol=-1.0)


def test_too_few_candidates_and_an_empty_mask():
    case = R.CASES["r10_so3_m33"]
    model, eng, spec = _double(case)
    x = R.mesh(case)[0]
    mask = np.zeros(33, dtype=bool)
    mask[[4, 20]] = True
    res = model.select_sensors(x, mask=mask)      # 2 points x 3 components = 6 candidates for 10 steps
    assert res.rank == 6 and sorted(set(res.point.tolist())) == [4, 20]
    assert eng.calls[-1][3][0] == np.bool_ and np.array_equal(eng.calls[-1][3][1], mask)
    assert model.select_sensors(x, mask=mask.astype(np.float32)).rank == 6      # nonzero = admitted
    empty = model.select_sensors(x, mask=np.zeros(33, dtype=bool))
    assert empty.rank == 0 and empty.point.shape == (0,) and empty.x.shape == (0, 2) and empty.diag.shape == (0,)


def test_argument_errors():
    case = R.CASES["r10_so3_m33"]
    model, eng, spec = _double(case)
    x = R.mesh(case)[0]
    for bad in (np.ones(32, dtype=bool), np.ones((33, 1), dtype=bool), np.ones((33, 3), dtype=bool)):
        with pytest.raises(ValueError, match="mask must have shape"):
            model.select_sensors(x, mask=bad)
    for k in (0, -1, 11):
        with pytest.raises(ValueError, match="n_sensors = %d outside 1 .. latent_dim = 10" % k):
            model.select_sensors(x, n_sensors=k)
    for bad in (x[:, :1], x[:0], np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError, match="x must have shape"):
            model.select_sensors(bad)
    assert not eng.calls


def test_the_other_classes_and_the_views_refuse():
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    for name in ("nif_swish", "ms_plain"):
        kind, cs, cp = ALL_SMALL[name]
        model = Model(types.SimpleNamespace(_spec=Spec(kind, cs, cp), _engine=None), "full")
        with pytest.raises(NotImplementedError, match="depends on the latent"):
            model.select_sensors(np.zeros((4, 1), np.float32))
    case = R.CASES["r10_so3_m33"]
    for role in ("p_to_lr", "lr_to_w", "x_to_u_given_w", "x_to_phi"):
        view = _double(case, role)[0]
        with pytest.raises(ValueError, match="full model only"):
            view.select_sensors(R.mesh(case)[0])


def test_the_sobolev_model_forwards():
    from nif_amd.model import SobolevModel
    case, phi, mask, ref = _ref("r10_so3_m33")
    model, eng, spec = _double(case)
    sm = SobolevModel.__new__(SobolevModel)
    sm._owner, sm._role = model._owner, "full"
    assert (lambda s: s.point * 3 + s.component)(sm.select_sensors(R.mesh(case)[0])).tolist() == ref.pivots.tolist()
