"""Sensor placement on the device (include/nif_hip_sensors.h, csrc/k_sensors.hip, Model.select_sensors) against the float64 reference
of tests/sensors_ref.py run ON THE DEVICE'S OWN model_x_to_phi(x): the forward pass's error is not in the comparison.  Pivots are
compared exactly, which is meaningful only where the two best scores of a step are apart by far more than float32 rounding: every case
first re-asserts gap >= 1e-3 and d_k / d_0 >= 0.05 on that phi (tests/test_select_sensors.py asserts them on the oracle's) and fails,
not skips, where they do not hold.

d against the reference's: D_BAR is the largest relative error measured on the MI355X over the cases of this file (printed by the
tests) x 8 for run-to-run headroom.  It has to stay far below 5e-4, the smallest admitted gap (1e-3 in squared norms) in
norms; it may not exceed 1e-5."""
import ctypes as C

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import sensors_ref as R
from tests.cfgs import ALL_SMALL

pytestmark = pytest.mark.gpu

D_MEASURED = 2.5e-7      # r64_so1_m257, 64 steps; every other case 1.5e-7 or less
D_BAR = 8 * D_MEASURED   # 2e-6
assert D_BAR <= 1e-5

_built, _runs = {}, {}


def _fresh(case):
    import nif_amd
    kind, cs, cp = case.net
    spec, ws = R.weights(case)
    m = getattr(nif_amd, kind)(cs, cp, mixed_policy=case.policy)
    model = m.build()
    model.set_weights(ws)
    return m, model, spec


def _net(name):
    """(m, model, spec) of a case, built once: nothing here changes weights"""
    if name not in _built:
        _built[name] = _fresh(R.DEFICIENT if name == "deficient" else R.CASES[name])
    return _built[name]


def _run(name):
    """(case, x, mask, reference on the device's phi, device pivots, device d) of a case, computed once"""
    if name not in _runs:
        case = R.DEFICIENT if name == "deficient" else R.CASES[name]
        m, model, spec = _net(name)
        x, mask = R.mesh(case)
        phi = m._engine.x_to_phi(x)
        assert phi.shape == (case.M, spec.so, spec.r) and np.isfinite(phi).all()
        ref = R.select(phi, case.K, mask)
        piv, d = m._engine.select_sensors(x, case.K, mask)
        assert piv.dtype == np.int64 and d.dtype == np.float32 and piv.shape == d.shape == (case.K,)
        _runs[name] = (case, x, mask, ref, piv, d)
    return _runs[name]


def _d_err(d, ref, n):
    return float(np.max(np.abs(d[:n].astype(np.float64) - ref.diag[:n]) / ref.diag[:n])) if n else 0.0


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_pivots_equal_the_reference_and_d_is_within_the_bar(name):
    case, x, mask, ref, piv, d = _run(name)
    assert (ref.pivots >= 0).all()
    ok, gap, rel = R.conditions_hold(ref)
    err = _d_err(d, ref, case.K)
    print("%s: on the device's phi min gap %.2e, min d_k / d_0 %.3f; d rel err %.2e (bar %.1e)" % (name, gap, rel, err, D_BAR))
    assert ok, "the conditions of the case do not hold on the device's phi: gap %.2e, d_k / d_0 %.3f" % (gap, rel)
    assert piv.tolist() == ref.pivots.tolist()
    assert err <= D_BAR, err
    if mask is not None:
        assert mask[piv // O.Spec(*case.net).so].all()


def test_a_masked_point_is_never_chosen_and_an_empty_mask_finds_nothing():
    name = "r10_so1_m257"
    case, x, mask, ref, piv, d = _run(name)
    m, model, spec = _net(name)
    e = m._engine
    off = np.ones(case.M, dtype=bool)
    off[piv[0] // spec.so] = False
    off[piv[3] // spec.so] = False
    p2, d2 = e.select_sensors(x, case.K, off)
    r2 = R.select(e.x_to_phi(x), case.K, off)
    assert R.conditions_hold(r2)[0], R.conditions_hold(r2)
    assert p2.tolist() == r2.pivots.tolist() and p2.tolist() != piv.tolist() and p2[0] != piv[0]
    assert off[p2 // spec.so].all() and _d_err(d2, r2, case.K) <= D_BAR
    # nonzero = admitted, whatever the dtype
    assert e.select_sensors(x, case.K, off.astype(np.uint8) * 200)[0].tolist() == p2.tolist()
    p0, d0 = e.select_sensors(x, case.K, np.zeros(case.M, dtype=bool))
    assert p0.tolist() == [-1] * case.K and d0.tolist() == [0.0] * case.K
    res = model.select_sensors(x, mask=np.zeros(case.M, dtype=bool))
    assert res.rank == 0 and res.point.shape == (0,)


def test_fewer_candidates_than_steps():
    name = "r10_so3_m33"
    case, x, mask, ref, piv, d = _run(name)
    m, model, spec = _net(name)
    e = m._engine
    two = np.zeros(case.M, dtype=bool)
    two[[4, 20]] = True
    p2, d2 = e.select_sensors(x, 10, two)      # M so = 6 candidates for 10 steps
    r2 = R.select(e.x_to_phi(x), 10, two)
    assert (r2.pivots >= 0).sum() == 6
    assert (p2[:6] >= 0).all() and sorted(set((p2[:6] // 3).tolist())) == [4, 20] and len(set(p2[:6].tolist())) == 6
    assert p2[6:].tolist() == [-1] * 4 and d2[6:].tolist() == [0.0] * 4 and (d2[:6] > 0).all()
    n = int(np.argmax(~((r2.gap >= R.GAP_MIN) & (r2.rel >= R.REL_MIN))))      # compared while the conditions hold
    assert n >= 3 and p2[:n].tolist() == r2.pivots[:n].tolist()
    p1, d1 = e.select_sensors(x[:1], 10)      # one point: so = 3 rows
    assert sorted(p1[:3].tolist()) == [0, 1, 2] and p1[3:].tolist() == [-1] * 7 and d1[3:].tolist() == [0.0] * 7
    assert model.select_sensors(x[:1]).rank == 3 and model.select_sensors(x, mask=two).rank <= 6


def test_a_rank_deficient_basis():
    """r = 10 on a 6-unit ShapeNet: rank 7.  Pivots are compared up to the rank; at the rank d falls to rounding"""
    case, x, mask, ref, piv, d = _run("deficient")
    m, model, spec = _net("deficient")
    rank = R.DEFICIENT_RANK
    ok, gap, rel = R.conditions_hold(ref, rank)
    assert ok, (gap, rel)
    assert int(np.argmax(~(ref.rel >= R.RANK_DROP))) == rank      # the reference's rank on the device's phi
    print("deficient: device d_k / d_0 = %s; reference %s" % (np.array2string(d / d[0], precision=2), np.array2string(ref.rel, precision=2)))
    assert piv[:rank].tolist() == ref.pivots[:rank].tolist() and _d_err(d, ref, rank) <= D_BAR
    assert (d[rank:] < R.RANK_DROP * d[0]).all()
    res = model.select_sensors(x)
    assert res.rank == rank and (res.point * spec.so + res.component).tolist() == piv[:rank].tolist()
    assert np.array_equal(res.x, x[res.point]) and np.array_equal(res.diag, d[:rank])


@pytest.mark.parametrize("name", ["r10_so1_m257", "r16_so4_m257", "r64_so1_m257", "w256_r10_so3_m129"])
def test_two_calls_are_bit_equal_and_a_permuted_mesh_permutes_the_pivots(name):
    case, x, mask, ref, piv, d = _run(name)
    m, model, spec = _net(name)
    e = m._engine
    p2, d2 = e.select_sensors(x, case.K, mask)
    assert np.array_equal(p2, piv) and d2.tobytes() == d.tobytes()
    perm = np.random.default_rng(5).permutation(case.M)
    xp = np.ascontiguousarray(x[perm])
    # the premise: phi of a point does not depend on its place in the mesh
    assert np.array_equal(e.x_to_phi(xp), e.x_to_phi(x)[perm]), "phi of a point depends on its position in the mesh"
    pp, dp = e.select_sensors(xp, case.K)
    assert (perm[pp // spec.so] * spec.so + pp % spec.so).tolist() == piv.tolist()
    assert dp.tobytes() == d.tobytes()


def test_dev_and_host_entries_agree_and_the_call_changes_nothing_else():
    name = "r10_so3_m500_k4"
    case, x, mask, ref, piv, d = _run(name)
    m, model, spec = _net(name)
    e = m._engine
    rng = np.random.default_rng(3)
    xin = rng.uniform(-1, 1, size=(70, spec.pi + spec.si)).astype(np.float32)
    y = rng.uniform(-1, 1, size=(70, spec.so)).astype(np.float32)
    loss0, g0 = e.loss_and_grad(xin, y)
    theta0, u0 = e.get_flat(), model.predict(xin)
    keep = rng.uniform(size=case.M) < 0.7
    ph, dh = e.select_sensors(x, case.K, keep)
    d_x, d_m = e.alloc(x.size), e.alloc((case.M + 3) // 4)
    d_p, d_d = e.alloc(2 * case.K), e.alloc(case.K)
    try:
        d_x.upload(x)
        mb = np.zeros((case.M + 3) // 4 * 4, dtype=np.uint8)
        mb[:case.M] = keep
        d_m.upload(mb.view(np.float32))
        for dm, want in ((None, (piv, d)), (d_m.at(0), (ph, dh))):
            e.select_sensors_dev(d_x.at(0), case.M, dm, case.K, d_p.at(0), d_d.at(0))
            e.sync()
            assert np.array_equal(d_p.download().view(np.int64), want[0]) and d_d.download().tobytes() == want[1].tobytes()
    finally:
        for b in (d_x, d_m, d_p, d_d):
            b.free()
    assert keep[ph // spec.so].all()
    loss1, g1 = e.grad_read()
    assert loss1 == loss0 and np.array_equal(g1, g0)
    assert np.array_equal(e.get_flat(), theta0) and np.array_equal(model.predict(xin), u0)


def test_refusals():
    import nif_amd
    from nif_amd import _lib
    # the hypernetwork classes
    for cfg in ("nif_swish", "ms_plain"):
        kind, cs, cp = ALL_SMALL[cfg]
        m = getattr(nif_amd, kind)(cs, cp)
        model = m.build()
        x = np.zeros((5, cs["input_dim"]), dtype=np.float32)
        with pytest.raises(_lib.NifError, match="not built for the hypernetwork classes.*depends on the latent"):
            m._engine.select_sensors(x, 1)
        with pytest.raises(NotImplementedError, match="depends on the latent"):
            model.select_sensors(x)
    name = "r10_so3_m33"
    case, x, mask, ref, piv, d = _run(name)
    m, model, spec = _net(name)
    e = m._engine
    for k in (0, -3, 11):
        with pytest.raises(_lib.NifError, match=r"K = %d outside 1 \.\. latent_dim = 10.*oversampling" % k):
            e.select_sensors(x, k)
    with pytest.raises(_lib.NifError, match="M = 0 < 1"):
        e.select_sensors(x[:0], 3)
    with pytest.raises(ValueError, match="n_sensors = 11"):
        model.select_sensors(x, n_sensors=11)
    for view in (m.model_p_to_lr(), m.model_x_to_phi()):
        with pytest.raises(ValueError, match="full model only"):
            view.select_sensors(x)
    # the struct's version and reserved fields, a capture
    po, do = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.float32)

    def args():
        return e._sensors_args(_lib.ptr(x), case.M, None, 3, _lib.ptr(po), _lib.ptr(do))
    for change, msg in ((lambda a: setattr(a, "abi_version", 2), "abi_version 2 != 1"), (lambda a: setattr(a, "reserved0", 1), "reserved fields"),
                        (lambda a: a.reserved.__setitem__(3, 7), "reserved fields"), (lambda a: setattr(a, "x", None), "bad argument"),
                        (lambda a: setattr(a, "diag_out", None), "bad argument")):
        a = args(); change(a)
        for fn in (e.lib.nif_select_sensors_dev, e.lib.nif_select_sensors):
            assert fn(C.byref(a)) == -1
            assert msg in e.lib.nif_last_error().decode()
    a = args()
    e.graph_begin()
    try:
        assert e.lib.nif_select_sensors_dev(C.byref(a)) == -4
        assert "not capturable" in e.lib.nif_last_error().decode()
        assert e.lib.nif_select_sensors(C.byref(a)) == -4
        with pytest.raises(_lib.NifError, match="not capturable"):
            e.select_sensors(x, 3)
    finally:
        e.graph_end()
    assert e.lib.nif_select_sensors(C.byref(a)) == 0
    assert po.tolist() == piv[:3].tolist() and do.tobytes() == d[:3].tobytes()


def test_workflow_sensors_then_encode_then_the_whole_field():
    """fields u = phi . a + bias of random a; r sensors; encode_snapshots from the readings at the sensors' points; the decoded field"""
    name = "r16_so4_m257"
    case, x, mask, ref, piv, d = _run(name)
    m, model, spec = _net(name)
    T = 6
    a = np.random.default_rng(11).normal(size=(T, spec.r)).astype(np.float32)
    u = model.predict_snapshots(x, latent=a)
    assert u.shape == (T, case.M, spec.so)
    res = model.select_sensors(x)
    assert res.rank == spec.r
    pts = np.unique(res.point)
    phi_s = m._engine.x_to_phi(x[pts]).astype(np.float64).reshape(-1, spec.r)
    cond = float(np.linalg.cond(phi_s))
    print("workflow: %d sensors at %d points, cond(Phi_s) = %.1f" % (res.rank, pts.size, cond))
    assert cond <= 1e3, cond
    enc = model.encode_snapshots(x[pts], u[:, pts, :], latent0=np.zeros((T, spec.r), dtype=np.float32), max_iter=20, tol=1e-6)
    back = model.predict_snapshots(x, latent=enc.latent)
    err = np.linalg.norm((back - u).reshape(T, -1), axis=1) / np.linalg.norm(u.reshape(T, -1), axis=1)
    print("workflow: rel-L2 of the decoded fields %s" % np.array2string(err, precision=2))
    assert err.max() <= 1e-3, err
