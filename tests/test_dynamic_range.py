"""The conditions under which tests/test_gpu_dynamic_range.py means something, checked on the float64 oracle alone (no GPU):
every stress does what its name says, the reference is stable under one float32 ulp of its weights at every (case, axis) pair, the
oracle itself is exactly equivariant under a power of two on the sample weights, and no entry of [grad | loss] is small enough to be
excused from the bit equality.  profiles/dynamic_range.md holds the figures printed here."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import range_cases as R
from tests.test_gpu_parity import _one_ulp_weights

_inputs = {}


def _host(case):
    if case not in _inputs:
        _inputs[case] = R.host_inputs(case)
    return _inputs[case]


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_case_sits_in_the_kernel_the_table_names(case):
    spec = R.spec_of(case)
    nh = spec.n_hidden_mats
    planes = R.hidden_planes(spec, _host(case)[1])
    assert len(planes) == nh * (1 if spec.kind == O.KIND_LL else spec.r + 1)
    assert all(v.size == spec.n * spec.n for _, _, v in planes)
    assert R.CASES[case][1] % 16 != 0 and R.CASES[case][1] > 128       # a ragged last tile, more than one 128-point block


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_each_stress_does_what_its_name_says(case):
    spec, ws, x, y, sw = _host(case)
    e0 = R.plane_max_exponents(spec, ws)
    is_base = lambda k: R._is_base(spec, k)
    # base_small: every base plane's maximum 2^10 lower, the modulation planes untouched
    e = R.plane_max_exponents(spec, R.base_small(spec, ws))
    assert all(e0[jk] - e[jk] == (10 if is_base(jk[1]) else 0) for jk in e0), (e0, e)
    if spec.kind != O.KIND_LL:
        e = R.plane_max_exponents(spec, R.mod_small(spec, ws))
        assert all(e0[jk] - e[jk] == (0 if is_base(jk[1]) else 12) for jk in e0), (e0, e)
        z = R.mod_small(spec, ws, factor=0.0)
        assert all((not v.any()) == (not is_base(k)) for _, k, v in R.hidden_planes(spec, z))
    # outlier6: one entry per plane moved, by 2^6, and it now leads the plane by at least 2^3
    wo = R.outlier6(spec, ws)
    for (j, k, v0), (_, _, v1) in zip(R.hidden_planes(spec, ws), R.hidden_planes(spec, wo)):
        moved = np.flatnonzero(v0 != v1)
        assert moved.size == 1 and v1[moved[0]] == 64.0 * v0[moved[0]], (case, j, k)
    gap = min(np.sort(np.abs(v))[-1] / np.sort(np.abs(v))[-2] for _, _, v in R.hidden_planes(spec, wo))
    # spread: an exponent span of at least 16 in every plane
    span = min(R.plane_exponent_span(v) for _, _, v in R.hidden_planes(spec, R.spread(spec, ws)))
    s = R.sw_wide(x.shape[0])
    es = np.log2(s.astype(np.float64))
    ym = R.y_mixed(y)
    ratio = np.abs(ym.astype(np.float64)).max(axis=1) / np.abs(y.astype(np.float64)).max(axis=1)
    print("%s: outlier leads its plane by >= %.1f, spread span >= %d, sw exponents %d..%d, y row factors %.1e..%.1e"
          % (case, gap, span, es.min(), es.max(), ratio.min(), ratio.max()))
    assert span >= 16
    assert gap >= 32.0, gap       # an outlier that does not lead its plane stresses nothing
    assert np.array_equal(es, np.round(es)) and es.min() <= -18 and es.max() >= 18
    assert ratio.min() < 2e-6 and ratio.max() > 5e3
    assert R.bg_2p30(x.shape[0]) == x.shape[0] << 22 and 2 ** 29 <= R.bg_2p30(x.shape[0]) < 2 ** 31
    # every stressed weight is still a float32 (exact powers of two: nothing was rounded), the untouched tensors are bit-identical
    for ax in R.WEIGHT_AXES:
        if ax in R.axes_of(case):
            w2 = R.stressed(ax, spec, ws, x, y, sw)[0]
            names = [nm for nm, _ in spec.param_shapes()]
            touched = {"pnet_last_w", "pnet_last_b"} if spec.kind != O.KIND_LL else {nm for nm in names if nm.startswith("snet_h")}
            assert all(nm in touched or np.array_equal(a, b) for nm, a, b in zip(names, ws, w2)), (case, ax)


@pytest.mark.parametrize("case,axis", R.pairs())
def test_reference_is_stable_under_one_ulp(case, axis):
    """the device of test_full_size_shard_sum_other_configs: where the float64 oracle itself moves by s under one float32 ulp of its
    weights, no float32 kernel can be held closer than s to it.  At most 2e-5 per tensor (0.4 of the 5e-5 bar), 1e-5 forward."""
    spec, ws, x, y, sw = _host(case)
    ws2, x2, y2, sw2, bg = R.stressed(axis, spec, ws, x, y, sw)
    s, nm, fwd = R.sensitivity(spec, ws2, x2, y2, sw2, bg, _one_ulp_weights)
    print("condition %s / %s: worst tensor %.2e (%s), forward %.2e" % (case, axis, s, nm, fwd))
    assert s <= R.SENS_BAR, (case, axis, nm, s)
    assert fwd <= R.SENS_FWD_BAR, (case, axis, fwd)


@pytest.mark.parametrize("case", R.END_CASES)
def test_reference_is_stable_at_the_ends(case):
    """the same condition for the inputs of test_finite_and_right_at_the_ends, and the size of the half pairs' budget on the one tensor
    that gets it there: a fraction of the tensor everywhere but where the targets make it cancel"""
    spec, ws, x, y, sw = _host(case)
    ybig = (y * np.float32(1e6)).astype(np.float32)
    wz = R.mod_small(spec, ws, factor=0.0)
    for what, w_, y_ in (("y * 1e6", ws, ybig), ("zero planes", wz, y)):
        s, nm, fwd = R.sensitivity(spec, w_, x, y_, sw, x.shape[0], _one_ulp_weights)
        print("condition %s / %s: worst tensor %.2e (%s), forward %.2e" % (case, what, s, nm, fwd))
        assert s <= R.SENS_BAR and fwd <= R.SENS_FWD_BAR, (case, what, nm, s, fwd)
    names = [nm for nm, _ in spec.param_shapes()]
    for what, y_ in (("y", y), ("y * 1e6", ybig)):
        g = O.loss_and_grad(spec, ws, x.astype(np.float64), y_.astype(np.float64), sw.astype(np.float64))[1]
        gn, gb = np.linalg.norm(O.flatten(g)), np.linalg.norm(g[names.index("pnet_bottleneck_b")])
        b = np.linalg.norm(R.latent_adjoint_budget(spec, ws, x, y_, sw))
        print("budget %s / %s: pnet_bottleneck_b %.2e |ref|, standing bar %.2e |ref|, budget of the half pairs %.2e |ref|"
              % (case, what, gb / gn, (5e-5 * gb + 2.5e-7 * gn) / gn, b / gn))
        assert b <= 5e-5 * gb + 2.5e-7 * gn      # the budget at most doubles that tensor's standing bar: the bar stays a bar


@pytest.mark.parametrize("case", sorted(R.CASES))
@pytest.mark.parametrize("loss", ["mse", "huber"])
def test_oracle_is_equivariant_and_nothing_is_exempt(case, loss):
    """float64 has the room: sw * 2^12 gives [grad | loss] * 2^12 bit for bit.  And no entry of the oracle's [grad | loss], times any
    2^k the GPU test uses, comes near float32's subnormals (2^-100 leaves 2^26 above them) -- so the GPU test excuses nothing.
    The Sobolev step of the two cases that have one, likewise."""
    spec, ws, x, y, sw = _host(case)
    x64, y64, s64 = x.astype(np.float64), y.astype(np.float64), sw.astype(np.float64)
    l0, g0 = O.loss_and_grad(spec, ws, x64, y64, s64, loss=loss)
    l1, g1 = O.loss_and_grad(spec, ws, x64, y64, s64 * 4096.0, loss=loss)
    r0, r1 = np.append(O.flatten(g0), l0), np.append(O.flatten(g1), l1)
    assert np.array_equal(r0 * 4096.0, r1), int((r0 * 4096.0 != r1).sum())
    refs = [("plain", r0), ("plain, B_global << 24", r0 * 2.0 ** -24)]
    if case in R.SOBOLEV[0] and loss == "mse":
        xi = [spec.pi, spec.pi + 1]
        gt = R.sobolev_targets(spec, x.shape[0]).astype(np.float64)
        ls, gs = O.sobolev_loss_and_grad(spec, ws, x64, y64, gt, xi, R.WJ, s64)[:2]
        ls1, gs1 = O.sobolev_loss_and_grad(spec, ws, x64, y64, gt, xi, R.WJ, s64 * 4096.0)[:2]
        rs0, rs1 = np.append(O.flatten(gs), ls), np.append(O.flatten(gs1), ls1)
        assert np.array_equal(rs0 * 4096.0, rs1)
        refs += [("sobolev", rs0), ("sobolev, B_global << 24", rs0 * 2.0 ** -24)]
    for what, r in refs:
        nz = np.abs(r[r != 0])
        worst = [R.exempt(r, k).size for k in R.KS]
        print("%s / %s / %s: smallest non-zero |entry| 2^%.1f, exempt per k %s" % (case, loss, what, np.log2(nz.min()), worst))
        assert sum(worst) == 0, (case, what, worst)
    if case in R.END_CASES and loss == "mse":     # the ends of the GPU file: sw = 2^-60 everywhere against the unweighted step
        lu, gu = O.loss_and_grad(spec, ws, x64, y64)
        ru = np.append(O.flatten(gu), lu)
        nz = np.abs(ru[ru != 0])
        print("%s / unweighted: smallest non-zero |entry| 2^%.1f, exempt at 2^-60: %d" % (case, np.log2(nz.min()), R.exempt(ru, -60).size))
        assert R.exempt(ru, -60).size == 0
