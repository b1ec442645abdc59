"""The derivative layers kernel by kernel: JacobianLayer, HessianLayer and the two-output model's predict() at the launch forms and
branches that nif_jacobian / hessian_core (nif_amd/csrc/nif_api.hip), launch_jac_impl (k_jac.hip), launch_mlp_jac (k_mlpjac.hip) and
the gather / contraction kernels of k_misc.hip choose.  Cases: tests/deriv_cases.py.

  launch form / branch                                                    reached by
  ----------------------------------------------------------------------  ---------------------------------------------------
  k_jac<1>: 8 of 16 features padded                                       ms_tiny_b1
  k_jac<2, SINE, 0>: nh (r + 1) = 9 planes, odd                           ms_32x3_r2_pi3
  k_jac<2, -1, 2>: class NIF, skip connections                            nif_32x2_pi3
  k_jac<3, SINE, 1>: PEXACT false (576 f32x4 per plane, 256 threads),     ms_res_48x2_pres
    resblocks
  k_jac<6>: grid cap 256, 3 planes, odd                                   ms_96x1_r2
  k_jac<8>: one plane buffer (one_buf), 36 planes                         ms_128x6_r5_si2
  k_jac: B <= 32, two waves inactive (t16 clamped to nt16 - 1)            ragged B = 1, 15, 17, 31
  k_jac: B = 33..48, an active wave without a valid point (ptc clamped)   ragged B = 33, 48
  k_jac: B = 49..63 / 65, a ragged last tile / a second group             ragged B = 49, 63, 65
  k_jac, plain and HESS: tg += gridDim.x, last_group, the prefetch of     wrap-around B = 64 cap + 64 + 17 on ms_32x3_r2_pi3,
    plane 0 for the next group, gpar carried across groups (its parity      nif_32x2_pi3 (cap 512, NBL 2), ms_96x1_r2 (cap 256,
    flips with an odd plane count; one_buf has no parity)                   NBL 6, odd), ms_128x6_r5_si2 (cap 256, NBL 8, one_buf)
  nif_jacobian: parameter seed in slot 0, 1, 2 (d_c + d zd_sz), anyp      x_idx forms [0,3,4], [3,0,4], [3,4,0], [0,1,2],
    switching the whole group to the unscaled partial products              [0,1,2,3,4], [4,3,2,1,0,3,0] on the pi = 3 cases
  nif_jacobian: the host gather of rows y_idx, ny > 16                    y_idx all, reversed, [so - 1] * 17
  hessian_core: hj != hk with equal seeds, ppos[], zdd_of with repeats    x_idx forms [3,3], [0,0], [1,4,1], [3,0,4,1]
  hessian_core, last-layer class: xc.empty(), phi alone with nxc = 1      x_idx [0,2] and the parameter-only anchor form
  k_hess_gather / k_ll_hess: 16 entries of y_idx                          y_idx [0,1,1,0] * 4
  hessian_check / hessian_core: ny = 17, 17 coordinate columns,           refusals, each followed by the anchor Hessian
    17 parameter columns, x_idx < 0, x_idx = pi + si
  k_mlp_jac<1|2|4>: tile >= ntiles inside a 4-tile block                  every ragged B (1 or 2 tiles of 4); <4> at so r = 30:
                                                                            ll_cfg4_128x2_r10_so3
  k_ll_jac_out, k_through_lw, k_ll_hess: pt >= B, padded points           ragged B on ll_32x2_pi3, ll_res_48x2_r4, ll_cfg4_..
  nif_hessian_dev: the caller's pointers at float offsets 1, 2, 3,        ms_32x3_r2_pi3, ms_res_48x2_pres, ll_32x2_pi3,
    32 rows of sentinel behind each output                                  ll_cfg4_128x2_r10_so3 at B = 1, 33, 190
  nif_sobolev_forward_dev: one and two passes, parameter streams          x_idx [3,4], [0,4], [0,1,2,3,4] on the pi = 3 cases

The reference is oracle.nif_oracle.hessian_analytic in fp64 over all columns, at the project's bars (whole tensor rel-L2: y 1e-5,
J 2e-5, H 1e-4, 2e-4 with a parameter column) and per point: max |k[a] - ref[a]| <= bar max |ref| + 3 s_a, s_a = the oracle's own
movement of that point under one ulp of weight noise.  Two runs that do the same arithmetic per point (another batch size, another
position in the batch, another entry point, another pointer offset) are compared bit for bit.  Different x_index forms are NOT: a
parameter seed switches the summation path of its whole group (anyp), the primal included."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests.deriv_cases import (ANCHOR_B, BAR_J, BAR_Y, CASES, NIF_ERR_INVALID, PI3, RAGGED_B, WRAP, Ref, assert_bars, bits_equal,
                               c_hessian, c_jacobian, hbar, hessian_dev, sobolev_forward_dev)
from tests.test_gpu_parity import _cfg, _make, _rel, _one_ulp_weights  # noqa: F401  (the shared fixtures of the parity suite)

pytestmark = pytest.mark.gpu


def _build(name, B=ANCHOR_B):
    m, model, spec, ws, x, _, _ = _make((CASES[name], B), boost=1.0)
    return SimpleNamespace(m=m, model=model, e=m._engine, spec=spec, ws=ws, x=x)


@functools.lru_cache(maxsize=None)
def _anchor(name):
    """the case's model, its anchor batch and the oracle on it (computed once, shared, never modified)"""
    a = _build(name)
    a.x.setflags(write=False)
    a.ref = Ref(a.spec, a.ws, a.x)
    return a


def _cols(spec, form):
    pi, si = spec.pi, spec.si
    return {"coord": list(range(pi, pi + si)), "param": list(range(pi)), "all": list(range(pi + si))}[form]


def _layers(model, x, yi, xi):
    """JacobianLayer and HessianLayer on one batch -> (y, J) of the first, (y, J, H) of the second"""
    import nif_amd
    return nif_amd.JacobianLayer(model, yi, xi)(x), nif_amd.HessianLayer(model, yi, xi)(x)


@functools.lru_cache(maxsize=None)
def _anchor_out(name, form):
    a = _anchor(name)
    return _layers(a.model, a.x, list(range(a.spec.so)), _cols(a.spec, form))


def _same(got, want, rows=slice(None)):
    return all(bits_equal(g, w[rows]) for g, w in zip(got, want))


def _check_request(what, spec, ref, yi, xi, jac, hess, rows=slice(None)):
    """(y, J) and (y, J, H) of one request against the gather of the all-columns oracle, H bit-symmetric"""
    ry, rj, rh = ref.gather(yi, xi, rows)
    if jac is not None:
        assert_bars(what + " JacobianLayer y", jac[0], ry, BAR_Y)
        assert_bars(what + " JacobianLayer J", jac[1], rj, BAR_J)
    if hess is not None:
        assert_bars(what + " HessianLayer y", hess[0], ry, BAR_Y)
        assert_bars(what + " HessianLayer J", hess[1], rj, BAR_J)
        assert_bars(what + " HessianLayer H", hess[2], rh, hbar(spec, xi))
        assert bits_equal(hess[2], np.swapaxes(hess[2], 2, 3)), what + ": H is not bit-symmetric"


# ---- 1. anchor batches against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_anchor_batch_matches_the_oracle_whole_tensor_and_per_point(name):
    """190 points, every output, all input columns in natural order -- and the coordinate-only and parameter-only requests the
    ragged test compares against: the footing of every bit-for-bit comparison below."""
    a = _anchor(name)
    yi = list(range(a.spec.so))
    for form in ("all", "coord", "param"):
        xi = _cols(a.spec, form)
        jac, hess = _anchor_out(name, form)
        assert jac[0].shape == (ANCHOR_B, a.spec.so) and jac[1].shape == (ANCHOR_B, len(yi), len(xi))
        assert hess[2].shape == (ANCHOR_B, len(yi), len(xi), len(xi))
        _check_request("%s %s" % (name, form), a.spec, a.ref, yi, xi, jac, hess)


# ---- 2. small and ragged batches --------------------------------------------------------------------------------------------
_RAGGED = [(n, B) for n in sorted(CASES) for B in ([1, 33, 65] if n == "ms_128x6_r5_si2" else RAGGED_B)]


@pytest.mark.parametrize("name,B", _RAGGED)
def test_small_and_ragged_batches_equal_the_anchor_rows_bit_for_bit(name, B):
    """The first B anchor rows alone: once on the model that has just run the anchor batch (stale tiles of it lie behind the live
    ones in the workspace), once on a freshly built model (nothing behind them)."""
    a = _anchor(name)
    yi = list(range(a.spec.so))
    fresh = _build(name, B)
    assert all(np.array_equal(w, v) for w, v in zip(fresh.ws, a.ws))
    for form in ("coord", "param", "all"):
        xi = _cols(a.spec, form)
        want_j, want_h = _anchor_out(name, form)
        again = _layers(a.model, a.x, yi, xi)                     # the anchor batch again: deterministic, and leaves its tiles behind
        assert _same(again[0], want_j) and _same(again[1], want_h), (name, form, "the anchor batch does not repeat itself")
        for which, model in (("stale", a.model), ("fresh", fresh.model)):
            jac, hess = _layers(model, a.x[:B], yi, xi)
            for nm, got, want in zip(("Jacobian y", "Jacobian J"), jac, want_j):
                assert bits_equal(got, want[:B]), (name, B, form, which, nm, _rel(got, want[:B].astype(np.float64)))
            for nm, got, want in zip(("Hessian y", "Hessian J", "Hessian H"), hess, want_h):
                assert bits_equal(got, want[:B]), (name, B, form, which, nm, _rel(got, want[:B].astype(np.float64)))


# ---- 3. grid wrap-around of k_jac, plain and HESS ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WRAP))
def test_grid_wrap_around_of_k_jac(name):
    """B = 64 cap + 64 + 17 is cap + 2 groups: blocks 0 and 1 of the capped grid take a second group (tg += gridDim.x, plane 0
    prefetched behind the last plane, gpar carried over), the others end after one; block 1's second group has one full wave,
    one with a single valid point and two inactive ones.  The rows [0, 64) and [64 cap - 40, B) -- the first group, the end of
    the first sweep and the whole second one -- form a batch of their own that is checked against the oracle; the big batch's
    results on those rows equal it bit for bit."""
    a = _anchor(name)
    spec, cap = a.spec, WRAP[name]
    B = 64 * cap + 64 + 17
    x = np.random.default_rng(5).uniform(-1, 1, size=(B, spec.pi + spec.si)).astype(np.float32)
    sel = np.r_[0:64, 64 * cap - 40:B]
    xs = np.ascontiguousarray(x[sel])
    ref = Ref(spec, a.ws, xs)
    yi, xa = list(range(spec.so)), _cols(spec, "all")
    xh = _cols(spec, "coord") + ([] if name == "ms_128x6_r5_si2" else [0])
    import nif_amd
    small_j = nif_amd.JacobianLayer(a.model, yi, xa)(xs)
    small_h = nif_amd.HessianLayer(a.model, yi, xh)(xs)
    _check_request(name + " wrap rows, all columns", spec, ref, yi, xa, small_j, None)
    _check_request(name + " wrap rows, x_index %s" % xh, spec, ref, yi, xh, None, small_h)
    big_j = nif_amd.JacobianLayer(a.model, yi, xa)(x)
    big_h = nif_amd.HessianLayer(a.model, yi, xh)(x)
    for nm, big, small in zip(("Jacobian y", "Jacobian J", "Hessian y", "Hessian J", "Hessian H"), big_j + big_h, small_j + small_h):
        assert np.isfinite(big).all(), (name, nm, "not finite", int(np.sum(~np.isfinite(big))))
        ok = np.all((big[sel].view(np.uint32) == small.view(np.uint32)).reshape(len(sel), -1), axis=1)
        assert ok.all(), (name, nm, "rows of the big batch that differ from the small one", sel[~ok][:16].tolist(), int(np.sum(~ok)))
    assert bits_equal(big_h[2], np.swapaxes(big_h[2], 2, 3))


# ---- 4. seed slots and index forms through the raw C ABI --------------------------------------------------------------------
JAC_X = [[3], [4, 3], [0, 1, 2], [0, 3, 4], [3, 0, 4], [3, 4, 0], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0, 3, 0]]
HESS_X = [[0, 2], [4, 3], [3, 0, 4, 1], [3, 3], [0, 0], [1, 4, 1]]


@pytest.mark.parametrize("name", PI3)
def test_jacobian_seed_slots_and_index_forms_at_the_c_abi(name):
    """nif_jacobian takes the columns in groups of three; a parameter seed reads its dz/dp from slot d of the tangent buffer and
    switches its whole group to the unscaled partial products.  Every form is the gather of the all-columns oracle."""
    a = _anchor(name)
    so = a.spec.so
    for yi in (list(range(so)), list(range(so))[::-1], [so - 1] * 17):
        for xi in JAC_X:
            rc, y, J = c_jacobian(a.e, a.x, yi, xi)
            assert rc == 0, (name, yi, xi, rc, a.e.lib.nif_last_error())
            assert y.shape == (ANCHOR_B, so)                       # all outputs whatever y_idx says
            _check_request("%s nif_jacobian y_idx %s x_idx %s" % (name, yi, xi), a.spec, a.ref, yi, xi, (y, J), None)
    y, J = a.e.jacobian(a.x, [1, 1, 0], [4, 4, 3])                  # the Python surface computes the distinct entries and gathers
    _check_request(name + " Engine.jacobian with repeats", a.spec, a.ref, [1, 1, 0], [4, 4, 3], (y, J), None)


@pytest.mark.parametrize("name", PI3)
def test_hessian_index_forms_at_the_c_abi(name):
    """nif_hessian with parameter-only columns (the last-layer class: phi alone), permutations and repeats -- the same seed in
    both slots of a pair at hj != hk, repeated parameter columns (ppos, the z'' slots) -- and 16 entries of y_idx."""
    a = _anchor(name)
    so = a.spec.so
    for yi in (list(range(so)), [0, 1, 1, 0] * 4):
        for xi in HESS_X:
            rc, y, J, H = c_hessian(a.e, a.x, yi, xi)
            assert rc == 0, (name, yi, xi, rc, a.e.lib.nif_last_error())
            assert y.shape == (ANCHOR_B, so)
            _check_request("%s nif_hessian y_idx %s x_idx %s" % (name, yi, xi), a.spec, a.ref, yi, xi, None, (y, J, H))
    out = a.e.hessian(a.x, [1, 1, 0], [4, 4, 3])
    _check_request(name + " Engine.hessian with repeats", a.spec, a.ref, [1, 1, 0], [4, 4, 3], None, out)


# ---- 5. refusals leave the context usable -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PI3)
def test_refused_hessians_leave_the_context_usable(name):
    a = _anchor(name)
    so, ncol = a.spec.so, a.spec.pi + a.spec.si
    yi, xi = list(range(so)), list(range(ncol))
    rc, y0, J0, H0 = c_hessian(a.e, a.x, yi, xi)
    assert rc == 0
    _check_request(name + " nif_hessian", a.spec, a.ref, yi, xi, None, (y0, J0, H0))
    refused = [
        ("ny = 17", [0] * 17, xi, "at most 16 entries"),
        ("17 coordinate columns", yi, [3, 4] * 8 + [3], "at most 16 coordinate and 16 parameter columns"),
        ("17 parameter columns", yi, [0, 1, 2] * 5 + [0, 1], "at most 16 coordinate and 16 parameter columns"),
        ("negative x_idx", yi, [3, -1], "x_index out of range"),
        ("x_idx = pi + si", yi, [3, ncol], "x_index out of range"),
    ]
    for what, ryi, rxi, msg in refused:
        rc = c_hessian(a.e, a.x, ryi, rxi)[0]
        err = a.e.lib.nif_last_error().decode("utf-8", "replace")
        assert rc == NIF_ERR_INVALID and msg in err, (name, what, rc, err)
        rc, y, J, H = c_hessian(a.e, a.x, yi, xi)
        assert rc == 0 and bits_equal(y, y0) and bits_equal(J, J0) and bits_equal(H, H0), (name, "after", what, rc)


# ---- 6. device-pointer entries inside sentinels -----------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 33, ANCHOR_B])
@pytest.mark.parametrize("name", ["ms_32x3_r2_pi3", "ms_res_48x2_pres", "ll_32x2_pi3", "ll_cfg4_128x2_r10_so3"])
def test_hessian_dev_writes_inside_its_outputs(name, B):
    """nif_hessian_dev writes through the caller's pointers: y, dydx and d2 at float offsets 1, 2, 3 from a 16-byte boundary,
    each with 32 of its rows of sentinel behind it (a tile's tail past row B would land there) -- every pad word untouched, the
    outputs equal to nif_hessian's bit for bit."""
    a = _anchor(name)
    yi, xi = list(range(a.spec.so)), _cols(a.spec, "all")
    for yq in (yi, yi[::-1]):
        y, J, H, pads = hessian_dev(a.e, a.x[:B], yq, xi)
        assert pads == (True, True, True), (name, B, yq, "nif_hessian_dev wrote outside (y, dydx, d2)", pads)
        rc, yh, Jh, Hh = c_hessian(a.e, a.x[:B], yq, xi)
        assert rc == 0
        assert bits_equal(y, yh) and bits_equal(J, Jh) and bits_equal(H, Hh), (name, B, yq)
        if B == ANCHOR_B:
            _check_request("%s nif_hessian_dev y_idx %s" % (name, yq), a.spec, a.ref, yq, xi, None, (y, J, H))


@functools.lru_cache(maxsize=None)
def _sobolev_anchor(name, xi):
    a = _anchor(name)
    return sobolev_forward_dev(a.e, a.x, list(xi))


@pytest.mark.parametrize("B", [1, 33, ANCHOR_B])
@pytest.mark.parametrize("name", PI3)
def test_sobolev_forward_dev_writes_inside_its_outputs(name, B):
    """predict() of the two-output model, coordinate and parameter columns, one pass and two: u and du/dx inside sentinels,
    against the oracle (another kernel than k_jac: no bit equality with it), the first B rows equal to the anchor call's."""
    a = _anchor(name)
    yi = list(range(a.spec.so))
    for xi in ([3, 4], [0, 4], [0, 1, 2, 3, 4]):
        rc0, u0, J0, pads0 = _sobolev_anchor(name, tuple(xi))
        assert rc0 == 0, (name, xi, rc0, a.e.lib.nif_last_error())
        rc, u, J, pads = sobolev_forward_dev(a.e, a.x[:B], xi)
        assert rc == 0, (name, B, xi, rc, a.e.lib.nif_last_error())
        assert pads == (True, True), (name, B, xi, "nif_sobolev_forward_dev wrote outside (u, du/dx)", pads)
        assert bits_equal(u, u0[:B]) and bits_equal(J, J0[:B]), (name, B, xi)
        if B == ANCHOR_B:
            assert pads0 == (True, True)
            _check_request("%s nif_sobolev_forward_dev x_idx %s" % (name, xi), a.spec, a.ref, yi, xi, (u, J), None)
