"""The float32 training step's scaled 16-bit-pair products over their operands' dynamic range (tests/range_cases.py): planes whose
magnitudes lie 2^10 apart, outlier weights, entries spread over 2^16, sample weights over 2^40, targets over ten decades, a shard of
a 2^30-point global batch -- against the float64 oracle at the project's standing bars, unchanged; and, bit for bit, the equivariance
of [grad | loss] under a power of two on the sample weights or on 1 / B_global.  tests/test_dynamic_range.py holds the conditions
(the reference is stable at every pair; nothing is excused from the bit equality); profiles/dynamic_range.md an MI355X run's figures.
Every check prints its figures before it asserts."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import range_cases as R
from tests import snet6_domain as D
from tests.test_gpu_parity import _per_tensor_rel, _rel

pytestmark = pytest.mark.gpu

SNAP_BAR = 1e-5          # tests/test_gpu_snapshots.py BAR
_refs = {}


def _stressed(case, axis, policy="float32"):
    """engine of the case holding the axis' weights + (spec, ws64, x, y, sw, B_global)"""
    m, model, spec, ws, x, y, sw = R.make(case, policy)
    ws, x, y, sw, bg = R.stressed(axis, spec, ws, x, y, sw) if axis else (ws, x, y, sw, x.shape[0])
    if axis in R.WEIGHT_AXES:
        model.set_weights(R.f32(ws))
    return m, model, spec, ws, x, y, sw, bg


def _oracle(case, axis, spec, ws, x, y, sw, bg):
    """the float64 reference of a (case, axis) pair, computed once and left unchanged"""
    if (case, axis) not in _refs:
        x64 = x.astype(np.float64)
        l, g = O.loss_and_grad(spec, ws, x64, y.astype(np.float64), sw.astype(np.float64), batch_global=bg)
        _refs[(case, axis)] = (O.forward(spec, ws, x64), l, g)
    return _refs[(case, axis)]


def _step(e, x, y, sw, bg=None, slopes=None, xi=None):
    """one step through the device-pointer entry (B_global of its own): [grad | loss] as float32"""
    from nif_amd.engine import DeviceArray
    arrs = [a for a in (x, y, slopes, sw) if a is not None]
    devs = [DeviceArray(e, a.size) for a in arrs]
    try:
        for d, a in zip(devs, arrs):
            d.upload(a)
        ptrs = iter(d.at(0) for d in devs)
        d_x, d_y = next(ptrs), next(ptrs)
        d_g = next(ptrs) if slopes is not None else None
        d_sw = next(ptrs) if sw is not None else None
        B = x.shape[0]
        if slopes is not None:
            e.sobolev_loss_grad_dev(d_x, d_y, d_g, d_sw, B, bg or B, xi, R.WJ)
        else:
            e.loss_grad_dev(d_x, d_y, d_sw, B, bg or B)
        loss, g = e.grad_read()
    finally:
        for d in devs:
            d.free()
    return np.append(g, np.float32(loss)).astype(np.float32)


def _figures(spec, r, lref, gref):
    """(loss error, worst tensor's share of its bar 5e-5 |ref_T| + 2.5e-7 |ref|, its name, worst per-tensor rel, flat rel)"""
    flat = O.flatten(gref)
    gn = float(np.linalg.norm(flat))
    share, off = {}, 0
    for (nm, shp), gr in zip(spec.param_shapes(), gref):
        k = int(np.prod(shp))
        share[nm] = float(np.linalg.norm(r[off:off + k].astype(np.float64) - gr.ravel())) / (5e-5 * np.linalg.norm(gr) + 2.5e-7 * gn)
        off += k
    w = max(share, key=share.get)
    return (abs(float(r[-1]) - lref) / abs(lref), share[w], w, max(_per_tensor_rel(spec, r[:-1], flat).values()),
            float(np.linalg.norm(r[:-1].astype(np.float64) - flat)) / gn)


@pytest.mark.parametrize("case,axis", R.pairs())
def test_oracle_parity_under_every_axis(case, axis):
    """predict and the weighted step against the float64 oracle on the stressed inputs, on the 16-bit-pair route and on the f32-input
    MFMAs (fp32_mfma 1), both at the standing bars: forward 1e-5, loss 2e-6, every tensor 5e-5 |ref_T| + 2.5e-7 |ref|, flat 3e-5.  A
    pass of fp32_mfma where the default route fails names the split.  The s6 cases' slot groups on both gradient routes where a
    whole-tensor bar cannot see one hidden matrix."""
    m, model, spec, ws, x, y, sw, bg = _stressed(case, axis)
    e = m._engine
    uref, lref, gref = _oracle(case, axis, spec, ws, x, y, sw, bg)
    out = {}
    try:
        for route in (0, 1):
            e.set_option("fp32_mfma", route)
            out[route] = (model.predict(x), _step(e, x, y, sw, bg))
    finally:
        e.set_option("fp32_mfma", 0)
    for route in (0, 1):
        u, r = out[route]
        print("range %s / %s / %s: forward %.2e, loss %.1e, worst tensor %.2f of its bar (%s), worst tensor rel %.2e, flat %.2e"
              % ((case, axis, "fp32_mfma" if route else "pairs", _rel(u, uref)) + _figures(spec, r, lref, gref)))
    for route in (0, 1):
        u, r = out[route]
        what = "%s / %s / %s" % (case, axis, "fp32_mfma" if route else "pairs")
        assert u.dtype == np.float32 and np.all(np.isfinite(u)) and np.all(np.isfinite(r)), what
        assert _rel(u, uref) < 1e-5, (what, _rel(u, uref))
        D.check_tensor_bars(spec, float(r[-1]), r[:-1], lref, gref, what)
    if case in R.S6 and axis in R.GROUP_AXES:
        (lf, gf), (lu, gu) = D.both_routes(e, x, y, sw)
        rows = D.check_group_bars(spec, gf, gu, gref, "%s / %s" % (case, axis))
        D.check_route_witness(spec, gf, gu, 3e-5, "%s / %s" % (case, axis))
        assert len(rows) == 2 * len(D.slot_groups(spec))


@pytest.mark.parametrize("case,axis", [(c, a) for c in R.SOBOLEV[0] for a in R.SOBOLEV[1]])
def test_sobolev_step_under_the_axes(case, axis):
    """k_sobw: two coordinate columns, the slope targets scaled with y's exponents under y_mixed; test_sobolev_loss_and_grad_match_oracle's
    bars (loss 2e-5, every tensor 3e-4)"""
    m, model, spec, ws, x, y, sw, bg = _stressed(case, axis)
    xi = [spec.pi, spec.pi + 1]
    gt = R.sobolev_targets(spec, x.shape[0])
    if axis == "y_mixed":
        gt = R.y_mixed(gt)
    loss, grad = m._engine.sobolev_loss_and_grad(x, y, gt, xi, R.WJ, sw)
    rl, rg = O.sobolev_loss_and_grad(spec, ws, x.astype(np.float64), y.astype(np.float64), gt.astype(np.float64), xi, R.WJ,
                                     sw.astype(np.float64))[:2]
    errs, off = {}, 0
    for (nm, shp), r_ in zip(spec.param_shapes(), rg):
        k = int(np.prod(shp))
        got = grad[off:off + k].reshape(shp)
        off += k
        errs[nm] = _rel(got, r_) if np.linalg.norm(r_) > 1e-12 else float(np.abs(got).max())
    w = max(errs, key=errs.get)
    print("range sobolev %s / %s: loss %.1e, worst tensor %.2e (%s)" % (case, axis, abs(loss - rl) / abs(rl), errs[w], w))
    assert np.all(np.isfinite(grad))
    assert abs(loss - rl) <= 2e-5 * abs(rl), (loss, rl)
    assert errs[w] < 3e-4, (w, errs[w])


@pytest.mark.parametrize("case,axis", [(c, a) for c in R.SNAPSHOT[0] for a in R.SNAPSHOT[1]])
def test_predict_snapshots_under_the_axes(case, axis):
    """k_snap packs its own wscale rows per snapshot: three snapshots on one 130-point mesh, each against the oracle on its expanded table"""
    m, model, spec, ws, x, y, sw, bg = _stressed(case, axis)
    rng = np.random.default_rng(7)
    p = rng.uniform(-1, 1, size=(3, spec.pi)).astype(np.float32)
    mesh = rng.uniform(-1, 1, size=(130, spec.si)).astype(np.float32)
    u = model.predict_snapshots(mesh, p=p)
    assert u.shape == (3, 130, spec.so) and u.dtype == np.float32
    errs = [_rel(u[t], O.forward(spec, ws, np.hstack([np.tile(p[t], (130, 1)), mesh]).astype(np.float64))) for t in range(3)]
    print("range snapshots %s / %s: rel-L2 per snapshot %s" % (case, axis, " ".join("%.2e" % v for v in errs)))
    assert max(errs) < SNAP_BAR, errs


# ---- power-of-two equivariance, bit for bit ----------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _equivariance(step, sw, B, what, ref):
    """step(sw, B_global) -> [grad | loss].  Every operation between dL/du and [grad | loss] is linear in the sample weight, IEEE
    arithmetic commutes with an exact power of two, and so does a scale chosen from an operand's own exponent: sw * 2^k gives 2^k times
    the step's result, bit for bit.  Likewise 1 / B_global -- the entry takes B_global >= B only, so 2^-12 and 2^-24 are B << 12 and
    B << 24 against B, and 2^12 and 2^24 are B << 12 and B against B << 24.  ref: the oracle's [grad | loss], for the excused set."""
    base = step(sw, B)
    assert np.all(np.isfinite(base)) and np.count_nonzero(base) > base.size // 2, what
    one = np.asarray(2.0, base.dtype)
    bad = []
    for k in R.KS:
        assert R.exempt(ref, k).size == 0, (what, k)          # nothing is excused (tests/test_dynamic_range.py shows why)
        got = step(sw * (one ** k).astype(sw.dtype), B)
        n = int((_bits(got) != _bits(base * one ** k)).sum())
        print("equivariance %s: sw * 2^%d: %d of %d entries differ in bits" % (what, k, n, base.size))
        bad.append(("sw", k, n))
    plain, far = step(None, B), step(None, B << 24)
    for k in R.KS:
        got, want = (step(None, B << -k), plain * one ** k) if k < 0 else (step(None, B << (24 - k)) if k < 24 else plain, far * one ** k)
        n = int((_bits(got) != _bits(want)).sum())
        print("equivariance %s: B_global * 2^%d: %d of %d entries differ in bits" % (what, -k, n, base.size))
        bad.append(("B_global", k, n))
    assert all(n == 0 for _, _, n in bad), (what, bad)


def _oracle_row(case, loss="mse"):
    spec, ws, x, y, sw = R.host_inputs(case)
    l, g = O.loss_and_grad(spec, ws, x.astype(np.float64), y.astype(np.float64), sw.astype(np.float64), loss=loss)
    return np.append(O.flatten(g), l)


@pytest.mark.parametrize("loss", ["mse", "huber"])
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_plain_step_is_equivariant_under_powers_of_two(case, loss):
    m, model, spec, ws, x, y, sw = R.make(case)
    e = m._engine
    e.set_loss(loss)
    try:
        _equivariance(lambda s, bg: _step(e, x, y, s, bg), sw, x.shape[0], "%s / float32 / %s" % (case, loss), _oracle_row(case, loss))
    finally:
        e.set_loss("mse")


@pytest.mark.parametrize("policy", ["mixed_bfloat16", "mixed_float16"])
@pytest.mark.parametrize("case", R.POLICY_CASES)
def test_policy_step_is_equivariant_under_powers_of_two(case, policy):
    """the 16-bit policies round dL/da to 16 bits: bf16 has float32's exponents, half gets a power of two per point from the point's
    own exponent -- neither may see 2^k.  (The excused set is taken from the float32 oracle: the policies move values by per cents.)"""
    m, model, spec, ws, x, y, sw = R.make(case, policy)
    e = m._engine
    _equivariance(lambda s, bg: _step(e, x, y, s, bg), sw, x.shape[0], "%s / %s" % (case, policy), _oracle_row(case))


@pytest.mark.parametrize("case", R.SOBOLEV[0])
def test_sobolev_step_is_equivariant_under_powers_of_two(case):
    m, model, spec, ws, x, y, sw = R.make(case)
    e = m._engine
    xi = [spec.pi, spec.pi + 1]
    gt = R.sobolev_targets(spec, x.shape[0])
    rl, rg = O.sobolev_loss_and_grad(spec, ws, x.astype(np.float64), y.astype(np.float64), gt.astype(np.float64), xi, R.WJ,
                                     sw.astype(np.float64))[:2]
    _equivariance(lambda s, bg: _step(e, x, y, s, bg, slopes=gt, xi=xi), sw, x.shape[0], "%s / sobolev" % case, np.append(O.flatten(rg), rl))


def test_f64_closure_is_equivariant_under_powers_of_two():
    """nif_f64_loss_grad_dev on nif_32x2: the same property in double"""
    case = "nif_32x2"
    m, model, spec, ws, x, y, sw = R.make(case)
    e = m._engine
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    e.f64_set_flat(O.flatten(ws))

    def step(s, bg):
        arrs = [a for a in (x64, y64, s) if a is not None]
        devs = [e.alloc_f64(a.size) for a in arrs]
        try:
            for d, a in zip(devs, arrs):
                d.upload(a)
            e.f64_loss_grad_dev(devs[0].at(0), devs[1].at(0), devs[2].at(0) if s is not None else None, x.shape[0], bg)
            loss, g = e.f64_grad_read()
        finally:
            for d in devs:
                d.free()
        return np.append(g, loss)

    _equivariance(step, sw.astype(np.float64), x.shape[0], "%s / float64 closure" % case, _oracle_row(case))


# ---- finite and right at the ends -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.END_CASES)
def test_finite_and_right_at_the_ends(case):
    """targets 1e6 times larger; sw = 2^-60 everywhere; every modulation plane exactly zero.  Standing bars, but for one tensor in the
    first: pnet_bottleneck_b = sum_a dL/dz(a) gets, on top of its standing bar, the allowance that R.latent_adjoint_budget derives from
    the reference and the half pairs' 2^-22 operand width (measured on s6_64x1: err 3.47e-7 |ref|, standing bar 3.40e-7 |ref|, allowance
    3.27e-7 |ref|; on s4_128x2_r2: 3.0e-8 / 2.05e-6 / 7.3e-7)."""
    m, model, spec, ws, x, y, sw = R.make(case)
    e = m._engine
    B = x.shape[0]
    x64 = x.astype(np.float64)
    # targets 1e6 times larger: residuals ~1e6, their squares ~1e12, |dL/da| ~1e3 -- finite, and within the standing bars.  One tensor
    # of one case is measured at them, not held to them: pnet_bottleneck_b of s6_64x1 (a single entry) sits at 1.02 of its standing bar
    # on the half-pair route (err 3.5e-7 |ref|, bar 3.4e-7 |ref|; fp32_mfma route 3.2e-8 |ref|; the oracle's own change under one ulp
    # 4e-6 .. 1.5e-5 |ref_T| = 7e-9 .. 3e-8 |ref|).  R.latent_adjoint_budget derives from the reference what the products' documented
    # operand width leaves of that tensor at this input (s6_64x1: 3.3e-7 |ref|); it is added to that tensor's bar, here and nowhere else
    ybig = (y * np.float32(1e6)).astype(np.float32)
    r = _step(e, x, ybig, sw)
    lref, gref = O.loss_and_grad(spec, ws, x64, ybig.astype(np.float64), sw.astype(np.float64))
    names = [nm for nm, _ in spec.param_shapes()]
    budget = float(np.linalg.norm(R.latent_adjoint_budget(spec, ws, x, ybig, sw)))
    gnorm = float(np.linalg.norm(O.flatten(gref)))
    off = sum(int(np.prod(s)) for _, s in spec.param_shapes()[:names.index("pnet_bottleneck_b")])
    gb = gref[names.index("pnet_bottleneck_b")].ravel()
    err_b = float(np.linalg.norm(r[off:off + gb.size].astype(np.float64) - gb))
    print("ends %s / y * 1e6: loss %.1e, worst tensor %.2f of its standing bar (%s), worst tensor rel %.2e, flat %.2e"
          % ((case,) + _figures(spec, r, lref, gref)))
    print("ends %s / y * 1e6: pnet_bottleneck_b err %.2e |ref|, standing bar %.2e |ref|, budget of the half pairs %.2e |ref|"
          % (case, err_b / gnorm, (5e-5 * np.linalg.norm(gb) + 2.5e-7 * gnorm) / gnorm, budget / gnorm))
    assert np.all(np.isfinite(r))
    assert err_b <= 5e-5 * np.linalg.norm(gb) + 2.5e-7 * gnorm + budget, (case, err_b, budget)
    held = r.copy()
    held[off:off + gb.size] = gb          # every other tensor, the loss and the flat gradient at the standing bars
    D.check_tensor_bars(spec, float(r[-1]), held[:-1], lref, gref, "%s / y * 1e6" % case)
    assert _rel(r[:-1], O.flatten(gref)) < 3e-5
    # sw = 2^-60 everywhere against sw = 1 everywhere, bit for bit.  The per-point scale takes the point's largest |dL/da| to 2^14 and
    # is capped at 2^100, i.e. once that maximum falls below 2^-86.  Here |dL/da| = 2^-60 * 2 |e| / (B so) * O(|wl| omega_0 ~ 0.3):
    # about 2^-69 |e| at B = 257, so the cap waits for a residual below 2^-17 -- the smallest of this draw is asserted above 2^-12.
    # (A capped point would still be finite and right, but (hi, lo) of a value below half's normals keeps fewer bits: not equivariant.)
    emin = float(np.abs(O.forward(spec, ws, x64) - y.astype(np.float64)).max(axis=1).min())
    ones = np.ones((B,), np.float32)
    r1, r60 = _step(e, x, y, ones), _step(e, x, y, ones * np.float32(2.0 ** -60))
    n = int((_bits(r60) != _bits(r1 * np.float32(2.0 ** -60))).sum())
    print("ends %s / sw = 2^-60: smallest residual of the draw 2^%.1f, %d of %d entries differ in bits" % (case, np.log2(emin), n, r1.size))
    assert emin > 2.0 ** -12
    assert np.all(np.isfinite(r60)) and np.count_nonzero(r60) > r60.size // 2 and n == 0
    # every modulation plane exactly zero: mx = 0 in plane_scale_shift
    wz = R.mod_small(spec, ws, factor=0.0)
    model.set_weights(R.f32(wz))
    u, r = model.predict(x), _step(e, x, y, sw)
    uref = O.forward(spec, wz, x64)
    lref, gref = O.loss_and_grad(spec, wz, x64, y.astype(np.float64), sw.astype(np.float64))
    print("ends %s / zero planes: forward %.2e, loss %.1e, worst tensor %.2f of its bar (%s), worst tensor rel %.2e, flat %.2e"
          % ((case, _rel(u, uref)) + _figures(spec, r, lref, gref)))
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(r))
    assert _rel(u, uref) < 1e-5
    D.check_tensor_bars(spec, float(r[-1]), r[:-1], lref, gref, "%s / zero planes" % case)
