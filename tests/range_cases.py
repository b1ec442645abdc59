"""Cases, stress builders and bars of tests/test_dynamic_range.py (CPU) and tests/test_gpu_dynamic_range.py: the scaled 16-bit-pair
products of the float32 training step over their operands' dynamic range.

The hidden n x n products of the float32 step run as half (hi, lo) pairs under three families of power-of-two scales: one per plane
and hidden matrix (csrc/k_pack_dev.h plane_scale_shift: the plane's maximum goes to 2^14), a fixed 2^12 on the sines, and one per
point on dL/da (from the point's maximum exponent, capped at 2^100).  Every other GPU test draws its weights from O.init_weights and
its data from [-1, 1] -- one operating point of all three.  The axes below move them, by exact powers of two, under fixed seeds.

Shallow on purpose: a deeper SIREN is chaotic in its own weights, and a parity bar means something only where the float64 reference
is itself stable under one float32 ulp of its weights (tests/test_dynamic_range.py asserts that for every (case, axis) pair;
profiles/dynamic_range.md holds the table).

Out of scope:
  - growing the planes (x 2^3 and more) and widening x: the net's own conditioning then exceeds the bars (hidden planes x 2^4 on a
    64x4 net move the oracle by 4e2 under one ulp, outlier x 2^8 on 64x2 by 4.3e-5, x * 8 by 3.1e-5);
  - the |a| >= 2^20 sine path.

Every check prints its figures before it asserts."""
import numpy as np

from oracle import nif_oracle as O
from tests.test_gpu_parity import _cfg, _make, _make_policy, _per_tensor_rel, _snet6_shape

# name: (cfg, batch, number of 16-feature blocks of its kernel, runs on k_snet6)
CASES = {
    "s6_64x1": (_cfg("NIFMultiScale", 64, 1, 32, 2, 1, 1, 1, 1, p_act="sine"), 257, 4, True),             # k_snet6<4, 0, 1, 1>
    "s6_64x2_si2_so2": (_cfg("NIFMultiScale", 64, 2, 32, 2, 1, 2, 2, 1, p_act="sine"), 257, 4, True),     # k_snet6<4, 0, 0, 0>
    "s4_32x2_r2": (_cfg("NIFMultiScale", 32, 2, 32, 2, 2, 2, 1, 1, p_act="swish"), 129, 2, False),        # k_snet4<2, .., 3>
    "s4_64x2_r3": (_cfg("NIFMultiScale", 64, 2, 32, 2, 3, 2, 1, 1, p_act="swish"), 129, 4, False),        # k_snet4<4, .., 3> + k_gw_lds
    "s4_96x2_r2": (_cfg("NIFMultiScale", 96, 2, 32, 1, 2, 2, 1, 1), 129, 6, False),                       # k_snet4<6, .., 3>
    "s4_128x2_r2": (_cfg("NIFMultiScale", 128, 2, 32, 2, 2, 2, 1, 1), 129, 8, False),                     # k_snet4<8, .., 3> + k_gw8
    "s4_res_64x2": (_cfg("NIFMultiScale", 64, 2, 32, 2, 2, 2, 1, 1, s_res=True), 129, 4, False),          # resblock form
    "ll_32x2_r3": (_cfg("LL", 32, 2, 32, 1, 3, 2, 2, 1), 130, 2, False),                                  # k_pnet + k_ll_out, phi planes
    "nif_32x2": (_cfg("NIF", 32, 2, 32, 2, 1, 1, 1, 1), 300, 2, False),                                   # k_small / k_nets: fp32 FMA, the control
}
S6 = [c for c in CASES if CASES[c][3]]
WEIGHT_AXES = ("base_small", "mod_small", "outlier6", "spread")
AXES = WEIGHT_AXES + ("sw_wide", "y_mixed", "bg_2p30")
SOBOLEV = (("s6_64x2_si2_so2", "s4_res_64x2"), ("base_small", "outlier6", "sw_wide", "y_mixed"))
SNAPSHOT = (("s6_64x1", "s4_64x2_r3"), ("base_small", "outlier6", "spread"))
GROUP_AXES = ("base_small", "outlier6", "spread")
POLICY_CASES = ("s6_64x1", "s4_64x2_r3")
END_CASES = ("s6_64x1", "s4_128x2_r2")
KS = (-24, -12, 12, 24)
SENS_BAR, SENS_FWD_BAR = 2e-5, 1e-5          # the oracle's own change under one float32 ulp: 0.4 of the 5e-5 tensor bar; the forward bar
SEED = 5
WJ = 0.05                                    # weight of the slope term in the Sobolev checks


def sobolev_targets(spec, B):
    """slope targets [B, so, 2] of the Sobolev checks: the draw of test_sobolev_loss_and_grad_match_oracle"""
    return np.random.default_rng(11).uniform(-1, 1, size=(B, spec.so, 2)).astype(np.float32)


def axes_of(case):
    """the last-layer class has no modulation planes (its hidden matrices are plain Keras variables): mod_small has nothing to act on"""
    return tuple(a for a in AXES if not (a == "mod_small" and CASES[case][0][0] == "NIFMultiScaleLastLayerParameterized"))


def pairs(cases=None, axes=None):
    return [(c, a) for c in (cases or sorted(CASES)) for a in axes_of(c) if axes is None or a in axes]


def spec_of(case):
    """the case's Spec, asserted to sit in the kernel the table names: a typo cannot move it out"""
    (kind, cs, cp), B, nbl, s6 = CASES[case]
    spec = O.Spec(kind, cs, cp)
    assert _snet6_shape(spec) == s6 and (spec.n + 15) // 16 == nbl, case
    if case.startswith("s4_"):
        assert spec.kind == O.KIND_MS and spec.s_res == ("res" in case), case
    if case.startswith("ll_"):
        assert spec.kind == O.KIND_LL, case
    if case.startswith("nif_"):
        assert spec.kind == O.KIND_NIF, case
    return spec


def make(case, policy="float32"):
    """(m, model, spec, ws64, x, y, sw) as tests.test_gpu_parity._make / _make_policy, on the case's own shape"""
    cfg, B = CASES[case][:2]
    spec_of(case)
    return _make((cfg, B)) if policy == "float32" else _make_policy((cfg, B), policy)


def host_inputs(case, seed=0):
    """what _make draws, without an engine: (spec, ws64, x, y, sw) -- the same generator calls in the same order"""
    (kind, cs, cp), B = CASES[case][:2]
    spec = spec_of(case)
    rng = np.random.default_rng(seed)
    ws = O.init_weights(spec, rng, dtype=np.float32)
    names = [nm for nm, _ in spec.param_shapes()]
    if kind != "NIF":
        boost = 30.0 if spec.kind == O.KIND_LL else 2.0
        ws[names.index("pnet_last_w")] = (ws[names.index("pnet_last_w")] * boost).astype(np.float32)
    x = rng.uniform(-1, 1, size=(B, spec.pi + spec.si)).astype(np.float32)
    y = rng.uniform(-1, 1, size=(B, spec.so)).astype(np.float32)
    sw = rng.uniform(0.5, 1.5, size=(B,)).astype(np.float32)
    return spec, [w.astype(np.float64) for w in ws], x, y, sw


# ---- the hidden planes ---------------------------------------------------------------------------------------------------------------
def hidden_planes(spec, ws):
    """[(matrix j, plane k, view)]: plane k < r of hidden matrix j is its modulation plane k (a row slice of pnet_last_w), plane r its
    base plane (a slice of pnet_last_b).  Last-layer class: the phi-net's hidden matrices, each its own base plane.  The views write
    through into ws."""
    names = [nm for nm, _ in spec.param_shapes()]
    out = []
    if spec.kind == O.KIND_LL:
        mats = [nm for nm in names if nm.startswith("snet_h") and "_w" in nm]
        assert len(mats) == spec.n_hidden_mats
        return [(j, 0, ws[names.index(nm)].reshape(-1)) for j, nm in enumerate(mats)]
    lw, lb = ws[names.index("pnet_last_w")], ws[names.index("pnet_last_b")]
    for j, (a, b) in enumerate(spec.slices()["wh"]):
        out += [(j, k, lw[k, a:b]) for k in range(spec.r)]
        out.append((j, spec.r, lb[a:b]))
    return out


def _is_base(spec, k):
    return spec.kind == O.KIND_LL or k == spec.r


def _copy(ws):
    return [np.array(w, dtype=np.float64) for w in ws]


def _f32_exact(ws):
    for w in ws:
        assert np.array_equal(w.astype(np.float32).astype(np.float64), w)
    return ws


def base_small(spec, ws, seed=SEED):
    """base plane of every hidden matrix x 2^-10: the plane scales sit 2^10 apart, the pre-scaled biases dominate"""
    ws = _copy(ws)
    for j, k, v in hidden_planes(spec, ws):
        if _is_base(spec, k):
            v *= 2.0 ** -10
    return _f32_exact(ws)


def mod_small(spec, ws, seed=SEED, factor=2.0 ** -12):
    """modulation planes x 2^-12 (factor 0: exact zeros, mx = 0 in plane_scale_shift)"""
    ws = _copy(ws)
    for j, k, v in hidden_planes(spec, ws):
        if not _is_base(spec, k):
            v *= factor
    return _f32_exact(ws)


def outlier6(spec, ws, seed=SEED):
    """one entry of each plane of each hidden matrix x 2^6: it sets the plane scale, everything else loses its lo bits.  The entry is
    drawn among those within a factor 2 of the plane's maximum, so that it leads the plane by 2^5 at least"""
    ws = _copy(ws)
    rng = np.random.default_rng(seed)
    for j, k, v in hidden_planes(spec, ws):
        nz = np.flatnonzero(np.abs(v) >= 0.5 * np.abs(v).max())
        v[nz[rng.integers(nz.size)]] *= 2.0 ** 6
    return _f32_exact(ws)


def spread(spec, ws, seed=SEED):
    """every entry of every hidden plane x 2^j, j uniform integer in [-16, 0]"""
    ws = _copy(ws)
    rng = np.random.default_rng(seed)
    for j, k, v in hidden_planes(spec, ws):
        v *= 2.0 ** rng.integers(-16, 1, size=v.shape)
    return _f32_exact(ws)


def sw_wide(B, seed=SEED):
    """sw = 2^j, j uniform integer in [-20, 20] per point: drives the per-point dL/da scale"""
    return (2.0 ** np.random.default_rng(seed).integers(-20, 21, size=B)).astype(np.float32)


def y_mixed_exponents(B, seed=SEED):
    return np.random.default_rng(seed).integers(-6, 5, size=B)


def y_mixed(y, seed=SEED):
    """every row of y x 10^j, j uniform integer in [-6, 4]: residuals from 1e-6 to 1e4 within one tile.  (10^j is no power of two: the
    product is rounded to float32 once, here, and both sides get the rounded targets.)  Any trailing axes (slope targets) follow."""
    f = 10.0 ** y_mixed_exponents(y.shape[0], seed).astype(np.float64)
    return (y.astype(np.float64) * f.reshape((-1,) + (1,) * (y.ndim - 1))).astype(np.float32)


def bg_2p30(B):
    """B_global = B << 22 (a shard of a 2^29..2^30-point global batch): dL/da lands far below half's range"""
    return B << 22


def stressed(axis, spec, ws, x, y, sw):
    """(ws64, x, y, sw, B_global) of one axis on a case's inputs; ws float64 holding float32 values"""
    B = x.shape[0]
    if axis in WEIGHT_AXES:
        return globals()[axis](spec, ws), x, y, sw, B
    if axis == "sw_wide":
        return ws, x, y, sw_wide(B), B
    if axis == "y_mixed":
        return ws, x, y_mixed(y), sw, B
    assert axis == "bg_2p30", axis
    return ws, x, y, sw, bg_2p30(B)


def f32(ws):
    return [w.astype(np.float32) for w in ws]


# ---- what a stress must do (asserted on the CPU) ---------------------------------------------------------------------------------------
def plane_max_exponents(spec, ws):
    """{(matrix, plane): exponent of the plane's largest magnitude} -- what plane_scale_shift reads"""
    return {(j, k): int(np.frexp(np.abs(v).max())[1]) for j, k, v in hidden_planes(spec, ws)}


def plane_exponent_span(v):
    e = np.frexp(np.abs(v[v != 0]))[1]
    return int(e.max() - e.min())


# ---- bars -------------------------------------------------------------------------------------------------------------------------------
def sensitivity(spec, ws, x, y, sw, bg, one_ulp):
    """the float64 oracle on ws and on ws moved one float32 ulp: (worst per-tensor change under _per_tensor_rel, its tensor, forward rel-L2)"""
    x64, y64, s64 = x.astype(np.float64), y.astype(np.float64), sw.astype(np.float64)
    ws_n = one_ulp(ws)
    g0 = O.flatten(O.loss_and_grad(spec, ws, x64, y64, s64, batch_global=bg)[1])
    g1 = O.flatten(O.loss_and_grad(spec, ws_n, x64, y64, s64, batch_global=bg)[1])
    rel = _per_tensor_rel(spec, g1, g0)
    u0, u1 = O.forward(spec, ws, x64), O.forward(spec, ws_n, x64)
    worst = max(rel, key=rel.get)
    return rel[worst], worst, float(np.linalg.norm(u1 - u0) / np.linalg.norm(u0))


def latent_adjoint_budget(spec, ws, x, y, sw):
    """What the half-pair products' documented operand width leaves of pnet_bottleneck_b at one input, from the float64 reference alone.

    pnet_bottleneck_b = sum_a dL/dz(a), and dL/dz_k(a) = sum_s g(a, s) M^(k)[s] over the po slots s is what leaves the ShapeNet kernels:
    per point, a sum of dot products <h_in, M^(k) dL/da> with heavy cancellation ("where the gradient error of the default
    path comes from").  Their operands are (hi, lo) half pairs, 11 + 11 bits: 2^-22 per operand against float32's 2^-24,
    so a point's dL/dz_k carries an error of up to 2^-22 S_k(a), S_k(a) = sum_s |g(a, s) M^(k)[s]|.  The points' errors come from
    different operands; over the batch they add as a root sum of squares:

        budget_k = 2^-22 sqrt(sum_a S_k(a)^2)

    Where the targets are 1e6 times the net's output the residual is the target's, its sign random from point to point, and the tensor
    cancels to 1e-4 of sum_a S(a) (s6_64x1: |ref_T| = 1.8e-3 |ref|, sum_a S(a) = 18 |ref|): the budget is then of the size of the
    standing bar's absolute term 2.5e-7 |ref| (3.3e-7 |ref| there; 8.5e-8 |ref| at the unscaled targets), and the standing bar alone
    cannot hold.  tests/test_dynamic_range.py asserts that it never exceeds the tensor's standing bar.  Returns budget [r]."""
    B = x.shape[0]
    x64, s64 = x.astype(np.float64), sw.astype(np.float64)
    pout = O.pnet_forward(spec, ws, x64[:, :spec.pi], keep=True)[0]
    u, tape = O.shapenet_given_w(spec, x64[:, spec.pi:spec.pi + spec.si], pout, keep=True)
    g_u = 2.0 * (u - y.astype(np.float64)) * s64[:, None] / (B * spec.so)
    g = O.shapenet_given_w_backward(spec, tape, g_u)                                   # [B, po]
    W = ws[[nm for nm, _ in spec.param_shapes()].index("pnet_last_w")]               # [r, po]
    S = np.abs(g[:, None, :] * W[None, :, :]).sum(axis=2)                              # [B, r]
    return 2.0 ** -22 * np.sqrt((S ** 2).sum(axis=0))


def exempt(ref_flat, k):
    """entries of [grad | loss] excused from the bit equality under 2^k: the oracle's value times 2^k lies below 2^-100 (float32 keeps
    24 bits only down to 2^-126; below, a scaled and an unscaled run round differently by right).  Exact zeros scale exactly."""
    a = np.abs(np.asarray(ref_flat, np.float64)) * 2.0 ** k
    return np.flatnonzero((a != 0) & (a < 2.0 ** -100))
