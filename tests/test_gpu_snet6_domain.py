"""The fused-gradient training kernel k_snet6 (csrc/k_snet6.hip) over its whole admission domain: one to four hidden matrices, one to
three coordinates and outputs, padded widths, ragged batches, zero sample weights, several tile rounds per workgroup, one context
over changing batch sizes, and the two policy forms -- against the fp64 oracle per Keras tensor AND per slot group (tests/snet6_domain.py),
with the k_snet4 + k_gw_* route of the same engine as the yardstick of the group bars and as the witness that the fused kernel is what
ran (the route is chosen silently in nif_api.hip step_chunk; the two routes never agree in bits).

Measured figures: profiles/snet6_domain.md (what these tests print under `pytest -s`)."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import snet6_domain as D
from tests.test_gpu_fuzz_regressions import _one_ulp
from tests.test_gpu_parity import CONFIGS, _make, _make_policy, _per_tensor_rel, _rel, _snet6_shape

pytestmark = pytest.mark.gpu

POLICIES = ["float32", "mixed_bfloat16", "mixed_float16"]
RND = {"mixed_bfloat16": O.bf16_round, "mixed_float16": O.f16_round}


def _f64(*arrs):
    return [None if a is None else a.astype(np.float64) for a in arrs]


def _float32_against_oracle(spec, engine, ws, x, y, sw, what, ref=None, loss_bar=2e-6, flat_bar=3e-5):
    """test 1's assertions on one batch: both routes against the oracle per tensor and per group, the fused route against the unfused
    one per group; returns the two gradients"""
    (l1, g1), (l0, g0) = D.both_routes(engine, x, y, sw)
    if ref is None:
        x64, y64, s64 = _f64(x, y, sw)
        ref = O.loss_and_grad(spec, ws, x64, y64, s64)
    lref, gref = ref
    D.check_tensor_bars(spec, l1, g1, lref, gref, what + " fused", loss_bar, flat_bar)
    D.check_tensor_bars(spec, l0, g0, lref, gref, what + " unfused", loss_bar, flat_bar)
    D.check_group_bars(spec, g1, g0, gref, what)
    return g1, g0


# ---- 1. oracle parity per tensor and per slot group ----------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_oracle_parity_per_tensor_and_slot_group(name, weighted):
    m, model, spec, ws, x, y, sw = D.make(name)
    _float32_against_oracle(spec, m._engine, ws, x, y, sw if weighted else None, name)
    m._engine.close()


# ---- 2. route witness ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", sorted(D.CASES) + ["ms_cfg2_64x4", "ms_cfg5_64x4_si2"])
def test_fused_route_is_what_ran(name, policy):
    """float32: the routes agree to 5e-5 flat (the bar of test_r6_sweep_case_16_snet6_ring_inside_its_allocation); under a policy to
    5e-3 (tools/exp/fuzz_snet6.py: the unfused policy route rounds its dL/da stash rows, the fused one sums exact (hi, lo) rows)"""
    if name in D.CASES:
        m, model, spec, ws, x, y, sw = D.make(name, policy=policy)
    else:
        m, model, spec, ws, x, y, sw = _make(name) if policy == "float32" else _make_policy(name, policy)
        assert _snet6_shape(spec)
    (l1, g1), (l0, g0) = D.both_routes(m._engine, x, y, sw)
    D.check_route_witness(spec, g1, g0, 5e-5 if policy == "float32" else 5e-3, "%s %s" % (name, policy))
    m._engine.close()


# ---- 3. ragged batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 15, 16, 17, 31, 32, 33, 112, 113, 127, 128, 129, 143])
def test_ragged_batches_at_tile_stash_tile_and_round_edges(B):
    """the edges of a 16-point tile, a 32-point stash tile and a 128-point workgroup round on 50 (padded) units, si 2, so 3"""
    name = "s6_50x2_si2_so3"
    m, model, spec, ws, x, y, sw = D.make(name, B=B)
    x64, y64, s64 = _f64(x, y, sw)
    u = model.predict(x)
    ref = O.forward(spec, ws, x64)
    print("B %d: predictions max abs err %.2e" % (B, np.abs(u - ref).max()))
    assert np.abs(u - ref).max() < 1e-5 * max(1.0, np.abs(ref).max())
    assert np.array_equal(u, model.predict(np.concatenate([x, x, x, x]))[:B])
    # the loss of a handful of points to 1e-5, the gradient per tensor with its floor and per group (no flat bar at these sizes)
    _float32_against_oracle(spec, m._engine, ws, x, y, sw, "%s B %d" % (name, B), loss_bar=1e-5, flat_bar=None)
    m._engine.close()


# ---- 4. zero sample weights ----------------------------------------------------------------------------------------------------------
def test_zero_sample_weights_on_a_tile_a_tail_and_scattered_rows():
    """weight exactly 0 on one whole 16-point tile, on the last five rows and on twenty scattered rows; those rows carry y = 1e3, which
    must not reach the loss or any gradient"""
    name = "s6_57x4_si2_so2"
    m, model, spec, ws, x, y, sw = D.make(name)
    B = x.shape[0]
    zero = np.zeros(B, bool)
    zero[32:48] = True
    zero[B - 5:] = True
    rest = np.flatnonzero(~zero)
    zero[np.random.default_rng(4).choice(rest, size=20, replace=False)] = True
    assert zero.sum() == 41
    sw = sw.copy(); y = y.copy()
    sw[zero] = 0.0
    y[zero] = 1e3
    _float32_against_oracle(spec, m._engine, ws, x, y, sw, name + " zero weights")
    m._engine.close()


# ---- 5. several tile rounds per workgroup --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [33189, 78413])
@pytest.mark.parametrize("name", ["s6_49x1_si1_so1", "s6_64x4_si3_so3"])
def test_several_tile_rounds_per_workgroup(name, B):
    """above 32 768 points the grid is capped at 256 workgroups of 8 tiles: 33 189 = 32 768 + 3 * 128 + 2 * 16 + 5 gives some workgroups
    two rounds and some one, with inactive waves and a partial tile; 78 413 = 2 * 32 768 + 100 * 128 + 77.  The loss is a sum over
    points, so 1031 distinct rows drawn B times with the oracle on the distinct rows weighted by their multiplicities is the exact
    reference -- and every distinct point sits at many tile, wave, workgroup and round indices of the launch"""
    Bu = 1031
    m, model, spec, ws, xu, yu, swu = D.make(name, B=Bu)
    idx = np.random.default_rng(5).integers(0, Bu, size=B)
    x, y, sw = xu[idx], yu[idx], swu[idx]
    x64, y64, s64 = _f64(xu, yu, swu)
    ref = O.loss_and_grad(spec, ws, x64, y64, s64 * np.bincount(idx, minlength=Bu), batch_global=B)
    e = m._engine
    what = "%s B %d" % (name, B)
    g1, g0 = _float32_against_oracle(spec, e, ws, x, y, sw, what, ref=ref)
    la, ga = e.loss_and_grad(x, y, sw)
    lb, gb = e.loss_and_grad(x, y, sw)
    assert la == lb and np.array_equal(ga, gb) and np.array_equal(ga, g1)
    D.check_route_witness(spec, g1, g0, 5e-5, what)
    e.close()


# ---- 6. one context, batches of changing size ----------------------------------------------------------------------------------------
def test_one_context_over_batches_of_changing_size():
    """the ring, stash and partial-row buffers of a context grow and are reused: every batch of the sequence gives the bits a fresh
    context gives at that size alone (sizing those buffers by the batch was the bug of test_r6_sweep_case_16_...)"""
    name = "s6_56x3_si3_so2"
    sizes = [2049, 17, 33189, 129, 1]
    m, model, spec, ws, x, y, sw = D.make(name, B=max(sizes))
    for B in sizes:
        got = m._engine.loss_and_grad(x[:B], y[:B], sw[:B])
        mf = D.make(name, B=1)[0]
        want = mf._engine.loss_and_grad(x[:B], y[:B], sw[:B])
        mf._engine.close()
        assert np.all(np.isfinite(want[1]))
        assert got[0] == want[0], (B, got[0], want[0])
        assert np.array_equal(got[1], want[1]), (B, int((got[1] != want[1]).sum()))
    m._engine.close()


# ---- 7. the policy forms k_snet6<4, 1> and <4, 2> ------------------------------------------------------------------------------------
SHALLOW = ["s6_49x1_si1_so1", "s6_64x1_si3_so3", "s6_50x2_si2_so3"]
DEEP = ["s6_63x3_si1_so2", "s6_64x4_si3_so3"]


@pytest.mark.parametrize("policy", POLICIES[1:])
@pytest.mark.parametrize("name", SHALLOW + DEEP)
def test_policy_forms_against_the_emulating_oracle(name, policy):
    """the emulating oracle rounds where the kernel rounds (planes_loss_and_grad(rnd=..., stash_bf16=False): k_snet6's policy forms
    keep no dL/da stash).  Shallow nets: the fixed bars of the policy tests (predictions and loss 5e-4, every tensor 2e-3).  Three
    and four hidden matrices: the emulating oracle's own movement s under one-ulp weight noise (a different set of roundings flips)
    comes close to those bars, so max(bar, 3 s) with the 5e-2 cap, as in test_policy_rounding_flips_on_a_31_point_batch.  Per slot
    group: max(5e-3, 3 s_G) of the group's own norm + the float32 floor"""
    B = max(D.CASES[name][1], 257)
    m, model, spec, ws, x, y, sw = D.make(name, B=B, policy=policy)
    assert m.mixed_policy_name == policy
    x64, y64, s64 = _f64(x, y, sw)
    fn = lambda w: O.planes_loss_and_grad(spec, w, x64, y64, s64, rnd=RND[policy], stash_bf16=False)
    rl, rg, ru = fn(ws)
    rflat = O.flatten(rg)
    gnorm = float(np.linalg.norm(rflat))
    s_u = s_l = 0.0
    s_t = {nm: 0.0 for nm, _ in spec.param_shapes()}
    s_g = {}
    for sd in (7, 8, 9):
        nl, ng, nu = fn(_one_ulp(ws, sd))
        nflat = O.flatten(ng)
        s_u, s_l = max(s_u, _rel(nu, ru)), max(s_l, abs(nl - rl) / abs(rl))
        for nm, v in _per_tensor_rel(spec, nflat, rflat).items():
            s_t[nm] = max(s_t[nm], v)
        for k, (err, ng_, _) in D.group_table(spec, nflat, rflat).items():
            s_g[k] = max(s_g.get(k, 0.0), err / ng_)
    u = model.predict(x)
    (loss, g), (l0, g0) = D.both_routes(m._engine, x, y, sw)
    e_u, e_l, rel = _rel(u, ru), abs(loss - rl) / abs(rl), _per_tensor_rel(spec, g, rflat)
    print("%s %s: predictions %.2e (s %.2e), loss %.2e (s %.2e), worst tensor %.2e (s %.2e)"
          % (name, policy, e_u, s_u, e_l, s_l, max(rel.values()), max(s_t.values())))
    if name in SHALLOW:
        assert e_u < 5e-4 and e_l <= 5e-4, (e_u, e_l)
        assert max(rel.values()) < 2e-3, rel
    else:
        assert e_u < max(5e-4, 3.0 * s_u) and e_u < 5e-2, (e_u, s_u)
        assert e_l < max(5e-4, 3.0 * s_l) and e_l < 5e-2, (e_l, s_l)
        for nm, v in rel.items():
            assert v < max(2e-3, 3.0 * s_t[nm]) and v < 5e-2, (nm, v, s_t[nm])
    table = D.group_table(spec, g, rflat)
    k = max(table, key=lambda k: table[k][0] / table[k][1])
    print("%s %s: worst group err / |ref_G| %.2e %s (s_G %.2e, worst s_G %.2e)"
          % (name, policy, table[k][0] / table[k][1], k, s_g[k], max(s_g.values())))
    for k, (err, ng_, _) in sorted(table.items()):
        assert err <= max(5e-3, 3.0 * s_g[k]) * ng_ + 2.5e-7 * gnorm, (k, err / ng_, s_g[k])
    D.check_route_witness(spec, g, g0, 5e-3, "%s %s" % (name, policy))
    m._engine.close()
