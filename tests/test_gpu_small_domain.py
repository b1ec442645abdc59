"""The one-launch small-batch step k_small (csrc/k_small.hip) over its whole admission domain: the route nif_api.hip loss_grad_core takes
against the restated rule on both sides of every boundary, the corners of the rule (four hidden matrices in either net, latent_dim 4,
four inputs / outputs / parameters, one and five units, no hidden matrix, the largest LDS footprints), the batch edges, every
activation of small_act, the other losses, zero sample weights, batch_global, the regularisers behind the launch and repeatability --
against the fp64 oracle per Keras tensor AND per slot group (tests/small_domain.py), with the tile kernels of the same engine
(small_step 0) as the yardstick of the group bars.

Measured figures: profiles/small_domain.md (what these tests print under `pytest -s`)."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import small_domain as D
from tests.test_gpu_parity import _per_tensor_rel, _rel, _stash_bf16, _stash_ph16

pytestmark = pytest.mark.gpu

PAD = "pad_nif_30x2"


def _f64(*arrs):
    return [None if a is None else a.astype(np.float64) for a in arrs]


# ---- 1. the route is the restated rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.INSIDE + D.OUTSIDE)
def test_first_step_of_a_fresh_context_takes_the_route_of_the_restated_rule(name):
    """inside: one launch on the ShapeNet group and none on the ParameterNet / weight-gradient groups; outside: the tile kernels, at
    their own bars (loss 2e-6, 5e-5 per tensor; mixed_bfloat16: the bars of the policy test against the oracle with the same casts)"""
    m, model, spec, ws, x, y, sw = D.make(name)
    e = m._engine
    (loss, g), counts = D.profiled_step(e, x, y, sw)
    print("%s: %s, launches %s" % (name, D.CASES[name]["side"], {k: v for k, v in counts.items() if v}))
    if name in D.INSIDE:
        assert D.ran_on_k_small(counts), counts
    else:
        assert D.ran_on_tile_kernels(counts) and not D.ran_on_k_small(counts), counts
        x64, y64, s64 = _f64(x, y, sw)
        if D.CASES[name]["policy"] == "float32":
            lref, gref = O.loss_and_grad(spec, ws, x64, y64, s64)
            D.check_tensor_bars(spec, loss, g, lref, O.flatten(gref), name + " tile", D.TILE_BAR)
        else:
            lref, gref, _ = O.planes_loss_and_grad(spec, ws, x64, y64, s64, rnd=O.bf16_round, stash_bf16=_stash_bf16(spec),
                                                   stash_ph16=_stash_ph16(spec))
            D.check_tensor_bars(spec, loss, g, lref, O.flatten(gref), name + " tile", 2e-3, loss_bar=5e-4)
    e.close()


@pytest.mark.parametrize("which", ["act_l2_reg", "act_l1_reg", "fp32_mfma"])
@pytest.mark.parametrize("name", [PAD, "ms_24x2_r4_so1"])
def test_activity_regulariser_and_fp32_mfma_send_an_inside_shape_to_the_tile_kernels(name, which):
    """k_small has no activity-regulariser term and is not the f32-input MFMA path: both must leave it, and still match the oracle
    (activity regulariser: the bars of test_activity_regularisers_match_oracle, loss 1e-5 and 3e-4 per tensor; fp32_mfma: the tile bars)"""
    m, model, spec, ws, x, y, sw = D.make(name)
    e = m._engine
    x64, y64, s64 = _f64(x, y, sw)
    act = None
    if which == "fp32_mfma":
        e.set_option("fp32_mfma", 1)
    else:
        act = (0.0, 3e-3) if which == "act_l2_reg" else (2e-4, 0.0)
        e.set_activity_regularizer(*act)
    (loss, g), counts = D.profiled_step(e, x, y, sw)
    print("%s %s: launches %s" % (name, which, {k: v for k, v in counts.items() if v}))
    assert D.ran_on_tile_kernels(counts) and not D.ran_on_k_small(counts), counts
    lref, gref = O.loss_and_grad(spec, ws, x64, y64, s64, act_reg=act)
    l0 = O.loss_and_grad(spec, ws, x64, y64, s64)[0]
    assert act is None or abs(lref - l0) > 1e-4 * abs(l0)                      # the term is visible
    D.check_tensor_bars(spec, loss, g, lref, O.flatten(gref), "%s %s" % (name, which), D.TILE_BAR if act is None else 3e-4,
                        loss_bar=D.LOSS_BAR if act is None else 1e-5)
    # switched off again, the same context is back on k_small
    if act is None:
        e.set_option("fp32_mfma", 0)
    else:
        e.set_activity_regularizer(0.0, 0.0)
    (l1, g1), counts = D.profiled_step(e, x, y, sw)
    assert D.ran_on_k_small(counts), counts
    D.check_tensor_bars(spec, l1, g1, l0, O.flatten(O.loss_and_grad(spec, ws, x64, y64, s64)[1]), "%s after %s" % (name, which), D.SMALL_BAR)
    e.close()


# ---- 2. oracle parity at the corners -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", D.INSIDE)
def test_oracle_parity_per_tensor_and_slot_group_at_the_corners(name, weighted):
    """every inside case of the table, weighted and unweighted, small_step 1 and 0 on one engine"""
    m, model, spec, ws, x, y, sw = D.make(name)
    D.against_oracle(spec, m._engine, ws, x, y, sw if weighted else None, "%s %s" % (name, "weighted" if weighted else "unweighted"),
                     raised=name in D.RAISED, raised_group=(name, weighted) in D.RAISED_GROUP)
    m._engine.close()


# ---- 3. batch edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 15, 16, 17, 31, 32, 33, 2047, 2048])
def test_batch_edges_of_a_wave_pair_a_workgroup_and_the_rule(B):
    """a wave takes two points, a workgroup 16, the rule 2048: the padded shape (30 of 32 ShapeNet lanes, 20 of 32 ParameterNet lanes)"""
    m, model, spec, ws, x, y, sw = D.make(PAD, B=B)
    e = m._engine
    (_, _), counts = D.profiled_step(e, x, y, sw)
    assert D.ran_on_k_small(counts), counts
    D.against_oracle(spec, e, ws, x, y, sw, "%s B %d" % (PAD, B))
    e.close()


def test_one_context_across_the_largest_batch_the_first_refused_one_and_back():
    """the padded shape again: k_small, the tile kernels at 2049 points, and k_small on the buffers those left; the two 2048-point
    results are the same bits"""
    sizes = [2048, 2049, 1, 2048, 16]
    m, model, spec, ws, x, y, sw = D.make("out_pad_b2049")
    e = m._engine
    got = []
    for B in sizes:
        (loss, g), counts = D.profiled_step(e, x[:B], y[:B], sw[:B])
        assert (D.ran_on_k_small(counts) if B <= 2048 else D.ran_on_tile_kernels(counts) and not D.ran_on_k_small(counts)), (B, counts)
        x64, y64, s64 = _f64(x[:B], y[:B], sw[:B])
        lref, gref = O.loss_and_grad(spec, ws, x64, y64, s64)
        D.check_tensor_bars(spec, loss, g, lref, O.flatten(gref), "sequence B %d" % B, D.SMALL_BAR if B <= 2048 else D.TILE_BAR)
        got.append((loss, g))
    assert got[0][0] == got[3][0] and np.array_equal(got[0][1], got[3][1]), int((got[0][1] != got[3][1]).sum())
    e.close()


# ---- 4. every activation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["nif", "ms"])
@pytest.mark.parametrize("act", D.ACTS)
def test_every_activation_of_the_run_time_switch(act, net):
    """net nif: the activation of BOTH nets of the padded class-NIF shape (skip connections; lanes beyond the widths must stay zero
    behind activations that do not map 0 to 0); net ms: p_act of the MLP_SimpleShortCut ParameterNet of a plain NIFMultiScale.  The
    draws keep every pre-activation 1e-5 away from a derivative kink (tests/test_small_domain.py)"""
    name = "act_%s_%s" % (net, act)
    m, model, spec, ws, x, y, sw = D.make(name)
    e = m._engine
    (_, _), counts = D.profiled_step(e, x, y, sw)
    assert D.ran_on_k_small(counts), counts
    D.against_oracle(spec, e, ws, x, y, sw, name, raised=name in D.RAISED, raised_group=(name, True) in D.RAISED_GROUP)
    e.close()


# ---- 5. the other losses -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["mae", "huber", "log_cosh"])
def test_other_losses_at_three_outputs_and_two_latents(loss):
    """targets x 3: |e| on both sides of Huber's delta; no |e| below 1e-5 (tests/test_small_domain.py), so mae's sign(e) is the
    oracle's everywhere and mae takes the bars of the others"""
    name = "loss_nif_30x2_so3_r2"
    m, model, spec, ws, x, y, sw = D.make(name)
    e = m._engine
    y = D.times3(y)
    e.set_loss(loss)
    (_, _), counts = D.profiled_step(e, x, y, sw)
    assert D.ran_on_k_small(counts), counts
    D.against_oracle(spec, e, ws, x, y, sw, "%s %s" % (name, loss), loss=loss)
    e.close()


# ---- 6. zero sample weights --------------------------------------------------------------------------------------------------------------
def test_zero_sample_weights_on_a_workgroup_on_wave_halves_and_on_the_tail():
    """weight exactly 0 on one whole 16-point workgroup, on one point of four wave pairs and on the last seven rows; those rows carry
    y = 1e3, which must not reach the loss or any gradient.  All weights 0: loss 0.0 and a gradient of zeros"""
    m, model, spec, ws, x, y, sw = D.make(PAD)
    e = m._engine
    B = x.shape[0]
    zero = np.zeros(B, bool)
    zero[32:48] = True
    zero[[64, 67, 70, 73]] = True
    zero[B - 7:] = True
    sw = sw.copy(); y = y.copy()
    sw[zero] = 0.0
    y[zero] = 1e3
    D.against_oracle(spec, e, ws, x, y, sw, PAD + " zero weights")
    (l1, g1), (l0, g0) = D.both_routes(e, x, y, np.zeros(B, np.float32))
    print("all weights 0: k_small loss %r, %d nonzero entries; tile loss %r, %d nonzero entries"
          % (l1, int((g1 != 0).sum()), l0, int((g0 != 0).sum())))
    assert l1 == 0.0 and np.all(np.isfinite(g1)) and np.all(g1 == 0.0)
    assert l0 == 0.0 and np.all(np.isfinite(g0)) and np.all(g0 == 0.0)
    e.close()


# ---- 7. batch_global ---------------------------------------------------------------------------------------------------------------------
def test_batch_global_scales_loss_and_gradient_by_an_exact_power_of_two():
    """a 512-point shard of a 2048-point batch: inv_bg = 2^-11 instead of 2^-9, the same products and the same sum order, so the loss
    and every gradient entry of normal magnitude are 0.25 x the bg = 512 run bit for bit; and the oracle's with batch_global"""
    B = 512
    m, model, spec, ws, x, y, sw = D.make(PAD, B=B)
    e = m._engine
    d_x, d_y, d_s = e.alloc(x.size), e.alloc(y.size), e.alloc(sw.size)
    d_x.upload(x); d_y.upload(y); d_s.upload(sw)
    res = {}
    for bg in (512, 2048):
        _, counts = D.profiled(e, lambda: e.loss_grad_dev(d_x.at(0), d_y.at(0), d_s.at(0), B, bg))
        assert D.ran_on_k_small(counts), counts
        res[bg] = e.grad_read()
        x64, y64, s64 = _f64(x, y, sw)
        lref, gref = O.loss_and_grad(spec, ws, x64, y64, s64, batch_global=bg)
        D.check_tensor_bars(spec, res[bg][0], res[bg][1], lref, O.flatten(gref), "%s B 512 bg %d" % (PAD, bg), D.SMALL_BAR)
    (la, ga), (lb, gb) = res[512], res[2048]
    normal = np.abs(ga) >= 1e-20
    print("bg 2048 vs 0.25 x bg 512: loss %r vs %r, %d of %d entries of normal magnitude, %d differ"
          % (lb, 0.25 * la, int(normal.sum()), ga.size, int((gb[normal] != np.float32(0.25) * ga[normal]).sum())))
    assert normal.sum() > 0.99 * ga.size
    assert np.float32(lb) == np.float32(0.25) * np.float32(la)
    assert np.array_equal(gb[normal], np.float32(0.25) * ga[normal])
    assert np.all(np.abs(gb[~normal]) <= 1e-20)
    e.close()


# ---- 8. the regularisers behind the launch -----------------------------------------------------------------------------------------------
def test_latent_jacobian_regulariser_behind_the_small_step():
    """jac_reg_pass adds to the gradient k_small's row reduction left (which is then not deferred): total = the oracle's step + the
    oracle's regulariser term, at the bars of test_jac_reg_matches_oracle"""
    l1 = 0.05
    m, model, spec, ws, x, y, sw = D.make(PAD)
    e = m._engine
    x64, y64, s64 = _f64(x, y, sw)
    e.set_jac_regularizer(l1)
    (loss, g), counts = D.profiled_step(e, x, y, sw)
    print("jac_reg: launches %s" % {k: v for k, v in counts.items() if v})
    assert counts["snet"] == 1 and counts["gw"] == 0, counts                      # the main step stayed on k_small
    l0, g0 = O.loss_and_grad(spec, ws, x64, y64, s64)
    lj, gj = O.jac_reg_loss_and_grad(spec, ws, x64[:, :spec.pi], l1)
    assert lj > 1e-6 * l0
    ref = O.flatten(g0) + O.flatten(gj)
    rel = _per_tensor_rel(spec, g, ref)
    print("jac_reg: loss %.9e ref %.9e + %.9e (%.1e), worst tensor %.2e" % (loss, l0, lj, abs(loss - (l0 + lj)) / (l0 + lj), max(rel.values())))
    assert abs(loss - (l0 + lj)) <= 1e-5 * (l0 + lj), (loss, l0, lj)
    assert max(rel.values()) < 3e-4, rel
    # the regulariser's own part, isolated: gradient(with) - gradient(without) against the oracle's term
    e.set_jac_regularizer(0.0)
    (lw, gw), counts = D.profiled_step(e, x, y, sw)
    assert D.ran_on_k_small(counts), counts
    dj = g.astype(np.float64) - gw
    npn = sum(int(np.prod(s_)) for nm, s_ in spec.param_shapes() if nm.startswith("pnet_") and not nm.startswith("pnet_last"))
    print("jac_reg: own part %.2e, own loss %.2e" % (_rel(dj[:npn], O.flatten(gj)[:npn]), abs((loss - lw) - lj) / lj))
    assert _rel(dj[:npn], O.flatten(gj)[:npn]) < 2e-3 and abs((loss - lw) - lj) < 2e-4 * lj + 1e-7 * l0
    assert np.array_equal(g[npn:], gw[npn:])              # the hyper layer lies downstream of the latent: untouched
    e.close()


@pytest.mark.parametrize("reg", ["l2", "l1"])
def test_weight_regulariser_behind_the_small_step(reg):
    """set_regularizer over every variable: Keras adds l2 sum w^2 (l1 sum |w|) to the loss and its gradient to the gradient.  With one
    set, the row reduction of the small step is not deferred.  The term is one rounding per entry: k_small's per-tensor bar holds; the
    loss at the 1e-5 of test_weight_regularisers_l2_and_l1"""
    val = 1e-3 if reg == "l2" else 2e-4
    m, model, spec, ws, x, y, sw = D.make(PAD)
    e = m._engine
    x64, y64, s64 = _f64(x, y, sw)
    lref, gref = O.loss_and_grad(spec, ws, x64, y64, s64)
    th, gref = O.flatten(ws), O.flatten(gref)
    l0 = lref
    if reg == "l2":
        lref += val * (th ** 2).sum(); gref = gref + 2 * val * th
        e.set_regularizer(0.0, val, 0, spec.n_params())
    else:
        lref += val * np.abs(th).sum(); gref = gref + val * np.sign(th)
        e.set_regularizer(val, 0.0, 0, spec.n_params())
    assert lref - l0 > 1e-3 * l0
    d_x, d_y, d_s = e.alloc(x.size), e.alloc(y.size), e.alloc(sw.size)
    d_x.upload(x); d_y.upload(y); d_s.upload(sw)
    B = x.shape[0]
    _, counts = D.profiled(e, lambda: e.loss_grad_dev(d_x.at(0), d_y.at(0), d_s.at(0), B, B))
    assert D.ran_on_k_small(counts), counts
    loss, g = e.grad_read()
    D.check_tensor_bars(spec, loss, g, lref, gref, "%s %s grad_read" % (PAD, reg), D.SMALL_BAR, loss_bar=1e-5)
    # without the profiler (the reduction could be deferred, and is not) and through the host entry: the same bits
    e.loss_grad_dev(d_x.at(0), d_y.at(0), d_s.at(0), B, B)
    loss2, g2 = e.grad_read()
    loss3, g3 = e.loss_and_grad(x, y, sw)
    assert loss2 == loss and np.array_equal(g2, g) and loss3 == loss and np.array_equal(g3, g)
    # a second read does not add the term twice
    loss4, g4 = e.grad_read()
    assert loss4 == loss and np.array_equal(g4, g)
    e.close()


# ---- 9. repeatability --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [PAD, "lds_ms_nh4_lst1_r4_siren"])
def test_the_same_call_gives_the_same_bits(name):
    """twice in a row, after a call on the tile kernels, and after a call with another batch size"""
    m, model, spec, ws, x, y, sw = D.make(name)
    e = m._engine
    a = e.loss_and_grad(x, y, sw)
    b = e.loss_and_grad(x, y, sw)
    e.set_option("small_step", 0)
    t = e.loss_and_grad(x, y, sw)
    e.set_option("small_step", 1)
    c = e.loss_and_grad(x, y, sw)
    e.loss_and_grad(x[:100], y[:100], sw[:100])
    d = e.loss_and_grad(x, y, sw)
    print("%s: %d of %d entries differ in bits between k_small and the tile kernels" % (name, int((a[1] != t[1]).sum()), a[1].size))
    assert np.all(np.isfinite(a[1])) and np.any(a[1] != t[1])      # (the tile route is another computation: it did run in between)
    for nm, o in (("twice", b), ("after small_step 0", c), ("after another batch size", d)):
        assert o[0] == a[0] and np.array_equal(o[1], a[1]), (name, nm, int((o[1] != a[1]).sum()))
    e.close()
