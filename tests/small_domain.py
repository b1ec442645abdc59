"""Cases, admission restatement, slot groups and bars of tests/test_small_domain.py (CPU) and tests/test_gpu_small_domain.py: the
admission domain of the one-launch small-batch step k_small (csrc/k_small.hip small_supported, chosen silently in nif_api.hip
loss_grad_core) -- class NIF with any Keras activation, plain-SIREN NIFMultiScale, MLP_SimpleShortCut / SIREN ParameterNets, 1..32
units, 0..4 hidden matrices in either net, latent_dim 1..4, 1..4 inputs / outputs / parameters, 1..2048 points, at most 128 KB of
dynamic LDS, float32.  Every check prints its figures before it asserts; profiles/small_domain.md holds those of an MI355X run under
`pytest -s`.

Why groups: every ShapeNet weight gradient lands in pnet_last_w [r, po] and pnet_last_b [po], but the kernel forms the first-layer row
of each coordinate, each hidden matrix, the last-layer column of each output and the biases from separate descriptors (small_desc), once
per latent row.  A per-tensor bar cannot see an error in one column of one plane; a bar relative to the group's own norm can.

nlayers = 0: the Python surface (nif_amd/spec.py), the C entry (nif_create refuses only negative counts) and the oracle all take a net
without hidden matrices, and small_supported admits nh = 0 and lst = 0 -- one inside case each (nif_L0, ms_lst0)."""
import numpy as np

from oracle import nif_oracle as O
from tests.test_gpu_parity import _cfg, _make, _make_policy, _per_tensor_rel

# ---- the admission rule, restated (csrc/k_small.hip small_layout / small_ntasks / small_supported, nif_internal.h NIF_SMALL_MAX_B) -----
SMALL_T, SMALL_W, SMALL_RS = 16, 32, 33
SMALL_MAX_B, SMALL_MAXH, SMALL_MAXR, SMALL_MAXT = 2048, 4, 4, 80
SMALL_LDS_MAX = 128 * 1024


def _layout_floats(pi, lst, r, si, nh):
    """small_layout(...).total: (r + 1) ShapeNet planes, the ParameterNet image, 16 per-point tapes, 16 words of loss partials"""
    ps = si * SMALL_W + nh * SMALL_W * SMALL_RS + SMALL_W * 4 + SMALL_W + nh * SMALL_W + 4
    pw = pi * SMALL_W + SMALL_W + lst * SMALL_W * SMALL_RS + lst * SMALL_W + SMALL_W * 4 + 4
    tp = 8 + 2 * (lst + 1) * SMALL_W + 4 + 4 + 2 * (nh + 1) * SMALL_W + 4
    if tp % 64 == 0:
        tp += 4
    return (r + 1) * ps + pw + SMALL_T * tp + 16


def small_lds_bytes(spec):
    """dynamic LDS of the k_small launch of this shape: it does not depend on the widths"""
    return 4 * _layout_floats(spec.pi, spec.lst, spec.r, spec.si, spec.n_hidden_mats)


def small_admits(spec, B, policy="float32"):
    """does loss_grad_core send the plain step of this shape and batch to k_small (no activity regulariser, fp32_mfma off)?"""
    if spec.kind == O.KIND_LL or spec.s_res or spec.p_res or policy != "float32":
        return False
    nh, lst = spec.n_hidden_mats, spec.lst
    if spec.n > 32 or spec.nst > 32 or nh > SMALL_MAXH or lst > SMALL_MAXH or not 1 <= spec.r <= SMALL_MAXR:
        return False
    if not (1 <= spec.si <= 4 and spec.so <= 4 and 1 <= spec.pi <= 4 and nh >= 0 and lst >= 0):
        return False
    if spec.pi + spec.si > 8 or 4 + 2 * lst + (spec.r + 1) * (4 + 2 * nh) > SMALL_MAXT:
        return False
    if small_lds_bytes(spec) > SMALL_LDS_MAX:
        return False
    return 1 <= B <= SMALL_MAX_B


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
ACTS = ["linear", "swish", "tanh", "relu", "sigmoid", "elu", "softplus", "gelu", "selu", "softsign", "exponential", "hard_sigmoid"]
KINKS = {"relu": (0.0,), "selu": (0.0,), "hard_sigmoid": (-2.5, 2.5)}      # where an activation's derivative jumps
MARGIN = 1e-5        # about a hundred fp32 roundings of an O(1) value: no float32 pre-activation lands on the other side of a kink


def _c(side, kind, n, L, nst, lst, r, si, so, pi, B, seed=0, scale=1.0, policy="float32", **kw):
    return {"side": side, "cfg": _cfg(kind, n, L, nst, lst, r, si, so, pi, **kw), "B": B, "seed": seed, "scale": scale, "policy": policy}


# the padded class-NIF shape of the batch-edge, activation, zero-weight, batch_global, regulariser and repeatability tests
def _pad(act="tanh", B=257, seed=0, scale=1.0, so=2):
    return _c("inside", "NIF", 30, 2, 20, 1, 2, 2, so, 2, B, seed=seed, scale=scale, act=act)


# seeds at which every float64 pre-activation keeps MARGIN from the kinks (test_small_domain.py asserts it).  Some 33 000 pre-activations
# of both nets at 257 points: about one seed in ten does for relu / selu; hard_sigmoid's +-2.5 is out of reach of these draws
ACT_SEEDS = {("nif", "relu"): 5, ("nif", "selu"): 4, ("ms", "relu"): 5, ("ms", "selu"): 10}

CASES = {
    # kind, units, hidden matrices, ParameterNet units, layers, latent_dim, si, so, pi, batch
    # the three largest footprints the rule admits (nh, lst, r at si = pi = 4): 128 416, 127 904 and 126 736 bytes
    "lds_ms_nh4_lst1_r4_siren": _c("inside", "NIFMultiScale", 29, 4, 27, 1, 4, 4, 2, 4, 293),
    "lds_ms_nh3_lst4_r4_swish": _c("inside", "NIFMultiScale", 32, 3, 32, 4, 4, 4, 3, 4, 203, p_act="swish"),
    "lds_nif_nh4_lst3_r3_tanh": _c("inside", "NIF", 30, 4, 31, 3, 3, 4, 4, 4, 131, act="tanh"),
    # ... and the inside neighbours of the two refusals below
    "lds_ms_nh4_lst1_r4_io1": _c("inside", "NIFMultiScale", 32, 4, 32, 1, 4, 1, 1, 1, 35),
    "lds_ms_nh4_lst3_r3_io1": _c("inside", "NIFMultiScale", 32, 4, 32, 3, 3, 1, 1, 1, 35),
    # every 4-wide image and the 8-word t_x row filled to the last word, on odd widths
    "nif_31x2_nst17_r4_io4": _c("inside", "NIF", 31, 2, 17, 2, 4, 4, 4, 4, 77),
    "ms_24x2_r4_so1": _c("inside", "NIFMultiScale", 24, 2, 20, 1, 4, 2, 1, 1, 45),
    "nif_1x1_nst1_b16": _c("inside", "NIF", 1, 1, 1, 1, 1, 1, 1, 1, 16),
    "nif_5x2_nst5": _c("inside", "NIF", 5, 2, 5, 2, 2, 2, 2, 1, 19),
    "nif_L0": _c("inside", "NIF", 12, 0, 10, 2, 2, 2, 2, 1, 21),
    "ms_lst0": _c("inside", "NIFMultiScale", 16, 2, 12, 0, 2, 1, 2, 2, 21),
    # the shapes the outside neighbours are one step away from
    "base_nif_32x2_r4_io4": _c("inside", "NIF", 32, 2, 32, 2, 4, 4, 4, 4, 49),
    "base_ms_32x4_lst1": _c("inside", "NIFMultiScale", 32, 4, 32, 1, 1, 1, 1, 1, 37),
    "base_ms_32x2_lst4": _c("inside", "NIFMultiScale", 32, 2, 32, 4, 1, 1, 1, 1, 37),
    "pad_nif_30x2": _pad(),
    "loss_nif_30x2_so3_r2": _pad(so=3),

    # outside: each one thing away from an inside case
    "out_33_units": _c("outside", "NIF", 33, 2, 32, 2, 4, 4, 4, 4, 49),
    "out_nst_33": _c("outside", "NIF", 32, 2, 33, 2, 4, 4, 4, 4, 49),
    "out_r5": _c("outside", "NIF", 32, 2, 32, 2, 5, 4, 4, 4, 49),
    "out_si5": _c("outside", "NIF", 32, 2, 32, 2, 4, 5, 4, 4, 49),
    "out_so5": _c("outside", "NIF", 32, 2, 32, 2, 4, 4, 5, 4, 49),
    "out_pi5": _c("outside", "NIF", 32, 2, 32, 2, 4, 4, 4, 5, 49),
    "out_b2049": _c("outside", "NIF", 32, 2, 32, 2, 4, 4, 4, 4, 2049),
    "out_pad_b2049": dict(_pad(B=2049), side="outside"),
    "out_mixed_bfloat16": _c("outside", "NIF", 32, 2, 32, 2, 4, 4, 4, 4, 49, policy="mixed_bfloat16"),
    "out_5_hidden_matrices": _c("outside", "NIFMultiScale", 32, 5, 32, 1, 1, 1, 1, 1, 37),
    "out_lst5": _c("outside", "NIFMultiScale", 32, 2, 32, 5, 1, 1, 1, 1, 37),
    "out_s_resblock": _c("outside", "NIFMultiScale", 32, 2, 32, 4, 1, 1, 1, 1, 37, s_res=True),
    "out_p_resblock": _c("outside", "NIFMultiScale", 32, 2, 32, 4, 1, 1, 1, 1, 37, p_res=True),
    "out_last_layer_class": _c("outside", "LL", 32, 2, 32, 4, 1, 1, 1, 1, 37),
    "out_lds_nh4_lst2_r4": _c("outside", "NIFMultiScale", 32, 4, 32, 2, 4, 1, 1, 1, 35),      # 134 560 bytes
    "out_lds_nh4_lst4_r3": _c("outside", "NIFMultiScale", 32, 4, 32, 4, 3, 1, 1, 1, 35),      # 133 264 bytes
}
# every activation through small_act: as the activation of both nets of the padded class-NIF shape, and as p_act of a plain NIFMultiScale
# 24 x 2 with a 20-unit MLP_SimpleShortCut ParameterNet.  exponential: exp(exp(.)) through skip connections -- a tamer draw, as in
# test_remaining_keras_activations
for _a in ACTS:
    _s = 0.3 if _a == "exponential" else 1.0
    CASES["act_nif_" + _a] = _pad(act=_a, seed=ACT_SEEDS.get(("nif", _a), 0), scale=_s)
    CASES["act_ms_" + _a] = _c("inside", "NIFMultiScale", 24, 2, 20, 2, 2, 2, 1, 2, 257, seed=ACT_SEEDS.get(("ms", _a), 0), scale=_s, p_act=_a)
INSIDE = sorted(k for k, c in CASES.items() if c["side"] == "inside")
OUTSIDE = sorted(k for k, c in CASES.items() if c["side"] == "outside")
SLOT_TENSORS = ("pnet_last_w", "pnet_last_b")


def spec_of(name):
    kind, cs, cp = CASES[name]["cfg"]
    return O.Spec(kind, cs, cp)


def check_side(name, B=None):
    c = CASES[name]
    got = small_admits(spec_of(name), c["B"] if B is None else B, c["policy"])
    assert got == (c["side"] == "inside"), (name, c["side"], got)


def reference_inputs(name, B=None):
    """(spec, ws64, x, y, sw) of a case without an engine: the draws of tests.test_gpu_parity._make / _make_policy restated (make()
    asserts that they are the same arrays), so that the conditions test_small_domain.py checks hold for what the GPU tests run"""
    c = CASES[name]
    spec = spec_of(name)
    B = c["B"] if B is None else B
    rng = np.random.default_rng(c["seed"])
    ws = O.init_weights(spec, rng, dtype=np.float32)
    names = [nm for nm, _ in spec.param_shapes()]
    i = names.index("pnet_last_w")
    if spec.kind == O.KIND_MS:
        ws[i] = (ws[i] * (2.0 if c["policy"] == "float32" else 1.0)).astype(np.float32)
    if spec.kind == O.KIND_LL and c["policy"] == "float32":
        ws[i] = (ws[i] * 30.0).astype(np.float32)
    x = rng.uniform(-1, 1, size=(B, spec.pi + spec.si)).astype(np.float32)
    y = rng.uniform(-1, 1, size=(B, spec.so)).astype(np.float32)
    sw = rng.uniform(0.5, 1.5, size=(B,)).astype(np.float32)
    if c["scale"] != 1.0:
        ws = [(w.astype(np.float64) * c["scale"]).astype(np.float32) for w in ws]
    return spec, [w.astype(np.float64) for w in ws], x, y, sw


def times3(y):
    """the targets of the loss tests: |prediction - target| on both sides of Huber's delta"""
    return (3.0 * y).astype(np.float32)


def make(name, B=None):
    """engine + oracle inputs of a case, as tests.test_gpu_parity._make (float32) or _make_policy; the case is asserted to sit on its
    labelled side of k_small's rule, so that a typo in the table cannot move it across the boundary"""
    c = CASES[name]
    B = c["B"] if B is None else B
    check_side(name, B)
    key = (c["cfg"], B)
    m, model, spec, ws, x, y, sw = _make(key, seed=c["seed"]) if c["policy"] == "float32" else _make_policy(key, c["policy"])
    if c["scale"] != 1.0:
        ws32 = [(w * c["scale"]).astype(np.float32) for w in ws]
        model.set_weights(ws32)
        ws = [w.astype(np.float64) for w in ws32]
    _, rws, rx, ry, rsw = reference_inputs(name, B)
    assert all(np.array_equal(a, b) for a, b in zip(ws, rws)) and np.array_equal(x, rx) and np.array_equal(y, ry) and np.array_equal(sw, rsw), name
    return m, model, spec, ws, x, y, sw


# ---- the oracle's pre-activations (the kink condition) ------------------------------------------------------------------------------------
def preactivations(spec, ws, inputs):
    """{"pnet": [a of the first layer, a of every hidden layer], "snet": [...]}: the float64 oracle's pre-activations of both nets"""
    assert spec.kind in (O.KIND_NIF, O.KIND_MS) and not spec.s_res and not spec.p_res
    inputs = np.asarray(inputs, np.float64)
    pout, _, (ptape, _) = O.pnet_forward(spec, ws, inputs[:, :spec.pi], keep=True)
    _, stape = O.shapenet_given_w(spec, inputs[:, spec.pi:spec.pi + spec.si], pout, keep=True)
    out = {"pnet": [rec[2] for rec in ptape], "snet": [rec[1] for rec in stape["acts"]]}
    assert len(out["pnet"]) == spec.lst + 1 and len(out["snet"]) == spec.n_hidden_mats + 1
    return out


def kink_margin(spec, ws, inputs):
    """the smallest distance of a pre-activation of either net from a point where that net's activation has a derivative jump (inf: none)"""
    pre = preactivations(spec, ws, inputs)
    worst = np.inf
    for net, act in (("pnet", "sine" if spec.p_siren else spec.p_act), ("snet", spec.s_act)):
        for k in KINKS.get(act, ()):
            worst = min([worst] + [float(np.abs(a - k).min()) for a in pre[net]])
    return worst


# ---- slot groups ----------------------------------------------------------------------------------------------------------------------------
def tensor_offsets(spec):
    """name -> (offset, size) of every Keras tensor in the flat gradient"""
    out, off = {}, 0
    for nm, shp in spec.param_shapes():
        k = int(np.prod(shp))
        out[nm] = (off, k)
        off += k
    return out


def slot_groups(spec):
    """the po axis of pnet_output split where the kernel's descriptors split it: [(name, indices)] -- one first-layer row per coordinate,
    one group per hidden matrix, one last-layer column per output (stride so), the first bias, one group per hidden bias, the last bias"""
    sl, n, si, so = spec.slices(), spec.n, spec.si, spec.so
    groups = []
    a, b = sl["w1"]
    groups += [("w1[%d]" % c, np.arange(a + c * n, a + (c + 1) * n)) for c in range(si)]
    groups += [("wh%d" % j, np.arange(a, b)) for j, (a, b) in enumerate(sl["wh"])]
    a, b = sl["wl"]
    groups += [("wl[:,%d]" % o, np.arange(a + o, b, so)) for o in range(so)]
    groups.append(("b1", np.arange(*sl["b1"])))
    groups += [("bh%d" % j, np.arange(a, b)) for j, (a, b) in enumerate(sl["bh"])]
    groups.append(("bl", np.arange(*sl["bl"])))
    every = np.concatenate([idx for _, idx in groups])
    assert np.array_equal(np.sort(every), np.arange(spec.po)) and len(groups) == si + so + 2 * spec.n_hidden_mats + 2
    return groups


def slot_rows(spec):
    """[(label, offset in the flat gradient)] of the r + 1 rows of po entries: pnet_last_w is [r, po], one set of groups per latent row"""
    offs = tensor_offsets(spec)
    assert offs["pnet_last_w"][1] == spec.r * spec.po and offs["pnet_last_b"][1] == spec.po
    return [("pnet_last_w[%d]" % k, offs["pnet_last_w"][0] + k * spec.po) for k in range(spec.r)] + [("pnet_last_b", offs["pnet_last_b"][0])]


def group_table(spec, g, gref):
    """{(row, group): (|g - ref| over the group, |ref| over the group)}; g, gref flat"""
    g, gref = np.asarray(g, np.float64), np.asarray(gref, np.float64)
    out, groups = {}, slot_groups(spec)
    for label, off in slot_rows(spec):
        a, b = g[off:off + spec.po], gref[off:off + spec.po]
        for nm, idx in groups:
            out[(label, nm)] = (float(np.linalg.norm(a[idx] - b[idx])), float(np.linalg.norm(b[idx])))
    assert len(out) == (spec.r + 1) * len(groups)
    return out


# ---- the two routes and the bars -----------------------------------------------------------------------------------------------------------
LOSS_BAR, SMALL_BAR, TILE_BAR, ROUTES_BAR, GROUP_FLOOR = 2e-6, 1e-5, 5e-5, 3e-5, 1e-5
# a raised bar of a named case: {name: reason}.  k_small's per-tensor bar of that case alone becomes max(1e-5, 3 x the tile route's error on
# the same tensor of the same batch); the floor (1e-6 of the whole gradient's norm) stays.  Figures: profiles/small_domain.md
RAISED = {
    "act_ms_softplus": "rounding, not a defect: the shortcut ParameterNet h + softplus(.) adds log 2 or more per layer, the latent grows and the "
                       "hidden sine arguments reach 13 (3.6 under swish); every tensor behind the latent then carries the SAME relative error "
                       "(1.3e-5: that of dL/dz), spread over its entries, 1e-6 with one hidden matrix less, and the tile route sits at "
                       "3.6e-5 .. 4.9e-5 on those tensors of the same batch.  k_small's softplus itself is at 1e-7 on the class-NIF shape",
}
# ... and a raised GROUP bar of a named (case, weighted) draw: 3 x the tile route's error on the group + 1e-5 of the group's norm + the
# floor of the per-tensor bars, 1e-6 of the whole gradient's norm
RAISED_GROUP = {
    ("act_ms_sigmoid", False): "rounding, not a defect: with so = 1 the group bl of a row is ONE entry, sum_b dL/du_b zt_k over 257 points, and in the "
                      "unweighted draw it cancels 365-fold (4.1e-3 of sum |terms| = 1.5; the whole gradient's norm is 48).  k_small's error "
                      "there is 5.9e-7 = 4e-7 of sum |terms| (six float32 roundings), the tile route's 1.0e-7; the weighted draw of the same "
                      "case is inside the bar (0.91), hard_sigmoid has its worst group in the same place (0.59), and where the sine "
                      "arguments are small (the other nine activations: 3.6 instead of 10) k_small uses at most 0.19 of the group bar",
}


def both_routes(engine, x, y, sw):
    """the same batch through k_small (small_step 1) and through the tile kernels (small_step 0) on one engine: ((loss, g), (loss, g))"""
    engine.set_option("small_step", 1)
    small = engine.loss_and_grad(x, y, sw)
    engine.set_option("small_step", 0)
    try:
        tile = engine.loss_and_grad(x, y, sw)
    finally:
        engine.set_option("small_step", 1)
    return small, tile


def profiled(engine, call):
    """call() under the profiler: (its result, {group: launches})"""
    engine.profile_enable(True)
    engine.profile_read(reset=True)
    try:
        out = call()
        prof = engine.profile_read(reset=True)
    finally:
        engine.profile_enable(False)
    return out, {k: v[1] for k, v in prof.items()}


def profiled_step(engine, x, y, sw):
    """one loss_and_grad under the profiler: ((loss, g), {group: launches})"""
    return profiled(engine, lambda: engine.loss_and_grad(x, y, sw))


def ran_on_k_small(counts):
    """k_small's launch is booked on the ShapeNet group and NOTHING on the ParameterNet / weight-gradient groups"""
    return counts["snet"] == 1 and counts["pnet_fwd"] == 0 and counts["pnet_bwd"] == 0 and counts["gw"] == 0


def ran_on_tile_kernels(counts):
    return counts["snet"] >= 1 and counts["pnet_fwd"] + counts["pnet_bwd"] + counts["gw"] >= 1


def check_tensor_bars(spec, loss, g, lref, gref_flat, what, bar, loss_bar=LOSS_BAR, yardstick=None):
    """loss to loss_bar of |ref|, every Keras tensor to `bar` of max(its norm, 1e-6 of the whole gradient's) (_per_tensor_rel).
    yardstick (a RAISED case): the tile route's figures of the same batch -- the tensor's bar is max(bar, 3 x the tile route's)"""
    assert np.isfinite(loss) and np.all(np.isfinite(g)), what
    el = abs(loss - lref) / abs(lref)
    rel = _per_tensor_rel(spec, np.asarray(g), gref_flat)
    bars = {nm: bar if yardstick is None else max(bar, 3.0 * yardstick[nm]) for nm in rel}
    k = max(rel, key=lambda nm: rel[nm] / bars[nm])
    print("%s: loss %.9e ref %.9e err %.1e (%.2f of the bar); worst tensor %s %.2e (%.2f of the bar%s)"
          % (what, loss, lref, el, el / loss_bar, k, rel[k], rel[k] / bars[k], "" if yardstick is None else " %.2e, RAISED" % bars[k]))
    assert el <= loss_bar, (what, loss, lref)
    assert rel[k] < bars[k], (what, rel, bars)
    return rel


def check_group_bars(spec, g_small, g_tile, gref_flat, what, raised=False):
    """per slot group of every latent row: k_small's error <= 3 x the tile route's error on that group + 1e-5 of the group's OWN norm
    (the tile route sums three bf16 (hi, lo) products per pair in another order: the yardstick, as in tests/snet6_domain.py).
    raised (a RAISED_GROUP case): + 1e-6 of the whole gradient's norm"""
    ts, tt = group_table(spec, g_small, gref_flat), group_table(spec, g_tile, gref_flat)
    floor = 1e-6 * float(np.linalg.norm(gref_flat)) if raised else 0.0
    bars = {k: 3.0 * tt[k][0] + GROUP_FLOOR * ts[k][1] + floor for k in ts}
    share = {k: ts[k][0] / max(bars[k], 1e-300) for k in ts}
    ks = max(ts, key=lambda k: ts[k][0] / max(ts[k][1], 1e-300))
    kt = max(tt, key=lambda k: tt[k][0] / max(tt[k][1], 1e-300))
    kr = max(share, key=share.get)
    print("%s: worst group err / |ref_G|: k_small %.2e (%s %s), tile %.2e (%s %s); share of the group bar 3 tile + 1e-5 |ref_G|%s used %.2f (%s %s)"
          % ((what, ts[ks][0] / max(ts[ks][1], 1e-300)) + ks + (tt[kt][0] / max(tt[kt][1], 1e-300),) + kt
             + (" + %.1e, RAISED" % floor if raised else "", share[kr]) + kr))
    for k in sorted(ts):
        assert ts[k][0] <= bars[k], (what, k, ts[k], tt[k], floor)
    return share[kr]


def against_oracle(spec, engine, ws, x, y, sw, what, loss="mse", raised=False, raised_group=False):
    """both routes of one batch against the fp64 oracle per Keras tensor, k_small per slot group with the tile route as the yardstick,
    and the routes against each other (3e-5 flat); returns ((loss, g) of k_small, (loss, g) of the tile route)"""
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)      # noqa: E731
    lref, gref = O.loss_and_grad(spec, ws, f64(x), f64(y), f64(sw), loss=loss)
    gref = O.flatten(gref)
    (l1, g1), (l0, g0) = both_routes(engine, x, y, sw)
    rel0 = check_tensor_bars(spec, l0, g0, lref, gref, what + " tile", TILE_BAR)
    check_tensor_bars(spec, l1, g1, lref, gref, what + " k_small", SMALL_BAR, yardstick=rel0 if raised else None)
    check_group_bars(spec, g1, g0, gref, what, raised=raised_group)
    d = float(np.linalg.norm(g1.astype(np.float64) - g0) / np.linalg.norm(g0.astype(np.float64)))
    print("%s: flat distance between the routes %.2e (%.2f of the bar)" % (what, d, d / ROUTES_BAR))
    assert d < ROUTES_BAR, (what, d)
    return (l1, g1), (l0, g0)
