"""Cases, slot groups and bars of tests/test_gpu_snet6_domain.py: the admission domain of the fused-gradient training kernel k_snet6
(csrc/k_snet6.hip snet6_supported) -- plain-SIREN NIFMultiScale, 49..64 units, latent_dim 1, 1..4 hidden matrices, si / so <= 3, any
ParameterNet, float32 and the two 16-bit policies.  Every check prints its figures before it asserts; profiles/snet6_domain.md holds
those of an MI355X run under `pytest -s`.

Why groups: every ShapeNet weight gradient lands in the two Keras tensors pnet_last_w [1, po] and pnet_last_b [po] (po up to 17 091),
but the kernel computes the first-layer row of each coordinate, the last-layer column of each output, the biases and each hidden matrix
in separate code.  A per-tensor bar cannot see an error of a per cent in a group of a few dozen entries; a bar relative to the group's
own norm can."""
import numpy as np

from oracle import nif_oracle as O
from tests.test_gpu_parity import _cfg, _make, _make_policy, _snet6_shape


def _case(n, L, si, so, pi, nst, lst, p_act, p_res, B):
    return _cfg("NIFMultiScale", n, L, nst, lst, 1, si, so, pi, p_act=p_act, p_res=p_res), B


# name: ((kind, cfg_shape_net, cfg_parameter_net), batch) -- units x matrices, si, so, pi, ParameterNet units x layers / activation / resblock
CASES = {
    "s6_49x1_si1_so1": _case(49, 1, 1, 1, 1, 32, 2, "sine", False, 129),
    "s6_64x1_si3_so3": _case(64, 1, 3, 3, 2, 20, 1, "swish", False, 127),
    "s6_50x2_si2_so3": _case(50, 2, 2, 3, 1, 32, 2, "sine", False, 257),
    "s6_64x2_si3_so1": _case(64, 2, 3, 1, 3, 40, 2, "tanh", True, 128),
    "s6_63x3_si1_so2": _case(63, 3, 1, 2, 1, 32, 1, "swish", False, 1000),
    "s6_56x3_si3_so2": _case(56, 3, 3, 2, 3, 20, 3, "swish", False, 17),
    "s6_57x4_si2_so2": _case(57, 4, 2, 2, 2, 32, 2, "sine", False, 333),
    "s6_64x4_si3_so3": _case(64, 4, 3, 3, 1, 32, 2, "swish", False, 1031),
    "s6_49x4_si1_so3": _case(49, 4, 1, 3, 3, 64, 2, "sine", True, 2049),
}
SLOT_TENSORS = ("pnet_last_w", "pnet_last_b")


def make(name, B=None, policy="float32"):
    """engine + oracle inputs of a case: float32 as tests.test_gpu_parity._make (hypernetwork last layer x 2), a policy as _make_policy
    (x 1); the case is asserted to sit inside k_snet6's shape rule, so that a typo in the table cannot move it out of the domain"""
    cfg, B0 = CASES[name]
    key = (cfg, B0 if B is None else B)
    out = _make(key) if policy == "float32" else _make_policy(key, policy)
    spec = out[2]
    assert _snet6_shape(spec) and spec.n_hidden_mats == spec.L and not spec.s_res, name
    return out


def tensor_offsets(spec):
    """name -> (offset, size) of every Keras tensor in the flat gradient"""
    out, off = {}, 0
    for nm, shp in spec.param_shapes():
        k = int(np.prod(shp))
        out[nm] = (off, k)
        off += k
    return out


def slot_groups(spec):
    """the po axis of pnet_output split where the kernel's code splits it: [(name, indices)] -- one first-layer row per coordinate, one
    group per hidden matrix, one last-layer column per output (stride so), the first bias, one group per hidden bias, the last bias"""
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


def slot_columns(spec):
    """indices of the two ShapeNet-slot tensors in the flat gradient"""
    offs = tensor_offsets(spec)
    return np.concatenate([np.arange(offs[t][0], offs[t][0] + offs[t][1]) for t in SLOT_TENSORS])


def group_table(spec, g, gref):
    """{(tensor, group): (|g - ref| over the group, |ref| over the group, |ref| over the tensor)}; g, gref flat"""
    g, gref = np.asarray(g, np.float64), np.asarray(gref, np.float64)
    offs, out = tensor_offsets(spec), {}
    for t in SLOT_TENSORS:
        off, k = offs[t]
        assert k == spec.po
        a, b = g[off:off + k], gref[off:off + k]
        nt = float(np.linalg.norm(b))
        for nm, idx in slot_groups(spec):
            out[(t, nm)] = (float(np.linalg.norm(a[idx] - b[idx])), float(np.linalg.norm(b[idx])), nt)
    return out


def both_routes(engine, x, y, sw):
    """the same batch through the fused kernel (fuse_gw 1) and through k_snet4 + k_gw_* (fuse_gw 0) on one engine: ((loss, g), (loss, g))"""
    engine.set_option("fuse_gw", 1)
    fused = engine.loss_and_grad(x, y, sw)
    engine.set_option("fuse_gw", 0)
    try:
        unfused = engine.loss_and_grad(x, y, sw)
    finally:
        engine.set_option("fuse_gw", 1)
    return fused, unfused


def check_tensor_bars(spec, loss, g, lref, gref, what, loss_bar=2e-6, flat_bar=3e-5):
    """the bars of test_loss_and_grad_match_oracle: loss 2e-6, every tensor 5e-5 of its norm + 2.5e-7 of the whole gradient's, flat 3e-5"""
    flat = O.flatten(gref)
    gnorm = float(np.linalg.norm(flat))
    print("%s: loss %.9e ref %.9e (%.1e)" % (what, loss, lref, abs(loss - lref) / abs(lref)))
    assert abs(loss - lref) <= loss_bar * abs(lref), (what, loss, lref)
    off = 0
    for (nm, shp), gr in zip(spec.param_shapes(), gref):
        k = int(np.prod(shp))
        err = float(np.linalg.norm(np.asarray(g[off:off + k], np.float64) - gr.ravel()))
        off += k
        assert err <= 5e-5 * np.linalg.norm(gr) + 2.5e-7 * gnorm, (what, nm, err, float(np.linalg.norm(gr)))
    rel = float(np.linalg.norm(np.asarray(g, np.float64) - flat)) / gnorm
    print("%s: flat gradient %.2e" % (what, rel))
    if flat_bar is not None:
        assert rel < flat_bar, (what, rel)


def measure_groups(spec, g_fused, g_unfused, gref):
    """per group: (err fused, err unfused, |ref_G|, |ref_T|) and the whole gradient's norm"""
    flat = O.flatten(gref)
    tf, tu = group_table(spec, g_fused, flat), group_table(spec, g_unfused, flat)
    return {k: (tf[k][0], tu[k][0], tf[k][1], tf[k][2]) for k in tf}, float(np.linalg.norm(flat))


def worst(rows):
    """(worst err_G / |ref_G| fused, its group, the same unfused, its group, worst err_G(fused) / err_G(unfused), its group,
    worst err_G(fused) / (3 err_G(unfused) + 5e-5 |ref_G|) = the share of the fused bar used, its group)"""
    kf = max(rows, key=lambda k: rows[k][0] / rows[k][2])
    ku = max(rows, key=lambda k: rows[k][1] / rows[k][2])
    kq = max(rows, key=lambda k: rows[k][0] / max(rows[k][1], 1e-300))
    kr = max(rows, key=lambda k: rows[k][0] / (3.0 * rows[k][1] + 5e-5 * rows[k][2]))
    return (rows[kf][0] / rows[kf][2], "%s %s" % kf, rows[ku][1] / rows[ku][2], "%s %s" % ku,
            rows[kq][0] / max(rows[kq][1], 1e-300), "%s %s" % kq,
            rows[kr][0] / (3.0 * rows[kr][1] + 5e-5 * rows[kr][2]), "%s %s" % kr)


def check_group_bars(spec, g_fused, g_unfused, gref, what):
    """both routes: err_G <= 5e-5 |ref_T| + 2.5e-7 |ref| (T the enclosing tensor; implied by the per-tensor bar, stated per group so that
    a failure names the group); fused route: err_G <= 3 err_G(unfused) + 5e-5 |ref_G| -- relative to the group's OWN norm, with the
    unfused route (which sums the same three bf16 (hi, lo) products per pair, in another order and tiling) as the yardstick"""
    rows, gnorm = measure_groups(spec, g_fused, g_unfused, gref)
    w = worst(rows)
    print("%s: worst group err / |ref_G|: fused %.2e (%s), unfused %.2e (%s); worst fused / unfused %.2f (%s); share of the fused bar "
          "3 unfused + 5e-5 |ref_G| used %.2f (%s)" % ((what,) + w))
    for k, (ef, eu, ng, nt) in sorted(rows.items()):
        assert eu <= 5e-5 * nt + 2.5e-7 * gnorm, (what, "unfused", k, eu, ng, nt)
        assert ef <= 5e-5 * nt + 2.5e-7 * gnorm, (what, "fused", k, ef, ng, nt)
    for k, (ef, eu, ng, nt) in sorted(rows.items()):
        assert ef <= 3.0 * eu + 5e-5 * ng, (what, "fused vs unfused", k, ef, eu, ng)
    return rows


def check_route_witness(spec, g_fused, g_unfused, bar, what):
    """every sum of the library has a fixed order, so a silent fallback to k_snet4 + k_gw_* under fuse_gw 1 reproduces fuse_gw 0 bit for
    bit; the fused kernel sums per workgroup in registers and cannot.  Different bits in the ShapeNet slot columns, yet the same gradient"""
    cols = slot_columns(spec)
    g1, g0 = np.asarray(g_fused), np.asarray(g_unfused)
    ndiff = int((g1[cols] != g0[cols]).sum())
    d = float(np.linalg.norm(g1.astype(np.float64) - g0) / np.linalg.norm(g0.astype(np.float64)))
    print("%s: %d of %d slot entries differ in bits between the routes, flat distance %.2e" % (what, ndiff, cols.size, d))
    assert np.all(np.isfinite(g1)) and np.all(np.isfinite(g0)), what
    assert ndiff > 0, (what, "fuse_gw 1 reproduced fuse_gw 0 bit for bit: the fused kernel did not run")
    assert d < bar, (what, d)
