"""tests/small_domain.py without a GPU: the case table against the restated admission rule of k_small, the LDS footprints of the
boundary shapes, and the conditions under which the fp64 oracle is a fair reference for a float32 kernel (no pre-activation within
1e-5 of a derivative kink, no |prediction - target| within 1e-5 of mae's)."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import small_domain as D


def test_every_case_sits_on_its_labelled_side_and_the_footprints_are_the_stated_ones():
    for name in D.CASES:
        D.check_side(name)
    assert len(D.INSIDE) + len(D.OUTSIDE) == len(D.CASES) and len(D.OUTSIDE) == 16
    lds = lambda nh, lst, r, si, pi: 4 * D._layout_floats(pi, lst, r, si, nh)      # noqa: E731
    assert lds(4, 1, 4, 4, 4) == 128416 and lds(3, 4, 4, 4, 4) == 127904 and lds(4, 3, 3, 4, 4) == 126736
    assert lds(4, 2, 4, 1, 1) == 134560 and lds(4, 4, 3, 1, 1) == 133264
    assert D.SMALL_LDS_MAX == 131072
    got = {name: D.small_lds_bytes(D.spec_of(name)) for name in D.CASES}
    assert got["lds_ms_nh4_lst1_r4_siren"] == 128416 and got["lds_ms_nh3_lst4_r4_swish"] == 127904
    assert got["lds_nif_nh4_lst3_r3_tanh"] == 126736
    assert got["out_lds_nh4_lst2_r4"] == 134560 and got["out_lds_nh4_lst4_r3"] == 133264
    # the two refusals are refused by the footprint alone: their inside neighbours differ in lst only
    for out, inn in (("out_lds_nh4_lst2_r4", "lds_ms_nh4_lst1_r4_io1"), ("out_lds_nh4_lst4_r3", "lds_ms_nh4_lst3_r3_io1")):
        a, b = D.spec_of(out), D.spec_of(inn)
        assert (a.n, a.nst, a.n_hidden_mats, a.r, a.si, a.so, a.pi) == (b.n, b.nst, b.n_hidden_mats, b.r, b.si, b.so, b.pi)
        assert a.lst == b.lst + 1 and got[inn] <= D.SMALL_LDS_MAX < got[out]
    # batch edges of the rule
    spec = D.spec_of("pad_nif_30x2")
    assert [D.small_admits(spec, B) for B in (0, 1, 2048, 2049)] == [False, True, True, False]
    assert not D.small_admits(spec, 257, "mixed_bfloat16") and not D.small_admits(spec, 257, "mixed_float16")
    # the extents the issue names are in the table
    specs = [D.spec_of(k) for k in D.INSIDE]
    assert any(s.n_hidden_mats == 4 for s in specs) and any(s.lst == 4 for s in specs) and any(s.r == 4 for s in specs)
    assert any(s.si == 4 and s.so == 4 and s.pi == 4 and s.r == 4 for s in specs)
    assert any(s.n == 1 and s.nst == 1 for s in specs) and any(s.n == 5 for s in specs)
    assert any(s.n_hidden_mats == 0 for s in specs) and any(s.lst == 0 for s in specs)


def test_slot_groups_cover_every_row_of_the_hyper_layer_once():
    for name in ("nif_31x2_nst17_r4_io4", "ms_24x2_r4_so1", "nif_1x1_nst1_b16", "nif_L0"):
        spec = D.spec_of(name)
        rows = D.slot_rows(spec)
        assert len(rows) == spec.r + 1
        offs = D.tensor_offsets(spec)
        cover = np.concatenate([off + idx for _, off in rows for _, idx in D.slot_groups(spec)])
        lo = offs["pnet_last_w"][0]
        assert np.array_equal(np.sort(cover), np.arange(lo, lo + (spec.r + 1) * spec.po))
        assert lo + (spec.r + 1) * spec.po == spec.n_params()
        g = np.random.default_rng(0).standard_normal(spec.n_params())
        t = D.group_table(spec, g, g)
        assert all(v[0] == 0.0 for v in t.values())
        tot = np.sqrt(sum(v[1] ** 2 for v in t.values()))
        assert abs(tot - np.linalg.norm(g[lo:])) <= 1e-12 * tot


@pytest.mark.parametrize("name", D.INSIDE + D.OUTSIDE)
def test_the_oracle_alone_is_finite_and_away_from_every_kink(name):
    spec, ws, x, y, sw = D.reference_inputs(name, B=min(D.CASES[name]["B"], 300))
    x64, y64, s64 = x.astype(np.float64), y.astype(np.float64), sw.astype(np.float64)
    loss, g = O.loss_and_grad(spec, ws, x64, y64, s64)
    g = O.flatten(g)
    assert np.isfinite(loss) and loss > 0.0 and np.all(np.isfinite(g)) and np.linalg.norm(g) > 0.0
    if name in D.INSIDE:
        pre = D.preactivations(spec, ws, x64)
        assert all(a.shape == (x.shape[0], spec.nst) for a in pre["pnet"]) and all(a.shape == (x.shape[0], spec.n) for a in pre["snet"])
        margin = D.kink_margin(spec, ws, x64)
        if name.startswith("act_"):
            print("%s: kink margin %.2e" % (name, margin))
        assert margin >= D.MARGIN, (name, margin)


def test_the_kink_helper_sees_a_kink():
    """a relu net whose first ParameterNet pre-activation of point 0 is moved onto 0 through the bias"""
    spec, ws, x, y, sw = D.reference_inputs("act_nif_relu")
    pre = D.preactivations(spec, ws, x)
    ws = [w.copy() for w in ws]
    ws[1][3] -= pre["pnet"][0][0, 3]
    assert D.kink_margin(spec, ws, x) < 1e-12
    # ... and an activation without a kink has no margin to keep
    spec, ws, x, y, sw = D.reference_inputs("act_nif_tanh")
    assert D.kink_margin(spec, ws, x) == np.inf


def test_the_mae_case_keeps_every_residual_off_zero():
    spec, ws, x, y, sw = D.reference_inputs("loss_nif_30x2_so3_r2")
    e = O.forward(spec, ws, x.astype(np.float64)) - D.times3(y).astype(np.float64)
    print("mae case: min |prediction - target| %.2e; |e| > 1 on %d of %d" % (np.abs(e).min(), int((np.abs(e) > 1).sum()), e.size))
    assert np.abs(e).min() >= D.MARGIN
    assert (np.abs(e) > 1.0).sum() > e.size // 10 and (np.abs(e) < 1.0).sum() > e.size // 10      # both sides of Huber's delta
