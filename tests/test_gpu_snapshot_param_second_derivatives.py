"""Model.predict_snapshot_parameter_derivatives(order=2) on the device: u, du/dp, d2u/dp2 and the mixed block d2u/dp dx of T snapshots
against oracle.nif_oracle.hessian_analytic in fp64 on the expanded table -- per snapshot, at the bars the point-wise HessianLayer holds
for parameter columns (BAR_Y, BAR_J, BAR_HP of tests/deriv_cases.py; whole tensor and per point), each case after the point-wise
nif_hessian on the same table has held them --, against tests/snapparam2_ref.latent_second along drawn directions, the bit-for-bit
contracts of the call, and its neighbours in the C-ABI.  Sizes and weights as tests/test_gpu_snapshot_param_derivatives.py."""
import ctypes as C

import numpy as np
import pytest

from tests.deriv_cases import BAR_HP, BAR_J, BAR_Y, CASES as DCASES, SENT, Fenced, Ref, assert_bars, bits_equal, c_hessian
from tests.snapparam2_ref import latent_second, pnet_directions
from tests.test_gpu_parity import _cfg, _make, _make_policy, _one_ulp_weights

pytestmark = pytest.mark.gpu

WIDE = "w129x1"
# the forms of k_jac_wt2: MODE 0 at NBL 1, 2 and 8, MODE 1 at NBL 3, MODE 2 at NBL 2; general pairs on the nets with pi = 3; the
# last-layer class at pi = 3, at so * r = 30, and wider than 128 units (phi alone)
HYPER = ["ms_tiny_b1", "ms_32x3_r2_pi3", "nif_32x2_pi3", "ms_res_48x2_pres", "ms_cfg3_128x3"]
LAST = ["ll_32x2_pi3", "ll_cfg4_128x2_r10_so3"]
NETS = HYPER + LAST + [WIDE]
# the limit of the call, 8 parameter columns (36 pairs), on the last-layer class: its p= route stacks one a'' vector per pair
LOCAL = {"ll_32x2_pi8": _cfg("LL", 32, 2, 32, 1, 3, 2, 2, 8)}
P8 = ["ll_32x2_pi8"]
MIXED = "ms_cfg2_64x4/mixed_bfloat16"
RAGGED = [1, 7, 64, 257, 33, 0]    # a single point, partial tiles, an exact tile multiple, tile + 1, an empty snapshot
SHARED_T, SHARED_M = 3, 100
ND = 4                             # directions of the drawn latent= tests: 10 pairs, 6 general and 4 diagonal
NIF_ERR_INVALID, NIF_ERR_STATE = -1, -4

_cache = {}


def _build(case):
    name, _, policy = case.partition("/")
    if name == WIDE:
        from tests.wide_ll_cases import fresh
        return fresh(name)
    if policy:
        return _make_policy(name, policy)
    if name in LOCAL:
        return _make((LOCAL[name], 8), boost=1.0)
    return _make((DCASES[name], 8), boost=1.0) if name in DCASES else _make(name, boost=1.0)


def _setup(case):
    """model + inputs + fp64 references of a case, built once and shared by the tests (nothing below writes into them)"""
    if case in _cache:
        return _cache[case]
    m, model, spec, ws, _, _, _ = _build(case)
    rng = np.random.default_rng(11)
    T = len(RAGGED)
    p = rng.uniform(-1, 1, size=(T, spec.pi)).astype(np.float32)              # distinct per snapshot: a mixed-up image is an O(1) error
    xs = [rng.uniform(-1, 1, size=(n, spec.si)).astype(np.float32) for n in RAGGED]
    xsh = rng.uniform(-1, 1, size=(SHARED_M, spec.si)).astype(np.float32)
    dirs = rng.uniform(-1, 1, size=(T, ND, spec.r)).astype(np.float32)
    dd = rng.uniform(-1, 1, size=(T, ND, ND, spec.r)).astype(np.float32)
    dd = (dd + dd.transpose(0, 2, 1, 3)).astype(np.float32)                   # a + a^T: symmetric bit for bit

    def table(t, x):
        return np.hstack([np.tile(p[t], (x.shape[0], 1)), x])

    d = dict(case=case, m=m, model=model, spec=spec, ws=ws, p=p, xs=xs, xsh=xsh, dirs=dirs, dd=dd, table=table, e=m._engine)
    # the coordinate columns of the case (a ShapeNet wider than 128 units has no phi' kernel: parameter columns alone)
    d["xi"] = None if case == WIDE else list(range(spec.si))
    if "/" not in case:
        d["ref_ragged"] = [Ref(spec, ws, table(t, xs[t])) if RAGGED[t] else None for t in range(T)]
        d["ref_shared"] = [Ref(spec, ws, table(t, xsh)) for t in range(SHARED_T)]
    _cache[case] = d
    return d


def _latents(d):
    """the float32 latents the device's own ParameterNet gives for p (last-layer class: the coefficient vectors)"""
    if "lat" not in d:
        d["lat"] = d["m"].model_p_to_lr().predict(d["p"])
        assert d["lat"].shape == (len(RAGGED), d["spec"].r) and d["lat"].dtype == np.float32
    return d["lat"]


def _oracle_dirs(d):
    """the float32 cast of the oracle's dz/dp [T, pi, r] and d2z/dp2 [T, pi, pi, r] at p"""
    if "odirs" not in d:
        spec = d["spec"]
        _, dz, ddz = pnet_directions(spec, d["ws"], d["p"], list(range(spec.pi)))
        dz, ddz = dz.astype(np.float32), ddz.astype(np.float32)
        assert bits_equal(ddz, ddz.transpose(0, 2, 1, 3))
        d["odirs"] = dz, ddz
    return d["odirs"]


def _blocks(pair_j, pair_h, nd):
    """the reference's (J, H) pairs over [nd parameter | coordinate] columns -> the pairs of dudp, d2udp2, dudx, d2udpdx"""
    return ((pair_j[0][:, :, :nd], pair_j[1][:, :, :nd]), (pair_h[0][:, :, :nd, :nd], pair_h[1][:, :, :nd, :nd]),
            (pair_j[0][:, :, nd:], pair_j[1][:, :, nd:]), (pair_h[0][:, :, :nd, nd:], pair_h[1][:, :, :nd, nd:]))


def _check(what, d, ref, outs, table=None):
    """outs = (u, dudp, d2udp2[, dudx, d2udpdx]) of one snapshot against its reference at every parameter column (and the case's
    coordinate columns when outs has five members).  With table: first the point-wise nif_hessian on it holds the same bars"""
    spec = d["spec"]
    yi, cols = list(range(spec.so)), list(range(spec.pi))
    xc = [spec.pi + j for j in d["xi"]] if len(outs) == 5 else []
    py, pj, ph = ref.gather(yi, cols + xc)
    bj, bh, bjx, bhx = _blocks(pj, ph, spec.pi)
    if table is not None:
        rc, hy, hj, hh = c_hessian(d["e"], table, yi, cols + xc)
        if d["case"] == WIDE:
            assert rc == NIF_ERR_INVALID                        # (no point-wise layer for this net: nothing to hold the bars first)
        else:
            assert rc == 0
            assert_bars(what + " nif_hessian y", hy, py, BAR_Y)
            assert_bars(what + " nif_hessian J", hj, pj, BAR_J)
            assert_bars(what + " nif_hessian H", hh, ph, BAR_HP)
    assert_bars(what + " u", outs[0], py, BAR_Y)
    assert_bars(what + " dudp", outs[1], bj, BAR_J)
    assert_bars(what + " d2udp2", outs[2], bh, BAR_HP)
    if xc:
        assert_bars(what + " dudx", outs[3], bjx, BAR_J)
        assert_bars(what + " d2udpdx", outs[4], bhx, BAR_HP)


def _check_all(what, d, ragged, shared, nd, with_layer=False):
    spec = d["spec"]
    nx = len(d["xi"]) if len(shared) == 5 else 0
    tails = [(spec.so,), (spec.so, nd), (spec.so, nd, nd)] + ([(spec.so, nx), (spec.so, nd, nx)] if nx else [])
    assert len(ragged) == len(shared) == len(tails)
    for out, tail in zip(shared, tails):
        assert out.shape == (SHARED_T, SHARED_M) + tail and out.dtype == np.float32
    for t, n in enumerate(RAGGED):
        for out, tail in zip(ragged, tails):
            assert out[t].shape == (n,) + tail and out[t].dtype == np.float32
        if n:
            _check("%s ragged snapshot %d (%d points)" % (what, t, n), d, d["ref_ragged"][t], [o[t] for o in ragged],
                   d["table"](t, d["xs"][t]) if with_layer else None)
    for t in range(SHARED_T):
        _check("%s shared snapshot %d" % (what, t), d, d["ref_shared"][t], [o[t] for o in shared],
               d["table"](t, d["xsh"]) if with_layer else None)


def _xkw(d, with_x=True):
    return dict(order=2, x_index=d["xi"]) if (with_x and d["xi"] is not None) else dict(order=2)


@pytest.mark.parametrize("name", NETS + P8)
def test_p_route_matches_the_oracle_snapshot_by_snapshot(name):
    d = _setup(name)
    f = d["model"].predict_snapshot_parameter_derivatives
    ragged = f(d["xs"], p=d["p"], **_xkw(d))
    shared = f(d["xsh"], p=d["p"][:SHARED_T], **_xkw(d))
    _check_all("%s p=" % name, d, ragged, shared, d["spec"].pi, with_layer=True)
    if d["xi"] is not None:             # without x_index: three outputs, the same second order
        r3 = f(d["xs"], p=d["p"], order=2)
        s3 = f(d["xsh"], p=d["p"][:SHARED_T], order=2)
        _check_all("%s p= without x_index" % name, d, r3, s3, d["spec"].pi)
        for k in range(3):
            assert bits_equal(s3[k], shared[k]) and all(bits_equal(a, b) for a, b in zip(r3[k], ragged[k])), (name, k)


@pytest.mark.parametrize("name", NETS + P8)
def test_latent_route_with_the_oracles_directions_matches_the_same_oracle(name):
    """latent= with the float32 latents of model_p_to_lr().predict(p), dlatent and d2latent = the float32 casts of the oracle's dz/dp and
    d2z/dp2: held to the reference of the p= route at the same bars"""
    d = _setup(name)
    lat, (dz, ddz) = _latents(d), _oracle_dirs(d)
    f = d["model"].predict_snapshot_parameter_derivatives
    ragged = f(d["xs"], latent=lat, dlatent=dz, d2latent=ddz, **_xkw(d))
    shared = f(d["xsh"], latent=lat[:SHARED_T], dlatent=dz[:SHARED_T], d2latent=ddz[:SHARED_T], **_xkw(d))
    _check_all("%s latent= dz/dp, d2z/dp2" % name, d, ragged, shared, d["spec"].pi)


@pytest.mark.parametrize("name", NETS)
def test_latent_route_along_four_drawn_directions_matches_autograd_through_the_field(name):
    """nd = 4 directions and a symmetric d2latent in U(-1, 1): ten pairs.  Reference: tests/snapparam2_ref.latent_second at the same
    float32 latents in float64, and the same under one ulp of weight noise for the per-point conditioning floor; bars: BAR_Y, BAR_J,
    BAR_HP through assert_bars (whole tensor and per point), per snapshot, every output"""
    d = _setup(name)
    spec, ws = d["spec"], [np.asarray(w, dtype=np.float64) for w in d["ws"]]
    ws1 = _one_ulp_weights(ws)
    lat, dirs, dd = _latents(d), d["dirs"], d["dd"]
    f = d["model"].predict_snapshot_parameter_derivatives
    ragged = f(d["xs"], latent=lat, dlatent=dirs, d2latent=dd, **_xkw(d))
    shared = f(d["xsh"], latent=lat[:SHARED_T], dlatent=dirs[:SHARED_T], d2latent=dd[:SHARED_T], **_xkw(d))
    xi = d["xi"] or []
    names = ["u", "dudp", "d2udp2", "dudx", "d2udpdx"]
    bars = [BAR_Y, BAR_J, BAR_HP, BAR_J, BAR_HP]
    for what, xs_, got in (("ragged", d["xs"], ragged), ("shared", [d["xsh"]] * SHARED_T, shared)):
        for t, x in enumerate(xs_):
            if not x.shape[0]:
                continue
            want = latent_second(spec, ws, lat[t].astype(np.float64), dirs[t], dd[t], x, xi)
            want1 = latent_second(spec, ws1, lat[t].astype(np.float64), dirs[t], dd[t], x, xi)
            for k in range(len(got)):
                assert got[k][t].dtype == np.float32
                assert_bars("%s %s snapshot %d %s" % (name, what, t, names[k]), got[k][t], (want[k], want1[k]), bars[k])


@pytest.mark.parametrize("name", NETS)
def test_bit_for_bit_symmetry_first_order_outputs_pairs_and_scaling(name):
    d = _setup(name)
    lat, dirs, dd = _latents(d), d["dirs"], d["dd"]
    f = d["model"].predict_snapshot_parameter_derivatives
    for x, sl in ((d["xs"], slice(None)), (d["xsh"], slice(0, SHARED_T))):
        # d2udp2 is symmetric, u and dudp are the order=1 call's: p= and latent=
        for kw in (dict(p=d["p"][sl]), dict(latent=lat[sl], dlatent=dirs[sl])):
            one = f(x, **kw)
            two = f(x, d2latent=dd[sl], **kw, **_xkw(d)) if "latent" in kw else f(x, **kw, **_xkw(d))
            for a, b in zip(one, two[:2]):
                assert all(bits_equal(u, v) for u, v in zip(a, b)), (name, sorted(kw))
            assert all(bits_equal(h, np.swapaxes(h, -1, -2)) for h in two[2]), (name, sorted(kw))
        # a pair of the nd = 4 call is the nd = 2 call that holds only those two directions
        four = f(x, latent=lat[sl], dlatent=dirs[sl], d2latent=dd[sl], **_xkw(d))
        for a, b in ((0, 1), (1, 3), (0, 3)):
            two = f(x, latent=lat[sl], dlatent=dirs[sl][:, [a, b]], d2latent=dd[sl][:, [a, b]][:, :, [a, b]], **_xkw(d))
            for h4, h2 in zip(four[2], two[2]):
                assert bits_equal(h2, np.asarray(h4)[..., [a, b], :][..., [a, b]]), (name, a, b)
            if d["xi"] is not None:
                for m4, m2 in zip(four[4], two[4]):
                    assert bits_equal(m2, np.asarray(m4)[..., [a, b], :]), (name, a, b)
        # every product is linear in each direction: doubling direction 1 doubles the pairs it is in, quadruples its diagonal pair,
        # doubles its mixed rows and leaves the rest (no d2latent: its term does not scale)
        base = f(x, latent=lat[sl], dlatent=dirs[sl], **_xkw(d))
        twice_dirs = dirs[sl].copy()
        twice_dirs[:, 1] *= 2.0
        twice = f(x, latent=lat[sl], dlatent=twice_dirs, **_xkw(d))
        scale = np.ones((ND, ND), np.float32)
        scale[1, :] *= 2.0
        scale[:, 1] *= 2.0
        for h1, h2 in zip(base[2], twice[2]):
            assert bits_equal(h2, np.asarray(h1) * scale), name
        if d["xi"] is not None:
            for m1, m2 in zip(base[4], twice[4]):
                assert bits_equal(m2, np.asarray(m1) * scale[:, :1]), name


@pytest.mark.parametrize("case,by", [(c, "p") for c in NETS + [MIXED]] + [(c, "latent") for c in NETS])
def test_permuting_the_snapshots_permutes_the_results_bit_for_bit(case, by):
    d = _setup(case)
    perm = [3, 0, 5, 4, 2, 1]
    f = d["model"].predict_snapshot_parameter_derivatives
    if by == "p":
        kw = lambda idx: dict(p=d["p"][idx], **_xkw(d))
    else:
        lat = _latents(d)
        kw = lambda idx: dict(latent=lat[idx], dlatent=d["dirs"][idx], d2latent=d["dd"][idx], **_xkw(d))
    ident = list(range(len(RAGGED)))
    a = f(d["xs"], **kw(ident))
    b = f([d["xs"][i] for i in perm], **kw(perm))
    sa = f(d["xsh"], **kw(ident))
    sb = f(d["xsh"], **kw(perm))
    for k in range(len(a)):
        for j, i in enumerate(perm):
            assert bits_equal(b[k][j], a[k][i]), (case, by, k, i)
        assert bits_equal(sb[k], sa[k][perm]), (case, by, k)


@pytest.mark.parametrize("case,by", [(c, "p") for c in NETS + [MIXED]] + [(c, "latent") for c in NETS])
def test_chunked_calls_are_bit_identical_to_the_unchunked_call(case, by, monkeypatch):
    from nif_amd.model import Model
    d = _setup(case)
    f = d["model"].predict_snapshot_parameter_derivatives
    kw = dict(p=d["p"], **_xkw(d)) if by == "p" else dict(latent=_latents(d), dlatent=d["dirs"], d2latent=d["dd"], **_xkw(d))
    whole = f(d["xs"], **kw)
    whole_s = f(d["xsh"], **kw)
    e, calls = d["e"], []
    orig = e.snapshot_param_second_derivatives_ragged
    monkeypatch.setattr(e, "snapshot_param_second_derivatives_ragged",
                        lambda rows, dr, ddr, xs, *a: (calls.append([x.shape[0] for x in xs]), orig(rows, dr, ddr, xs, *a))[1])
    monkeypatch.setattr(Model, "_SNAPSHOT_CHUNK_BYTES", 100)                    # below one point's bytes ...
    e.set_option("snapshot_image_bytes", 1)                                     # ... and one snapshot image at a time inside the library
    try:
        parts = f(d["xs"], batch_size=100, **kw)                                # 100 points per chunk
        parts_s = f(d["xsh"], batch_size=250, **kw)                             # two whole snapshots per chunk
    finally:
        e.set_option("snapshot_image_bytes", 0)
    assert calls == [[1, 7, 64], [100], [100], [57, 33]]                        # T = 6 in four chunks, the long snapshot cut twice
    for k in range(len(whole)):
        for a, b in zip(parts[k], whole[k]):
            assert bits_equal(a, b)
        assert bits_equal(parts_s[k], whole_s[k])


def test_mixed_policy_with_p_equals_nif_hessians_blocks_bit_for_bit():
    d = _setup(MIXED)
    spec = d["spec"]
    yi, cols = list(range(spec.so)), list(range(spec.pi)) + [spec.pi + j for j in d["xi"]]
    f = d["model"].predict_snapshot_parameter_derivatives
    ragged = f(d["xs"], p=d["p"], **_xkw(d))
    shared = f(d["xsh"], p=d["p"][:SHARED_T], **_xkw(d))
    one = f(d["xsh"], p=d["p"][:SHARED_T])
    assert bits_equal(one[0], shared[0]) and bits_equal(one[1], shared[1])
    pi = spec.pi
    for x_of, got_of, ts in ((lambda t: d["xs"][t], lambda t: [o[t] for o in ragged], [t for t, n in enumerate(RAGGED) if n]),
                             (lambda t: d["xsh"], lambda t: [o[t] for o in shared], range(SHARED_T))):
        for t in ts:
            rc, y, J, H = c_hessian(d["e"], d["table"](t, x_of(t)), yi, cols)
            assert rc == 0
            got = got_of(t)
            assert bits_equal(got[2], H[:, :, :pi, :pi]) and bits_equal(got[4], H[:, :, :pi, pi:]) and bits_equal(got[3], J[:, :, pi:]), t


def test_mixed_policy_with_latents_is_refused_and_predict_works_afterwards():
    from nif_amd._lib import NifError
    d = _setup(MIXED)
    x = d["table"](0, d["xsh"])
    before = d["model"].predict(x)
    lat = _latents(d)
    for mesh in (d["xsh"], d["xs"]):
        with pytest.raises(NifError) as ei:
            d["model"].predict_snapshot_parameter_derivatives(mesh, latent=lat, dlatent=d["dirs"], order=2)
        assert "not built" in str(ei.value) and "mixed_bfloat16" in str(ei.value)
    assert np.array_equal(d["model"].predict(x), before)


def test_the_wide_last_layer_net_refuses_coordinate_columns_with_the_128_unit_message():
    from nif_amd._lib import NifError
    d = _setup(WIDE)
    with pytest.raises(NifError) as ei:
        d["model"].predict_snapshot_parameter_derivatives(d["xsh"], p=d["p"][:SHARED_T], order=2, x_index=[0])
    assert "up to 128 units" in str(ei.value)
    out = d["model"].predict_snapshot_parameter_derivatives(d["xsh"], p=d["p"][:SHARED_T], order=2)
    assert bits_equal(out[0], d["model"].predict_snapshots(d["xsh"], p=d["p"][:SHARED_T]))


def _i32(idx):
    return (C.c_int32 * len(idx))(*[int(i) for i in idx])


def _args(e, rows, drows, ddrows, nd, T, x, offsets, M, yi, pi_, xi, outs):
    """nif_snapparam2_args over raw pointers (host or device); the index arrays and offsets stay alive on the struct.  drows None: rows
    are p rows with the columns pi_; else latents with nd directions each.  outs: u, dudp, d2udp2[, dudx, d2udpdx]"""
    from nif_amd import _lib
    a = _lib.nif_snapparam2_args()
    a.abi_version, a.ctx = _lib.NIF_SNAPPARAM2_ABI_VERSION, e.ctx
    a.rows, a.rows_are_latent, a.T, a.x, a.M = rows, 0 if drows is None else 1, T, x, M
    a._keep = (_i32(yi), None if pi_ is None else _i32(pi_), offsets, _i32(xi) if xi else None)
    a.offsets_host = None if offsets is None else offsets.ctypes.data_as(C.POINTER(C.c_int64))
    a.y_idx, a.ny = a._keep[0], len(yi)
    if drows is None:
        a.p_idx, a.np = a._keep[1], len(pi_)
    else:
        a.drows, a.ddrows, a.nd = drows, ddrows, nd
    if xi:
        a.x_idx, a.nxc = a._keep[3], len(xi)
        a.dudx, a.d2udpdx = outs[3], outs[4]
    a.u, a.dudp, a.d2udp2 = outs[0], outs[1], outs[2]
    return a


def _forms(d):
    """(offsets, x, n) of the shared and the ragged form over all len(RAGGED) rows of p"""
    off = np.concatenate([[0], np.cumsum(RAGGED)]).astype(np.int64)
    return ((None, np.ascontiguousarray(d["xsh"]), len(RAGGED) * SHARED_M), (off, np.ascontiguousarray(np.concatenate(d["xs"])), sum(RAGGED)))


def _rows_of(s, ny, nd, nx):
    return [s.so, ny * nd, ny * nd * nd] + ([ny * nx, ny * nd * nx] if nx else [])


def _shapes_of(s, n, ny, nd, nx):
    return [(n, s.so), (n, ny, nd), (n, ny, nd, nd)] + ([(n, ny, nx), (n, ny, nd, nx)] if nx else [])


@pytest.mark.parametrize("name", ["ms_res_48x2_pres", "ll_32x2_pi3"])
def test_host_pointer_entry_equals_the_model_call(name):
    from nif_amd._lib import check, ptr
    d = _setup(name)
    e, s = d["e"], d["spec"]
    yi, cols, xi = list(range(s.so))[::-1], list(range(s.pi)), d["xi"]
    lat, dirs, dd = np.ascontiguousarray(_latents(d)), np.ascontiguousarray(d["dirs"]), np.ascontiguousarray(d["dd"])
    f = d["model"].predict_snapshot_parameter_derivatives
    for offsets, x, n in _forms(d):
        mesh = d["xsh"] if offsets is None else d["xs"]
        for by in ("p", "latent"):
            nd = len(cols) if by == "p" else ND
            outs = [np.empty(sh, np.float32) for sh in _shapes_of(s, n, len(yi), nd, len(xi))]
            if by == "p":
                a = _args(e, ptr(d["p"]), None, None, 0, len(RAGGED), ptr(x), offsets, SHARED_M, yi, cols, xi, [ptr(o) for o in outs])
                want = f(mesh, p=d["p"], y_index=yi, order=2, x_index=xi)
            else:
                a = _args(e, ptr(lat), ptr(dirs), ptr(dd), ND, len(RAGGED), ptr(x), offsets, SHARED_M, yi, None, xi, [ptr(o) for o in outs])
                want = f(mesh, latent=lat, dlatent=dirs, d2latent=dd, y_index=yi, order=2, x_index=xi)
            check(e.lib.nif_snapshot_param_second_derivatives(C.byref(a)))
            for got, w in zip(outs, want):
                assert bits_equal(got, np.concatenate(list(w)).reshape(got.shape)), (name, by, offsets is None)


@pytest.mark.parametrize("name", ["nif_32x2_pi3", "ms_cfg3_128x3", "ll_cfg4_128x2_r10_so3", WIDE])
def test_dev_entry_writes_inside_its_outputs(name):
    """the five outputs at float offsets 1, 2, 3, 1, 2 from a 16-byte boundary, each with 32 of its rows of sentinel behind it (a tile's
    tail past a snapshot's last point would land in the next snapshot or there): every pad word untouched, the results the model's"""
    from nif_amd.engine import DeviceArray
    d = _setup(name)
    e, s = d["e"], d["spec"]
    yi, cols, xi = list(range(s.so)), list(range(s.pi)), d["xi"] or []
    lat, dirs, dd = _latents(d), d["dirs"], d["dd"]
    f = d["model"].predict_snapshot_parameter_derivatives
    for offsets, x, n in _forms(d):
        mesh = d["xsh"] if offsets is None else d["xs"]
        for by in ("p", "latent"):
            nd = len(cols) if by == "p" else ND
            rows = d["p"] if by == "p" else lat
            d_r, d_d, d_dd, d_x = DeviceArray(e, rows.size), DeviceArray(e, dirs.size), DeviceArray(e, dd.size), DeviceArray(e, x.size)
            d_r.upload(rows); d_d.upload(dirs); d_dd.upload(dd); d_x.upload(x)
            fences = [Fenced(e, n, row, off) for row, off in zip(_rows_of(s, len(yi), nd, len(xi)), (1, 2, 3, 1, 2))]
            try:
                a = _args(e, d_r.at(0), None if by == "p" else d_d.at(0), None if by == "p" else d_dd.at(0), nd, len(RAGGED), d_x.at(0),
                          offsets, SHARED_M, yi, cols if by == "p" else None, xi, [fc.at() for fc in fences])
                rc = e.lib.nif_snapshot_param_second_derivatives_dev(C.byref(a))
                e.sync()
            finally:
                taken = [fc.take(sh) for fc, sh in zip(fences, _shapes_of(s, n, len(yi), nd, len(xi)))]
                d_r.free(); d_d.free(); d_dd.free(); d_x.free()
            assert rc == 0, e.lib.nif_last_error()
            assert all(ok for _, ok in taken), (name, by, offsets is None, "wrote outside", [ok for _, ok in taken])
            assert not any(np.any(o.view(np.uint32) == SENT.view(np.uint32)) for o, _ in taken)
            kw = dict(order=2, x_index=xi) if xi else dict(order=2)
            want = f(mesh, p=d["p"], **kw) if by == "p" else f(mesh, latent=lat, dlatent=dirs, d2latent=dd, **kw)
            for (got, _), w in zip(taken, want):
                assert bits_equal(got, np.concatenate(list(w)).reshape(got.shape))


def test_the_c_abi_refuses_what_the_header_says_it_refuses_and_stays_usable():
    from nif_amd._lib import ptr
    d = _setup("ms_res_48x2_pres")
    e, s = d["e"], d["spec"]
    yi, cols, xi = list(range(s.so)), list(range(s.pi)), d["xi"]
    T, n = len(RAGGED), len(RAGGED) * SHARED_M
    lat, dirs, dd = np.ascontiguousarray(_latents(d)), np.ascontiguousarray(d["dirs"]), np.ascontiguousarray(d["dd"])
    nmax = max(s.pi, ND)
    outs = [np.empty(sh, np.float32) for sh in _shapes_of(s, n, s.so, nmax, len(xi))]

    def call(latent=False, yi=yi, pi_=cols, xi=xi, **fields):
        po = [ptr(o) for o in outs]
        if latent:
            a = _args(e, ptr(lat), ptr(dirs), ptr(dd), ND, T, ptr(d["xsh"]), None, SHARED_M, yi, None, xi, po)
        else:
            a = _args(e, ptr(d["p"]), None, None, 0, T, ptr(d["xsh"]), None, SHARED_M, yi, pi_, xi, po)
        for k, v in fields.items():
            setattr(a, k, v)
        rc = e.lib.nif_snapshot_param_second_derivatives(C.byref(a))
        return rc, e.lib.nif_last_error().decode()

    assert call()[0] == 0
    # (the p= call fills [n, so, pi, ..] at the front of every output)
    flat = lambda: [o.reshape(-1)[:int(np.prod(sh))].copy() for o, sh in zip(outs, _shapes_of(s, n, s.so, s.pi, len(xi)))]
    good = flat()
    assert call(latent=True)[0] == 0
    keep = _i32([0])
    refused = [
        (dict(abi_version=2), "abi_version"),
        (dict(latent=True, drows=None), "need drows"),                           # latents without directions
        (dict(drows=ptr(dirs)), "go with latent rows"),                          # directions with p rows
        (dict(ddrows=ptr(dd)), "go with latent rows"),
        (dict(nd=1), "go with latent rows"),
        (dict(latent=True, p_idx=keep, np=1), "not with latents"),               # parameter columns with latents
        (dict(latent=True, nd=0), "1 to 8 directions"),
        (dict(latent=True, nd=9), "1 to 8 directions"),
        (dict(np=0), "1 to 8 parameter columns"),
        (dict(np=9), "1 to 8 parameter columns"),
        (dict(p_idx=None), "1 to 8 parameter columns"),
        (dict(pi_=[s.pi]), "p_index out of range"),
        (dict(pi_=[-1]), "p_index out of range"),
        (dict(pi_=[0, 0]), "repeated"),
        (dict(xi=[s.si]), "x_index out of range"),
        (dict(xi=[-1]), "x_index out of range"),
        (dict(xi=[0, 0]), "repeated"),
        (dict(nxc=-1), "nxc"),
        (dict(nxc=0), "go together"),                                            # x_idx without its count
        (dict(x_idx=None), "go together"),
        (dict(dudx=None), "bad argument"),                                       # coordinate columns without their outputs
        (dict(d2udp2=None), "bad argument"),
        (dict(yi=[s.so]), "y_index out of range"),
        (dict(yi=[0] * 17), "at most 16 entries"),
    ]
    for kw, msg in refused:
        rc, err = call(**kw)
        assert rc == NIF_ERR_INVALID and msg in err, (kw, rc, err)
        assert call()[0] == 0 and all(bits_equal(o, g) for o, g in zip(flat(), good)), kw      # usable, and the same, behind every refusal
    # outputs of the coordinate block without coordinate columns
    po = [ptr(o) for o in outs]
    a = _args(e, ptr(d["p"]), None, None, 0, T, ptr(d["xsh"]), None, SHARED_M, yi, cols, None, po)
    a.dudx = po[3]
    assert e.lib.nif_snapshot_param_second_derivatives(C.byref(a)) == NIF_ERR_INVALID and b"exactly when nxc is 0" in e.lib.nif_last_error()
    a = _args(e, ptr(d["p"]), None, None, 0, T, ptr(d["xsh"]), None, SHARED_M, yi, cols, xi, po)
    a.reserved[3] = 7
    assert e.lib.nif_snapshot_param_second_derivatives(C.byref(a)) == NIF_ERR_INVALID and b"reserved" in e.lib.nif_last_error()
    assert call()[0] == 0 and all(bits_equal(o, g) for o, g in zip(flat(), good))
    x = d["table"](0, d["xsh"])
    assert d["model"].predict(x).shape == (SHARED_M, s.so)


@pytest.mark.parametrize("name", ["ms_res_48x2_pres", "ll_plain_32x2_r3"])
def test_call_behind_a_deferred_optimizer_tail_and_after_set_weights_sees_the_new_weights(name):
    """Adam(1e-3), the step tests/test_gpu_snapshots.py takes for the same call order"""
    import nif_amd
    from oracle import nif_oracle as O
    m, model, spec, ws, x, y, sw = _make(name, boost=1.0)          # a model of its own: this test writes weights
    rng = np.random.default_rng(11)
    p = rng.uniform(-1, 1, size=(SHARED_T, spec.pi)).astype(np.float32)
    xsh = rng.uniform(-1, 1, size=(SHARED_M, spec.si)).astype(np.float32)
    d = dict(case=name, spec=spec, e=m._engine, xi=list(range(spec.si)))
    table = lambda t: np.hstack([np.tile(p[t], (SHARED_M, 1)), xsh])
    e = m._engine
    f = model.predict_snapshot_parameter_derivatives
    u0 = f(xsh, p=p, order=2, x_index=d["xi"])
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    e.loss_grad_dev(d_x.at(0), d_y.at(0), None, x.shape[0], x.shape[0])          # fused tail on (the default): the reduction waits
    e.adam_step_dev(nif_amd.Adam(1e-3).as_struct())
    u1 = f(xsh, p=p, order=2, x_index=d["xi"])
    ws_now = [w.astype(np.float64) for w in model.get_weights()]
    assert not np.array_equal(O.flatten(ws_now), O.flatten(ws)) and not bits_equal(u1[2], u0[2])
    for t in range(SHARED_T):
        _check("%s behind the tail, snapshot %d" % (name, t), d, Ref(spec, ws_now, table(t)), [o[t] for o in u1])
    ws2 = [(w * 1.125).astype(np.float32) for w in ws]
    model.set_weights(ws2)
    u2 = f(xsh, p=p[:1], order=2, x_index=d["xi"])
    _check("%s after set_weights" % name, d, Ref(spec, [w.astype(np.float64) for w in ws2], table(0)), [o[0] for o in u2])


def test_call_inside_a_graph_capture_is_refused_and_the_context_stays_usable():
    from nif_amd._lib import NifError
    m, model, spec, ws, x, y, sw = _make("ms_res_48x2_pres", boost=1.0)
    d = _setup("ms_res_48x2_pres")
    yi, cols, xi = list(range(spec.so)), list(range(spec.pi)), d["xi"]
    f = model.predict_snapshot_parameter_derivatives
    good = f(d["xsh"], p=d["p"][:1], order=2, x_index=xi)           # (planes packed, workspaces sized before the capture)
    e = m._engine
    n = len(RAGGED) * SHARED_M
    rows = _rows_of(spec, len(yi), len(cols), len(xi))
    at = np.concatenate([[0], np.cumsum([n * r for r in rows])])
    d_p, d_x, d_o = e.alloc(d["p"].size), e.alloc(d["xsh"].size), e.alloc(int(at[-1]))
    d_p.upload(d["p"]); d_x.upload(d["xsh"])
    off = np.array([0, 30, 60, 80, 90, 95, 100], dtype=np.int64)
    e.graph_begin()
    try:
        with pytest.raises(NifError):
            f(d["xsh"], p=d["p"], order=2)
        with pytest.raises(NifError):
            f(d["xs"], p=d["p"], order=2, x_index=xi)
        # the library's own refusal, on operands that were resident before the capture began
        for offsets in (None, off):
            a = _args(e, d_p.at(0), None, None, 0, len(RAGGED), d_x.at(0), offsets, SHARED_M, yi, cols, xi, [d_o.at(int(i)) for i in at[:-1]])
            assert e.lib.nif_snapshot_param_second_derivatives_dev(C.byref(a)) == NIF_ERR_STATE
            assert b"not capturable" in e.lib.nif_last_error()
    finally:
        e.graph_end()
    again = f(d["xsh"], p=d["p"][:1], order=2, x_index=xi)
    assert all(bits_equal(a, b) for a, b in zip(again, good))
