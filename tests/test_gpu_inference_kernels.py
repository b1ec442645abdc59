"""The factorised inference path kernel by kernel: model_lr_to_w (k_latent_to_w_flat<R> / k_latent_to_w, nif_amd/csrc/k_misc.hip)
and model_x_to_u_given_w (k_given_w<N> / k_given_w_generic, and k_pnet + k_ll_out for the last-layer class), at the launch forms
and branches launch_latent_to_w / launch_given_w choose, through the host entries and the _dev entries with offset pointers.

model_lr_to_w is checked ELEMENT BY ELEMENT against a proven bound: w[a, s] = b_s + sum_k lr[a, k] W[k, s] is a chain of r fused
multiply-adds in fp32, so |w - w64| <= (r + 2) 2^-24 (|b_s| + sum_k |lr[a, k]| |W[k, s]|) -- no room for a wrong row, a wrong column,
a stale bias or a zero.  Each case names the form and the branch it is meant to reach (launch_latent_to_w's geometry): a change of
a threshold there shows up here in review."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from nif_amd._lib import check
from tests.test_gpu_parity import _cfg, _make, _rel

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
SENT = np.float32(-7.654321e33)       # sentinel around the _dev outputs (compared bit for bit)


def _model(cfg, seed=0):
    m, model, spec, ws, x, y, sw = _make((cfg, 4), seed=seed)
    return m, spec, ws


def _last(spec, ws):
    _, _, _, last, _ = O._pnet_split(spec, ws)
    return last[0], last[1]            # [r, po], [po]


def _check_w(w, lr, W, b, row0=0, chunk_floats=1 << 22):
    """element-wise bound of model_lr_to_w on rows row0.. of the output (w [nr, po] fp32, lr [nr, r]); also returns the
    squared norms of the error and of the reference for a whole-tensor rel-L2"""
    r, po = W.shape
    W64, Wa, b64 = W.astype(np.float64), np.abs(W.astype(np.float64)), b.astype(np.float64)
    step = max(1, chunk_floats // po)
    e2 = n2 = 0.0
    for i in range(0, w.shape[0], step):
        l64 = lr[i:i + step].astype(np.float64)
        ref = l64 @ W64 + b64
        mag = np.abs(l64) @ Wa + np.abs(b64)
        err = np.abs(w[i:i + step].astype(np.float64) - ref)
        bad = np.argwhere(~(err <= (r + 2) * EPS32 * mag))
        if bad.size:
            a, s = bad[0]
            raise AssertionError("model_lr_to_w: %d elements outside the fma bound, first w[%d, %d] = %r, exact %r; all: %s"
                                 % (len(bad), row0 + i + a, s, float(w[i + a, s]), float(ref[a, s]),
                                    [(int(row0 + i + p), int(q)) for p, q in bad[:8]]))
        e2 += float(np.sum(err * err)); n2 += float(np.sum(ref * ref))
    return e2, n2


# ---- model_lr_to_w ------------------------------------------------------------------------------------------------------
# name: (cfg, B, what it reaches)
L2W = {
    # flat form, one unit per thread (B po <= 2^24 floats), R = 1, 2, 3, 4 and the generic R = 0 at r = 5, 8
    "flat_r1": (_cfg("NIF", 32, 2, 32, 2, 1, 1, 1, 1), 300, "k_latent_to_w_flat<1>, one iteration"),
    "flat_r2": (_cfg("NIFMultiScale", 48, 2, 40, 2, 2, 2, 2, 1, s_res=True, p_res=True), 515, "k_latent_to_w_flat<2>, po 9650"),
    "flat_r3": (_cfg("NIFMultiScale", 64, 2, 32, 2, 3, 2, 1, 1, p_act="swish"), 129, "k_latent_to_w_flat<3>, po 8577"),
    "flat_r4": (_cfg("NIFMultiScale", 48, 2, 32, 1, 4, 2, 1, 1), 1031, "k_latent_to_w_flat<4>, po 4897"),
    "flat_r5": (_cfg("NIF", 30, 2, 20, 1, 5, 2, 2, 2, act="tanh"), 257, "k_latent_to_w_flat<0> at r = 5, po 2012"),
    "flat_r8": (_cfg("NIFMultiScale", 32, 2, 32, 2, 8, 3, 2, 1), 4097, "k_latent_to_w_flat<0> at r = 8, po 2306"),
    # flat form, span > NIF_L2W_T units: every thread takes two or more units (e += 4 NIF_L2W_T; sc += ds; a += da)
    "flat_span_po2209": (_cfg("NIF", 32, 2, 32, 2, 1, 1, 1, 1), 8000, "flat<1>, span 2048, po < 4096: da = 1, ds = 1887"),
    "flat_span_po195": (_cfg("NIFMultiScale", 8, 2, 16, 1, 1, 2, 3, 1), 90000, "flat<1>, span 2048, po 195: da = 21, ds = 1"),
    "flat_span_po16833": (_cfg("NIFMultiScale", 64, 4, 32, 2, 1, 1, 1, 1), 1100, "flat<1>, span 2048, po > 4096: da = 0"),
    # column-window form: (r+1) planes over 144 KB
    "win_128x3": (_cfg("NIFMultiScale", 128, 3, 64, 2, 1, 2, 1, 1), 160, "k_latent_to_w, ncw 3, rows_per_block 1"),
    "win_128x3_rpb2": (_cfg("NIFMultiScale", 128, 3, 64, 2, 1, 2, 1, 1), 3001, "k_latent_to_w, ncw 3, rows_per_block 2"),
    "win_res_64x2_r2": (_cfg("NIFMultiScale", 64, 2, 32, 2, 2, 2, 1, 1, s_res=True), 5001, "k_latent_to_w r = 2, ncw 2, rows_per_block 2"),
}


def _lr_for(m, spec, ws, B, seed=1):
    """latents from the hypernetwork (checked against the oracle on the first rows), spread to both signs"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, size=(B, spec.pi)).astype(np.float32)
    lr = m._engine.p_to_lr(p)
    k = min(B, 512)
    assert _rel(lr[:k], O.model_p_to_lr(spec, ws, p[:k].astype(np.float64))) < 1e-5
    return lr


@pytest.mark.parametrize("name", sorted(L2W))
def test_lr_to_w_host_entry_element_bound(name):
    cfg, B, _ = L2W[name]
    m, spec, ws = _model(cfg)
    lr = _lr_for(m, spec, ws, B)
    w = m._engine.lr_to_w(lr)
    assert w.shape == (B, spec.po)
    W, b = _last(spec, ws)
    e2, n2 = _check_w(w, lr, W, b)
    assert np.sqrt(e2 / n2) < 1e-6
    if B * spec.po <= 1 << 24:
        assert _rel(w, O.model_lr_to_w(spec, ws, lr.astype(np.float64))) < 1e-6


def _lr_to_w_dev(e, lr, po, w_off, lr_off):
    """nif_latent_to_w_dev with the output at float offset 4 + w_off and the latents at lr_off, sentinels on both sides;
    -> (w [B, po], whether every sentinel is untouched)"""
    from nif_amd.engine import DeviceArray
    B, r = lr.shape
    d_lr = DeviceArray(e, lr.size + lr_off)
    d_lr.upload(lr, lr_off)
    n = 4 + w_off + B * po + 8
    d_w = DeviceArray(e, n)
    d_w.upload(np.full(n, SENT, dtype=np.float32))
    check(e.lib.nif_latent_to_w_dev(e.ctx, d_lr.at(lr_off), B, d_w.at(4 + w_off)))
    full = d_w.download()
    d_w.free(); d_lr.free()
    pad = np.concatenate([full[:4 + w_off], full[4 + w_off + B * po:]])
    return full[4 + w_off:4 + w_off + B * po].reshape(B, po), bool(np.all(pad.view(np.uint32) == SENT.view(np.uint32)))


@pytest.mark.parametrize("name", ["flat_span_po195", "flat_span_po2209", "win_128x3"])
@pytest.mark.parametrize("w_off", [0, 1, 2, 3])
def test_lr_to_w_dev_entry_at_misaligned_pointers(name, w_off):
    """The output of the _dev entry at any float offset (both forms write 16-byte aligned units whatever the buffer's
    misalignment), the latents at another.  flat_span_po195 at offsets 2 and 3 is the case whose first thread started in front
    of the buffer and, on its second unit, took it for row 21 with a negative column: zeros in w[20, 193:195]."""
    cfg, B, _ = L2W[name]
    m, spec, ws = _model(cfg)
    e = m._engine
    lr = _lr_for(m, spec, ws, B)
    w, pad_ok = _lr_to_w_dev(e, lr, spec.po, w_off, (w_off + 1) % 4)
    W, b = _last(spec, ws)
    _check_w(w, lr, W, b)
    assert pad_ok, "nif_latent_to_w_dev wrote outside its output"
    host = e.lr_to_w(lr)
    assert np.array_equal(w.view(np.uint32), host.view(np.uint32))     # same summation order at any alignment


def _rows_of(d, po, lo, hi, off):
    return d.download((hi - lo) * po, off + lo * po).reshape(hi - lo, po)


def test_lr_to_w_and_given_w_past_2_to_the_31_floats():
    """bench.py's configs[1] net (po 16833) at 2^17 points: B po = 2.2e9 floats, so element indices cross 2^31 (what bench.py
    runs by default).  Only the rows around the crossing, the first and the last rows are downloaded and checked;
    then k_given_w<64> reads the same buffer (pt * po past 2^31) and u of those rows is checked against the oracle."""
    import bench
    from nif_amd.engine import DeviceArray
    m, spec, ws = _model(("NIFMultiScale", bench.CFG_SHAPE, bench.CFG_PARAM))
    e, po = m._engine, spec.po
    B, off = 1 << 17, 1 + 4
    rng = np.random.default_rng(3)
    p = rng.uniform(-1, 1, size=(B, 1)).astype(np.float32)
    xs = rng.uniform(-1, 1, size=(B, 1)).astype(np.float32)
    lr = e.p_to_lr(p)
    d_lr, d_x, d_u = DeviceArray(e, B), DeviceArray(e, B), DeviceArray(e, B)
    d_w = DeviceArray(e, off + B * po + 8)
    try:
        d_lr.upload(lr); d_x.upload(xs)
        d_w.upload(np.full(off, SENT, dtype=np.float32))
        d_w.upload(np.full(8, SENT, dtype=np.float32), off + B * po)
        check(e.lib.nif_latent_to_w_dev(e.ctx, d_lr.at(0), B, d_w.at(off)))
        check(e.lib.nif_shapenet_given_w_dev(e.ctx, d_x.at(0), d_w.at(off), B, d_u.at(0)))
        u = d_u.download()
        a31 = ((1 << 31) - off) // po                       # the row that holds float index 2^31 of the allocation
        assert 127570 <= a31 <= 127590
        W, b = _last(spec, ws)
        for lo, hi in [(0, 8), (127570, 127591), (B - 8, B)]:
            w = _rows_of(d_w, po, lo, hi, off)
            _check_w(w, lr[lo:hi], W, b, row0=lo)
            ref = O.shapenet_given_w(spec, xs[lo:hi].astype(np.float64), w.astype(np.float64))
            assert np.all(np.abs(u[lo:hi, None] - ref) <= 1e-5 * max(1.0, float(np.abs(ref).max()))), (lo, u[lo:hi], ref[:, 0])
        pads = np.concatenate([d_w.download(off, 0), d_w.download(8, off + B * po)])
        assert np.all(pads.view(np.uint32) == SENT.view(np.uint32))
    finally:
        for d in (d_w, d_lr, d_x, d_u):
            d.free()


def test_lr_to_w_tiny_net_with_a_large_latent():
    """8 units, latent_dim 64 (po 97) at 2^22 points: the flat form's latents in LDS (NR r floats beside the planes) were not
    counted, and an uncapped span asked for ~290 KB of LDS -- the launch failed.  Sampled rows against the bound."""
    from nif_amd.engine import DeviceArray
    m, spec, ws = _model(_cfg("NIFMultiScale", 8, 1, 16, 1, 64, 1, 1, 1))
    e, po = m._engine, spec.po
    assert po == 97
    B = 1 << 22
    rng = np.random.default_rng(4)
    lr = rng.standard_normal((B, 64), dtype=np.float32)
    d_lr, d_w = DeviceArray(e, lr.size), DeviceArray(e, 4 + B * po + 8)
    try:
        d_lr.upload(lr)
        d_w.upload(np.full(4, SENT, dtype=np.float32))
        d_w.upload(np.full(8, SENT, dtype=np.float32), 4 + B * po)
        check(e.lib.nif_latent_to_w_dev(e.ctx, d_lr.at(0), B, d_w.at(4)))
        W, b = _last(spec, ws)
        starts = [0, B // 3, B // 2 - 100, B - 1000] + sorted(rng.integers(0, B - 64, size=8).tolist())
        for lo in starts:
            hi = min(B, lo + 1000)
            _check_w(_rows_of(d_w, po, lo, hi, 4), lr[lo:hi], W, b, row0=lo)
        pads = np.concatenate([d_w.download(4, 0), d_w.download(8, 4 + B * po)])
        assert np.all(pads.view(np.uint32) == SENT.view(np.uint32))
    finally:
        d_w.free(); d_lr.free()


# ---- model_x_to_u_given_w -----------------------------------------------------------------------------------------------
# name: (cfg, B); the kernel is chosen by the width alone: k_given_w<32|64|128> ("t"), else k_given_w_generic ("g").  "res": the
# res_first / res_second branch; "nif": the skip connection (nif_skip) under another activation; g80 / g96 / g120: the lane + 64 < n
# half of the generic kernel; "grid_stride": B > 8192 = 2048 workgroups x 4 waves, so waves take a second point
GW = {
    "t32_si1_so1": (_cfg("NIFMultiScale", 32, 2, 32, 1, 1, 1, 1, 1), 77),
    "t32_res_si3_so2": (_cfg("NIFMultiScale", 32, 1, 32, 1, 1, 3, 2, 1, s_res=True), 3),
    "t32_nif_selu": (_cfg("NIF", 32, 3, 32, 1, 1, 2, 1, 1, act="selu"), 77),
    "t32_grid_stride": (_cfg("NIFMultiScale", 32, 2, 32, 1, 1, 1, 1, 1), 9001),
    "t64_si2_so3": (_cfg("NIFMultiScale", 64, 2, 32, 1, 1, 2, 3, 1), 77),
    "t64_res_si1": (_cfg("NIFMultiScale", 64, 2, 32, 1, 2, 1, 1, 1, s_res=True), 1),
    "t64_nif_gelu": (_cfg("NIF", 64, 2, 32, 1, 1, 2, 2, 1, act="gelu"), 77),
    "t128_si2": (_cfg("NIFMultiScale", 128, 2, 32, 1, 1, 2, 1, 1), 1),
    "t128_res_so2": (_cfg("NIFMultiScale", 128, 1, 32, 1, 1, 2, 2, 1, s_res=True), 77),
    "t128_nif_swish": (_cfg("NIF", 128, 1, 32, 1, 1, 3, 3, 1, act="swish"), 3),
    "g8_si2_so3": (_cfg("NIFMultiScale", 8, 2, 16, 1, 1, 2, 3, 1), 3),
    "g8_grid_stride": (_cfg("NIFMultiScale", 8, 2, 16, 1, 1, 2, 3, 1), 12001),
    "g30_nif_tanh": (_cfg("NIF", 30, 2, 20, 1, 2, 2, 2, 2, act="tanh"), 77),
    "g48_res": (_cfg("NIFMultiScale", 48, 2, 40, 1, 2, 2, 2, 1, s_res=True), 77),
    "g48_nif_selu": (_cfg("NIF", 48, 2, 32, 1, 1, 3, 1, 1, act="selu"), 3),
    "g80_res_so2": (_cfg("NIFMultiScale", 80, 1, 32, 1, 1, 2, 2, 1, s_res=True), 1),
    "g80_nif_swish": (_cfg("NIF", 80, 2, 32, 1, 2, 1, 1, 1, act="swish"), 77),
    "g96_si3": (_cfg("NIFMultiScale", 96, 2, 32, 1, 2, 3, 1, 1), 77),
    "g120_so3": (_cfg("NIFMultiScale", 120, 2, 32, 1, 1, 2, 3, 1), 77),
    "g120_nif_gelu": (_cfg("NIF", 120, 1, 32, 1, 1, 1, 2, 1, act="gelu"), 3),
}


def _gw_inputs(m, spec, B, source, seed=2):
    rng = np.random.default_rng(seed)
    xs = rng.uniform(-1, 1, size=(B, spec.si)).astype(np.float32)
    if source == "hyper":
        p = rng.uniform(-1, 1, size=(B, spec.pi)).astype(np.float32)
        w = m._engine.lr_to_w(m._engine.p_to_lr(p))
    else:
        w = (rng.standard_normal((B, spec.po)) * 0.01).astype(np.float32)    # test_given_w_arbitrary_weights' scale
    return xs, w


def _gw_ref(spec, xs, w, chunk=1024):
    return np.concatenate([O.shapenet_given_w(spec, xs[i:i + chunk].astype(np.float64), w[i:i + chunk].astype(np.float64))
                           for i in range(0, xs.shape[0], chunk)])


def _assert_u_bars(u, ref):
    """the existing bars of the path, met by every case below as they stand (hypernetwork w and random w at 0.01): per point
    |u - u64| <= 1e-5 max(1, max |u64|), whole tensor rel-L2 < 1e-5"""
    tol = 1e-5 * max(1.0, float(np.abs(ref).max()))
    err = np.abs(u.astype(np.float64) - ref)
    assert np.all(err <= tol), ("per point", float(err.max()), tol, np.unravel_index(int(np.argmax(err)), err.shape))
    assert _rel(u, ref) < 1e-5, ("rel-L2", _rel(u, ref))


def _given_w_dev(e, xs, w, so, offs):
    from nif_amd.engine import DeviceArray
    B = xs.shape[0]
    ox, ow, ou = offs
    d_x, d_w = DeviceArray(e, xs.size + ox), DeviceArray(e, w.size + ow)
    d_u = DeviceArray(e, 4 + ou + B * so + 8)
    d_x.upload(xs, ox); d_w.upload(w, ow)
    d_u.upload(np.full(d_u.n, SENT, dtype=np.float32))
    check(e.lib.nif_shapenet_given_w_dev(e.ctx, d_x.at(ox), d_w.at(ow), B, d_u.at(4 + ou)))
    full = d_u.download()
    for d in (d_x, d_w, d_u):
        d.free()
    pad = np.concatenate([full[:4 + ou], full[4 + ou + B * so:]])
    return full[4 + ou:4 + ou + B * so].reshape(B, so), bool(np.all(pad.view(np.uint32) == SENT.view(np.uint32)))


@pytest.mark.parametrize("source", ["hyper", "random"])
@pytest.mark.parametrize("name", sorted(GW))
def test_given_w_matches_oracle_and_is_bitwise_consistent(name, source):
    cfg, B = GW[name]
    m, spec, ws = _model(cfg)
    e = m._engine
    xs, w = _gw_inputs(m, spec, B, source)
    u = e.x_to_u_given_w(xs, w)
    assert u.shape == (B, spec.so)
    _assert_u_bars(u, _gw_ref(spec, xs, w))
    # the _dev entry at misaligned x, w and u, a sentinel around u
    for offs in [(1, 2, 3), (2, 3, 1), (3, 1, 2)]:
        ud, pad_ok = _given_w_dev(e, xs, w, spec.so, offs)
        assert pad_ok, ("nif_shapenet_given_w_dev wrote outside u", offs)
        assert np.array_equal(ud.view(np.uint32), u.view(np.uint32)), offs
    # points are independent rows: a permutation permutes u exactly, one row alone is the same row inside the batch
    perm = np.random.default_rng(9).permutation(B)
    assert np.array_equal(e.x_to_u_given_w(xs[perm], w[perm]).view(np.uint32), u[perm].view(np.uint32))
    i = B // 2
    assert np.array_equal(e.x_to_u_given_w(xs[i:i + 1], w[i:i + 1]).view(np.uint32), u[i:i + 1].view(np.uint32))


@pytest.mark.parametrize("name", ["ll_plain_32x2_r3", "ll_cfg4_128x2_r10_so3"])
def test_last_layer_class_phi_and_given_w_past_one_grid(name):
    """The last-layer class: x -> phi (k_pnet) and u = Dot(phi, w) + bias (k_pnet + k_ll_out) at B > 8192, with the bars of
    test_last_layer_class_submodels."""
    from tests.test_gpu_parity import CONFIGS
    cfg, _ = CONFIGS[name]
    m, spec, ws = _model(cfg)
    B = 9001
    rng = np.random.default_rng(6)
    p = rng.uniform(-1, 1, size=(B, spec.pi)).astype(np.float32)
    xs = rng.uniform(-1, 1, size=(B, spec.si)).astype(np.float32)
    lr = m.model_p_to_lr().predict(p)
    assert _rel(lr, O.model_p_to_lr(spec, ws, p.astype(np.float64))) < 1e-5
    phi = m.model_x_to_phi().predict(xs)
    assert phi.shape == (B, spec.so, spec.r)
    assert _rel(phi, O.model_x_to_phi(spec, ws, xs.astype(np.float64))) < 1e-5
    u = m.model_x_to_u_given_w().predict([xs, lr])
    ref = np.einsum("bsj,bj->bs", phi.astype(np.float64), lr.astype(np.float64)) + ws[-1]
    assert _rel(u, ref) < 1e-5
    ws_rand = (rng.standard_normal((B, spec.r))).astype(np.float32)
    u2 = m._engine.x_to_u_given_w(xs, ws_rand)
    ref2 = np.einsum("bsj,bj->bs", phi.astype(np.float64), ws_rand.astype(np.float64)) + ws[-1]
    assert _rel(u2, ref2) < 1e-5
