"""Model.predict_snapshot_derivatives on the device: u, du/dx and d2u/dx2 of T snapshots, one ParameterNet input (or one latent vector)
per mesh, against oracle.nif_oracle.hessian_analytic in fp64 on the expanded table -- per snapshot, at the bars the point-wise layers
hold in tests/deriv_cases.py (BAR_Y, BAR_J, hbar; whole tensor and per point) -- and against HessianLayer, plus the call's neighbours
in the C-ABI (weights, a deferred optimizer tail, a graph capture, refusals).  Weights as tests/deriv_cases.py draws them
(_make(boost=1.0)): the weights at which the point-wise layers are held to these bars."""
import ctypes as C

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests.deriv_cases import BAR_J, BAR_Y, SENT, Fenced, Ref, assert_bars, bits_equal, hbar
from tests.test_gpu_parity import _make, _make_policy

pytestmark = pytest.mark.gpu

NETS = ["nif_pad_n30_tanh_r2_so2", "ms_32x2_r7_si3", "ms_res_48x2_pres", "ms_cfg3_128x3", "ll_plain_32x2_r3", "ll_cfg4_128x2_r10_so3"]
MIXED = "ms_cfg2_64x4/mixed_bfloat16"
CASES = NETS + [MIXED]
RAGGED = [1, 7, 64, 257, 33, 0]    # a single point, partial tiles, an exact tile multiple, tile + 1, an empty snapshot
SHARED_T, SHARED_M = 3, 100
NIF_ERR_INVALID, NIF_ERR_STATE = -1, -4

_cache = {}


def _setup(case):
    """model + inputs + fp64 references of a case, built once and shared by the tests (nothing below writes into them)"""
    if case in _cache:
        return _cache[case]
    name, _, policy = case.partition("/")
    m, model, spec, ws, _, _, _ = _make_policy(name, policy) if policy else _make(name, boost=1.0)
    rng = np.random.default_rng(11)
    T = len(RAGGED)
    p = rng.uniform(-1, 1, size=(T, spec.pi)).astype(np.float32)              # distinct per snapshot: a mixed-up image is an O(1) error
    xs = [rng.uniform(-1, 1, size=(n, spec.si)).astype(np.float32) for n in RAGGED]
    xsh = rng.uniform(-1, 1, size=(SHARED_M, spec.si)).astype(np.float32)

    def table(t, x):
        return np.hstack([np.tile(p[t], (x.shape[0], 1)), x])

    d = dict(m=m, model=model, spec=spec, ws=ws, p=p, xs=xs, xsh=xsh, table=table, e=m._engine)
    if not policy:
        d["ref_ragged"] = [Ref(spec, ws, table(t, xs[t])) if RAGGED[t] else None for t in range(T)]
        d["ref_shared"] = [Ref(spec, ws, table(t, xsh)) for t in range(SHARED_T)]
    _cache[case] = d
    return d


def _check(what, spec, ref, yi, xi, outs):
    """outs = (u, dudx[, d2udx2]) of one snapshot against the gather of its reference; xi counts coordinates from 0"""
    cols = [spec.pi + j for j in xi]
    py, pj, ph = ref.gather(yi, cols)
    assert_bars(what + " u", outs[0], py, BAR_Y)
    assert_bars(what + " dudx", outs[1], pj, BAR_J)
    if len(outs) > 2:
        assert_bars(what + " d2udx2", outs[2], ph, hbar(spec, cols))
        assert np.array_equal(outs[2], np.swapaxes(outs[2], -1, -2)), what + ": d2udx2 is not bit-symmetric"


def _check_all(what, d, ragged, shared, yi, xi):
    spec = d["spec"]
    ny, nx = len(yi), len(xi)
    tails = [(spec.so,), (ny, nx), (ny, nx, nx)][:len(ragged)]
    for out, tail in zip(shared, tails):
        assert out.shape == (SHARED_T, SHARED_M) + tail and out.dtype == np.float32
    for t, n in enumerate(RAGGED):
        for out, tail in zip(ragged, tails):
            assert out[t].shape == (n,) + tail and out[t].dtype == np.float32
        if n:
            _check("%s ragged snapshot %d (%d points)" % (what, t, n), spec, d["ref_ragged"][t], yi, xi, [o[t] for o in ragged])
    for t in range(SHARED_T):
        _check("%s shared snapshot %d" % (what, t), spec, d["ref_shared"][t], yi, xi, [o[t] for o in shared])


def _all_idx(spec):
    return list(range(spec.so)), list(range(spec.si))


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", NETS)
def test_p_path_matches_the_oracle_snapshot_by_snapshot(name, order):
    d = _setup(name)
    yi, xi = _all_idx(d["spec"])
    ragged = d["model"].predict_snapshot_derivatives(d["xs"], p=d["p"], order=order)
    shared = d["model"].predict_snapshot_derivatives(d["xsh"], p=d["p"][:SHARED_T], order=order)
    assert len(ragged) == len(shared) == order + 1
    _check_all("%s p= order %d" % (name, order), d, ragged, shared, yi, xi)


@pytest.mark.parametrize("name", NETS)
def test_latent_path_matches_the_same_oracle(name):
    """latent= with the float32 latents of model_p_to_lr().predict(p), held to the reference of the p= path (the oracle's own
    ParameterNet in fp64) at the same bars"""
    d = _setup(name)
    yi, xi = _all_idx(d["spec"])
    lat = d["m"].model_p_to_lr().predict(d["p"])
    assert lat.shape == (len(RAGGED), d["spec"].r) and lat.dtype == np.float32
    ragged = d["model"].predict_snapshot_derivatives(d["xs"], latent=lat, order=2)
    shared = d["model"].predict_snapshot_derivatives(d["xsh"], latent=lat[:SHARED_T], order=2)
    _check_all("%s latent=" % name, d, ragged, shared, yi, xi)


@pytest.mark.parametrize("case", ["ll_plain_32x2_r3", "ll_cfg4_128x2_r10_so3", MIXED])
def test_order_1_returns_the_u_and_dudx_of_order_2_bit_for_bit_where_the_kernels_are_the_same(case):
    """the last-layer class and the point-wise fallback run the second-order kernels at either order (the hypernetwork classes
    run k_jac<.., SNAP> with three first-order streams at order 1: held to the bars by the p= test above)"""
    d = _setup(case)
    for x, p in ((d["xs"], d["p"]), (d["xsh"], d["p"][:SHARED_T])):
        o1 = d["model"].predict_snapshot_derivatives(x, p=p, order=1)
        o2 = d["model"].predict_snapshot_derivatives(x, p=p, order=2)
        for a, b in zip(o1, o2[:2]):
            for sa, sb in zip(a, b):
                assert bits_equal(sa, sb)


@pytest.mark.parametrize("name", NETS)
def test_index_forms_are_gathers_of_the_all_columns_result(name):
    """y_index reversed with a repeat, x_index a subset in non-natural order: the oracle's gather at the bars; the y_index gather alone
    (same x_index, same launches) bit for bit"""
    d = _setup(name)
    spec = d["spec"]
    yi = list(range(spec.so))[::-1] + [spec.so - 1]
    xi = list(range(spec.si))[::-1][:max(1, spec.si - 1)] if spec.si > 1 else [0]
    for order in (1, 2):
        ragged = d["model"].predict_snapshot_derivatives(d["xs"], p=d["p"], x_index=xi, y_index=yi, order=order)
        shared = d["model"].predict_snapshot_derivatives(d["xsh"], p=d["p"][:SHARED_T], x_index=xi, y_index=yi, order=order)
        _check_all("%s y_index %s x_index %s order %d" % (name, yi, xi, order), d, ragged, shared, yi, xi)
        full = d["model"].predict_snapshot_derivatives(d["xs"], p=d["p"], x_index=xi, order=order)
        for t in range(len(RAGGED)):
            assert bits_equal(ragged[0][t], full[0][t])
            assert bits_equal(ragged[1][t], full[1][t][:, yi])
            if order == 2:
                assert bits_equal(ragged[2][t], full[2][t][:, yi])


# (latent= is not built under a mixed policy: test_mixed_policy_with_latents_is_refused_and_predict_works_afterwards)
@pytest.mark.parametrize("case,by", [(c, "p") for c in CASES] + [(c, "latent") for c in NETS])
def test_permuting_the_snapshots_permutes_the_results_bit_for_bit(case, by):
    d = _setup(case)
    rows = d["p"] if by == "p" else d["m"].model_p_to_lr().predict(d["p"])
    perm = [3, 0, 5, 4, 2, 1]
    kw = lambda r: {by: r, "order": 2}
    a = d["model"].predict_snapshot_derivatives(d["xs"], **kw(rows))
    b = d["model"].predict_snapshot_derivatives([d["xs"][i] for i in perm], **kw(rows[perm]))
    sa = d["model"].predict_snapshot_derivatives(d["xsh"], **kw(rows))
    sb = d["model"].predict_snapshot_derivatives(d["xsh"], **kw(rows[perm]))
    for k in range(3):
        for j, i in enumerate(perm):
            assert bits_equal(b[k][j], a[k][i]), (case, by, k, i)
        assert bits_equal(sb[k], sa[k][perm]), (case, by, k)


@pytest.mark.parametrize("case", CASES)
def test_chunked_calls_are_bit_identical_to_the_unchunked_call(case, monkeypatch):
    from nif_amd.model import Model
    d = _setup(case)
    whole = d["model"].predict_snapshot_derivatives(d["xs"], p=d["p"], order=2)
    whole_s = d["model"].predict_snapshot_derivatives(d["xsh"], p=d["p"], order=2)
    e, calls = d["e"], []
    orig = e.snapshot_derivatives_ragged
    monkeypatch.setattr(e, "snapshot_derivatives_ragged", lambda rows, lat, xs, *a: (calls.append([x.shape[0] for x in xs]), orig(rows, lat, xs, *a))[1])
    monkeypatch.setattr(Model, "_SNAPSHOT_CHUNK_BYTES", 100)                    # below one point's bytes ...
    e.set_option("snapshot_image_bytes", 1)                                     # ... and one snapshot image at a time inside the library
    try:
        parts = d["model"].predict_snapshot_derivatives(d["xs"], p=d["p"], order=2, batch_size=100)      # 100 points per chunk
        parts_s = d["model"].predict_snapshot_derivatives(d["xsh"], p=d["p"], order=2, batch_size=250)   # two whole snapshots per chunk
    finally:
        e.set_option("snapshot_image_bytes", 0)
    assert calls == [[1, 7, 64], [100], [100], [57, 33]]                        # T = 6 in four chunks, the long snapshot cut twice
    for k in range(3):
        for a, b in zip(parts[k], whole[k]):
            assert bits_equal(a, b)
        assert bits_equal(parts_s[k], whole_s[k])


def test_mixed_policy_with_p_equals_the_hessian_layer_bit_for_bit():
    import nif_amd
    d = _setup(MIXED)
    spec = d["spec"]
    yi, xi = _all_idx(spec)
    layer = nif_amd.HessianLayer(d["model"], yi, [spec.pi + j for j in xi])
    ragged = d["model"].predict_snapshot_derivatives(d["xs"], p=d["p"], order=2)
    shared = d["model"].predict_snapshot_derivatives(d["xsh"], p=d["p"][:SHARED_T], order=2)
    for t, n in enumerate(RAGGED):
        if n:
            for got, want in zip([o[t] for o in ragged], layer(d["table"](t, d["xs"][t]))):
                assert bits_equal(got, want), t
    for t in range(SHARED_T):
        for got, want in zip([o[t] for o in shared], layer(d["table"](t, d["xsh"]))):
            assert bits_equal(got, want), t


def test_mixed_policy_with_latents_is_refused_and_predict_works_afterwards():
    from nif_amd._lib import NifError
    d = _setup(MIXED)
    x = d["table"](0, d["xsh"])
    before = d["model"].predict(x)
    lat = d["m"].model_p_to_lr().predict(d["p"])
    for mesh in (d["xsh"], d["xs"]):
        with pytest.raises(NifError) as ei:
            d["model"].predict_snapshot_derivatives(mesh, latent=lat)
        assert "not built" in str(ei.value) and "mixed_bfloat16" in str(ei.value)
    assert np.array_equal(d["model"].predict(x), before)


def _i32(idx):
    return (C.c_int32 * len(idx))(*[int(i) for i in idx])


def _args(e, order, rows, is_latent, T, x, offsets, M, yi, xi, u, dudx, d2):
    """nif_snapderiv_args over raw pointers (host or device); the index arrays and offsets stay alive on the struct"""
    from nif_amd import _lib
    a = _lib.nif_snapderiv_args()
    a.abi_version, a.order, a.ctx = _lib.NIF_SNAPDERIV_ABI_VERSION, order, e.ctx
    a.rows, a.rows_are_latent, a.T, a.x, a.M = rows, 1 if is_latent else 0, T, x, M
    a._keep = (_i32(yi), _i32(xi), offsets)
    a.offsets_host = None if offsets is None else offsets.ctypes.data_as(C.POINTER(C.c_int64))
    a.y_idx, a.ny, a.x_idx, a.nx = a._keep[0], len(yi), a._keep[1], len(xi)
    a.u, a.dudx, a.d2udx2 = u, dudx, d2
    return a


def _forms(d):
    """(offsets, x, n) of the shared and the ragged form over all len(RAGGED) rows of p"""
    off = np.concatenate([[0], np.cumsum(RAGGED)]).astype(np.int64)
    return ((None, np.ascontiguousarray(d["xsh"]), len(RAGGED) * SHARED_M), (off, np.ascontiguousarray(np.concatenate(d["xs"])), sum(RAGGED)))


@pytest.mark.parametrize("name", ["ms_res_48x2_pres", "ll_plain_32x2_r3"])
def test_host_pointer_entry_equals_the_device_pointer_entry(name):
    from nif_amd._lib import check, ptr
    d = _setup(name)
    e, s = d["e"], d["spec"]
    yi, xi = list(range(s.so))[::-1], list(range(s.si))
    ny, nx = len(yi), len(xi)
    for order in (1, 2):
        for offsets, x, n in _forms(d):
            u, dj, dh = np.empty((n, s.so), np.float32), np.empty((n, ny, nx), np.float32), np.empty((n, ny, nx, nx), np.float32)
            a = _args(e, order, ptr(d["p"]), False, len(RAGGED), ptr(x), offsets, SHARED_M, yi, xi, ptr(u), ptr(dj), ptr(dh) if order == 2 else None)
            check(e.lib.nif_snapshot_derivatives(C.byref(a)))
            want = d["model"].predict_snapshot_derivatives(d["xsh"] if offsets is None else d["xs"], p=d["p"], y_index=yi, x_index=xi, order=order)
            for got, w in zip((u, dj, dh), want):
                assert bits_equal(got, np.concatenate(list(w)).reshape(got.shape)), (name, order, offsets is None)


@pytest.mark.parametrize("name", ["nif_pad_n30_tanh_r2_so2", "ms_cfg3_128x3", "ll_cfg4_128x2_r10_so3"])
def test_dev_entry_writes_inside_its_outputs(name):
    """u, dudx and d2udx2 at float offsets 1, 2, 3 from a 16-byte boundary, each with 32 of its rows of sentinel behind it (a tile's tail
    past a snapshot's last point would land in the next snapshot or there): every pad word untouched, the results the model's"""
    from nif_amd.engine import DeviceArray
    d = _setup(name)
    e, s = d["e"], d["spec"]
    yi, xi = _all_idx(s)
    ny, nx = len(yi), len(xi)
    for offsets, x, n in _forms(d):
        d_p, d_x = DeviceArray(e, d["p"].size), DeviceArray(e, x.size)
        d_p.upload(d["p"]); d_x.upload(x)
        fu, fj, fh = Fenced(e, n, s.so, 1), Fenced(e, n, ny * nx, 2), Fenced(e, n, ny * nx * nx, 3)
        try:
            a = _args(e, 2, d_p.at(0), False, len(RAGGED), d_x.at(0), offsets, SHARED_M, yi, xi, fu.at(), fj.at(), fh.at())
            rc = e.lib.nif_snapshot_derivatives_dev(C.byref(a))
            e.sync()
        finally:
            u, oku = fu.take((n, s.so))
            J, okj = fj.take((n, ny, nx))
            H, okh = fh.take((n, ny, nx, nx))
            d_p.free(); d_x.free()
        assert rc == 0, e.lib.nif_last_error()
        assert (oku, okj, okh) == (True, True, True), (name, offsets is None, "wrote outside (u, dudx, d2udx2)")
        assert not np.any(u.view(np.uint32) == SENT.view(np.uint32)) and not np.any(H.view(np.uint32) == SENT.view(np.uint32))
        want = d["model"].predict_snapshot_derivatives(d["xsh"] if offsets is None else d["xs"], p=d["p"], order=2)
        for got, w in zip((u, J, H), want):
            assert bits_equal(got, np.concatenate(list(w)).reshape(got.shape))


def test_the_c_abi_refuses_what_the_header_says_it_refuses():
    from nif_amd._lib import ptr
    d = _setup("ms_res_48x2_pres")
    e, s = d["e"], d["spec"]
    yi, xi = _all_idx(s)
    n = len(RAGGED) * SHARED_M
    u, dj, dh = np.empty((n, s.so), np.float32), np.empty((n, s.so, s.si), np.float32), np.empty((n, s.so, s.si, s.si), np.float32)

    def call(order=2, yi=yi, xi=xi, **fields):
        a = _args(e, order, ptr(d["p"]), False, len(RAGGED), ptr(d["xsh"]), None, SHARED_M, yi, xi, ptr(u), ptr(dj), ptr(dh))
        for k, v in fields.items():
            setattr(a, k, v)
        rc = e.lib.nif_snapshot_derivatives(C.byref(a))
        return rc, e.lib.nif_last_error().decode()

    assert call()[0] == 0
    good = [x.copy() for x in (u, dj, dh)]
    refused = [
        (dict(abi_version=2), "abi_version"),
        (dict(reserved0=1), "reserved"),
        (dict(reserved1=1), "reserved"),
        (dict(reserved2=1), "reserved"),
        (dict(order=3), "order must be 1 or 2"),
        (dict(order=0), "order must be 1 or 2"),
        (dict(yi=[s.so]), "y_index out of range"),
        (dict(yi=[0] * 17), "at most 16 entries"),
        (dict(xi=[s.si]), "x_index out of range"),
        (dict(xi=[-1]), "x_index out of range"),
        (dict(xi=[0, 1, 0]), "repeated"),
    ]
    for kw, msg in refused:
        rc, err = call(**kw)
        assert rc == NIF_ERR_INVALID and msg in err, (kw, rc, err)
    a = _args(e, 2, ptr(d["p"]), False, len(RAGGED), ptr(d["xsh"]), None, SHARED_M, yi, xi, ptr(u), ptr(dj), ptr(dh))
    a.reserved[3] = 7
    assert e.lib.nif_snapshot_derivatives(C.byref(a)) == NIF_ERR_INVALID
    assert call()[0] == 0 and all(bits_equal(x, g) for x, g in zip((u, dj, dh), good))      # the context is as usable as before


STATE_NETS = ["ms_res_48x2_pres", "ll_plain_32x2_r3"]


@pytest.mark.parametrize("name", STATE_NETS)
def test_call_behind_a_deferred_optimizer_tail_and_after_set_weights_sees_the_new_weights(name):
    """Adam(1e-3), the step tests/test_gpu_snapshots.py takes for the same call order (its docstring: why not 1e-2)"""
    import nif_amd
    m, model, spec, ws, x, y, sw = _make(name, boost=1.0)          # a model of its own: this test writes weights
    d = _setup(name)
    yi, xi = _all_idx(spec)
    e = m._engine
    u0 = model.predict_snapshot_derivatives(d["xsh"], p=d["p"][:SHARED_T], order=2)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    e.loss_grad_dev(d_x.at(0), d_y.at(0), None, x.shape[0], x.shape[0])          # fused tail on (the default): the reduction waits
    e.adam_step_dev(nif_amd.Adam(1e-3).as_struct())
    u1 = model.predict_snapshot_derivatives(d["xsh"], p=d["p"][:SHARED_T], order=2)
    ws_now = [w.astype(np.float64) for w in model.get_weights()]
    assert not np.array_equal(O.flatten(ws_now), O.flatten(ws)) and not bits_equal(u1[1], u0[1])
    for t in range(SHARED_T):
        _check("%s behind the tail, snapshot %d" % (name, t), spec, Ref(spec, ws_now, d["table"](t, d["xsh"])), yi, xi, [o[t] for o in u1])
    ws2 = [(w * 1.125).astype(np.float32) for w in ws]
    model.set_weights(ws2)
    u2 = model.predict_snapshot_derivatives(d["xsh"], p=d["p"][:1], order=2)
    _check("%s after set_weights" % name, spec, Ref(spec, [w.astype(np.float64) for w in ws2], d["table"](0, d["xsh"])), yi, xi, [o[0] for o in u2])


def test_call_inside_a_graph_capture_is_refused_and_the_context_stays_usable():
    from nif_amd._lib import NifError
    m, model, spec, ws, x, y, sw = _make("ms_res_48x2_pres", boost=1.0)
    d = _setup("ms_res_48x2_pres")
    yi, xi = _all_idx(spec)
    ny, nx = len(yi), len(xi)
    good = model.predict_snapshot_derivatives(d["xsh"], p=d["p"][:1], order=2)      # (planes packed, workspaces sized before the capture)
    e = m._engine
    n = len(RAGGED) * SHARED_M
    d_p, d_x, d_o = e.alloc(d["p"].size), e.alloc(d["xsh"].size), e.alloc(n * (spec.so + ny * nx + ny * nx * nx))
    d_p.upload(d["p"]); d_x.upload(d["xsh"])
    off = np.array([0, 30, 60, 80, 90, 95, 100], dtype=np.int64)
    e.graph_begin()
    try:
        with pytest.raises(NifError):
            model.predict_snapshot_derivatives(d["xsh"], p=d["p"])
        with pytest.raises(NifError):
            model.predict_snapshot_derivatives(d["xs"], p=d["p"])
        # the library's own refusal, on operands that were resident before the capture began
        for offsets in (None, off):
            a = _args(e, 2, d_p.at(0), False, len(RAGGED), d_x.at(0), offsets, SHARED_M, yi, xi, d_o.at(0), d_o.at(n * spec.so),
                      d_o.at(n * (spec.so + ny * nx)))
            assert e.lib.nif_snapshot_derivatives_dev(C.byref(a)) == NIF_ERR_STATE
            assert b"not capturable" in e.lib.nif_last_error()
    finally:
        e.graph_end()
    again = model.predict_snapshot_derivatives(d["xsh"], p=d["p"][:1], order=2)
    assert all(bits_equal(a, b) for a, b in zip(again, good))


@pytest.mark.parametrize("name", ["ms_res_48x2_pres", "ms_cfg3_128x3", "ll_cfg4_128x2_r10_so3"])
def test_the_neighbours_give_bit_identical_results_before_and_after_a_call(name):
    import nif_amd
    d = _setup(name)
    model, spec = d["model"], d["spec"]
    yi = list(range(spec.so))
    cols = list(range(spec.pi + spec.si))
    x = d["table"](1, d["xsh"])

    def neighbours():
        return ([model.predict(x), model.predict_snapshots(d["xs"], p=d["p"])[3]] + list(nif_amd.JacobianLayer(model, yi, cols)(x))
                + list(nif_amd.HessianLayer(model, yi, cols)(x)))

    before = neighbours()
    for order in (1, 2):
        model.predict_snapshot_derivatives(d["xs"], p=d["p"], order=order)
        model.predict_snapshot_derivatives(d["xsh"], p=d["p"], order=order)
        after = neighbours()
        assert all(bits_equal(a, b) for a, b in zip(before, after)), (name, order)


def test_a_wide_last_layer_net_is_refused_with_the_128_unit_message_and_stays_usable():
    from nif_amd._lib import NifError
    from tests.wide_ll_cases import make
    m, model, spec, ws, x, y, sw = make("w144x2")
    before = model.predict(x)
    rng = np.random.default_rng(3)
    p = rng.uniform(-1, 1, size=(2, spec.pi)).astype(np.float32)
    mesh = rng.uniform(-1, 1, size=(40, spec.si)).astype(np.float32)
    for order in (1, 2):
        for xm in (mesh, [mesh, mesh[:7]]):
            with pytest.raises(NifError) as ei:
                model.predict_snapshot_derivatives(xm, p=p, order=order)
            assert "up to 128 units (this one has 144)" in str(ei.value)
    assert np.array_equal(model.predict(x), before)
    assert model.predict_snapshots(mesh, p=p).shape == (2, 40, spec.so)
