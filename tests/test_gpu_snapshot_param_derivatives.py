"""Model.predict_snapshot_parameter_derivatives on the device: u and du/dp of T snapshots, one ParameterNet input (or one latent vector
with its directions) per mesh, against oracle.nif_oracle.hessian_analytic in fp64 on the expanded table, parameter columns -- per
snapshot, at the bars the point-wise layers hold for parameter columns in tests/deriv_cases.py (BAR_Y, BAR_J; whole tensor and per
point) -- against tests/encode_ref.field_and_jac along drawn directions, against JacobianLayer, plus the call's neighbours in the
C-ABI (weights, a deferred optimizer tail, a graph capture, refusals).  Weights as tests/deriv_cases.py draws them (_make(boost=1.0));
the wide last-layer case as tests/wide_ll_cases.py makes it."""
import ctypes as C

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests.deriv_cases import BAR_J, BAR_Y, SENT, Fenced, Ref, assert_bars, bits_equal
from tests.encode_ref import field_and_jac
from tests.test_gpu_parity import _make, _make_policy

pytestmark = pytest.mark.gpu

WIDE = "w129x1"
NETS = ["nif_pad_n30_tanh_r2_so2", "ms_32x2_r7_si3", "ms_res_48x2_pres", "ms_cfg3_128x3", "ll_plain_32x2_r3", "ll_cfg4_128x2_r10_so3", WIDE]
MIXED = "ms_cfg2_64x4/mixed_bfloat16"
CASES = NETS + [MIXED]
RAGGED = [1, 7, 64, 257, 33, 0]    # a single point, partial tiles, an exact tile multiple, tile + 1, an empty snapshot
SHARED_T, SHARED_M = 3, 100
ND = 7                             # directions of the latent= tests: three launches of 3 + 3 + 1 streams
NIF_ERR_INVALID, NIF_ERR_STATE = -1, -4

_cache = {}


def _build(case):
    name, _, policy = case.partition("/")
    if name == WIDE:
        from tests.wide_ll_cases import fresh
        return fresh(name)
    return _make_policy(name, policy) if policy else _make(name, boost=1.0)


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

    def table(t, x):
        return np.hstack([np.tile(p[t], (x.shape[0], 1)), x])

    d = dict(m=m, model=model, spec=spec, ws=ws, p=p, xs=xs, xsh=xsh, dirs=dirs, table=table, e=m._engine)
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


def _dzdp(d):
    """the float32 cast of the oracle's dz/dp [T, pi, r] at p (last-layer class: da/dp = dz/dp . last_w)"""
    if "dzdp" not in d:
        spec, ws = d["spec"], [np.asarray(w, dtype=np.float64) for w in d["ws"]]
        _, zd, _ = O.pnet_tangents(spec, ws, d["p"].astype(np.float64), list(range(spec.pi)))
        zd = np.stack(zd, axis=1)
        if spec.kind == O.KIND_LL:
            zd = zd @ O._pnet_split(spec, ws)[3][0]
        d["dzdp"] = zd.astype(np.float32)
    return d["dzdp"]


def _check(what, spec, ref, yi, cols, outs):
    """outs = (u, dudp) of one snapshot against the gather of its reference at the parameter columns `cols`"""
    py, pj, _ = ref.gather(yi, cols)
    assert_bars(what + " u", outs[0], py, BAR_Y)
    assert_bars(what + " dudp", outs[1], pj, BAR_J)


def _check_all(what, d, ragged, shared, yi, cols):
    spec = d["spec"]
    tails = [(spec.so,), (len(yi), len(cols))]
    for out, tail in zip(shared, tails):
        assert out.shape == (SHARED_T, SHARED_M) + tail and out.dtype == np.float32
    for t, n in enumerate(RAGGED):
        for out, tail in zip(ragged, tails):
            assert out[t].shape == (n,) + tail and out[t].dtype == np.float32
        if n:
            _check("%s ragged snapshot %d (%d points)" % (what, t, n), spec, d["ref_ragged"][t], yi, cols, [o[t] for o in ragged])
    for t in range(SHARED_T):
        _check("%s shared snapshot %d" % (what, t), spec, d["ref_shared"][t], yi, cols, [o[t] for o in shared])


def _all_idx(spec):
    return list(range(spec.so)), list(range(spec.pi))


@pytest.mark.parametrize("name", NETS)
def test_p_path_matches_the_oracle_snapshot_by_snapshot(name):
    d = _setup(name)
    yi, cols = _all_idx(d["spec"])
    f = d["model"].predict_snapshot_parameter_derivatives
    ragged = f(d["xs"], p=d["p"])
    shared = f(d["xsh"], p=d["p"][:SHARED_T])
    assert len(ragged) == len(shared) == 2
    _check_all("%s p=" % name, d, ragged, shared, yi, cols)


@pytest.mark.parametrize("name", NETS)
def test_latent_path_with_the_oracles_dzdp_matches_the_same_oracle(name):
    """latent= with the float32 latents of model_p_to_lr().predict(p) and dlatent = the float32 cast of the oracle's dz/dp, nd = pi:
    held to the reference of the p= path at the same bars"""
    d = _setup(name)
    yi, cols = _all_idx(d["spec"])
    lat, dz = _latents(d), _dzdp(d)
    f = d["model"].predict_snapshot_parameter_derivatives
    ragged = f(d["xs"], latent=lat, dlatent=dz)
    shared = f(d["xsh"], latent=lat[:SHARED_T], dlatent=dz[:SHARED_T])
    _check_all("%s latent= dz/dp" % name, d, ragged, shared, yi, cols)


@pytest.mark.parametrize("name", NETS)
def test_latent_path_along_seven_drawn_directions_matches_autograd_through_the_field(name):
    """nd = 7 directions in U(-1, 1): three launches of 3 + 3 + 1 streams on the weight-tangent kernel.  Reference: torch autograd
    through tests/encode_ref's restatement of the field at the same float32 latents, contracted with the directions in float64;
    bar: BAR_J relative to the reference's norm, per snapshot"""
    d = _setup(name)
    spec, ws = d["spec"], [np.asarray(w, dtype=np.float64) for w in d["ws"]]
    lat, dirs = _latents(d), d["dirs"]
    f = d["model"].predict_snapshot_parameter_derivatives
    ragged = f(d["xs"], latent=lat, dlatent=dirs)
    shared = f(d["xsh"], latent=lat[:SHARED_T], dlatent=dirs[:SHARED_T])
    assert shared[1].shape == (SHARED_T, SHARED_M, spec.so, ND)
    for what, xs_, got in (("ragged", d["xs"], ragged), ("shared", [d["xsh"]] * SHARED_T, shared)):
        for t, x in enumerate(xs_):
            assert got[1][t].shape == (x.shape[0], spec.so, ND) and got[1][t].dtype == np.float32
            if not x.shape[0]:
                continue
            u, J = field_and_jac(spec, ws, lat[t].astype(np.float64), x)
            want = np.einsum("msk,dk->msd", J, dirs[t].astype(np.float64))
            err = np.linalg.norm(got[1][t].astype(np.float64) - want) / np.linalg.norm(want)
            erru = np.linalg.norm(got[0][t].astype(np.float64) - u) / np.linalg.norm(u)
            print("%s %s snapshot %d: dudp rel-L2 %.3e (%.2f of the bar), u rel-L2 %.3e" % (name, what, t, err, err / BAR_J, erru))
            assert err < BAR_J, (name, what, t, err)


@pytest.mark.parametrize("name", NETS)
def test_index_forms_are_gathers_of_the_all_columns_result(name):
    """p_index=[c] alone and any y_index subset or order: gathers of the all-columns call, bit for bit"""
    d = _setup(name)
    spec = d["spec"]
    f = d["model"].predict_snapshot_parameter_derivatives
    yi = list(range(spec.so))[::-1] + [spec.so - 1]
    full = f(d["xs"], p=d["p"])
    full_s = f(d["xsh"], p=d["p"][:SHARED_T])
    for c in range(spec.pi):
        one = f(d["xs"], p=d["p"], p_index=[c], y_index=yi)
        one_s = f(d["xsh"], p=d["p"][:SHARED_T], p_index=[c], y_index=yi)
        for t in range(len(RAGGED)):
            assert bits_equal(one[0][t], full[0][t])
            assert bits_equal(one[1][t], full[1][t][:, yi][:, :, [c]]), (name, c, t)
        assert bits_equal(one_s[0], full_s[0]) and bits_equal(one_s[1], full_s[1][:, :, yi][:, :, :, [c]])
    if spec.pi > 1:
        cols = list(range(spec.pi))[::-1]
        rev = f(d["xs"], p=d["p"], p_index=cols)
        for t in range(len(RAGGED)):
            assert bits_equal(rev[1][t], full[1][t][:, :, cols]), (name, t)


@pytest.mark.parametrize("name", NETS)
def test_a_direction_does_not_depend_on_its_neighbours_and_scales_exactly(name):
    """direction d of an nd = 7 call equals the nd = 1 call with that direction (for every position inside a launch group), and
    doubling dlatent doubles dudp: a power of two is exact through every product"""
    d = _setup(name)
    lat, dirs = _latents(d), d["dirs"]
    f = d["model"].predict_snapshot_parameter_derivatives
    for x, sl in ((d["xs"], slice(None)), (d["xsh"], slice(0, SHARED_T))):
        seven = f(x, latent=lat[sl], dlatent=dirs[sl])
        for k in (0, 1, 2, 4, 6):
            one = f(x, latent=lat[sl], dlatent=dirs[sl][:, k:k + 1])
            for a, b, ua, ub in zip(one[1], seven[1], one[0], seven[0]):
                assert bits_equal(a, b[..., k:k + 1]), (name, k)
                assert bits_equal(ua, ub)
        twice = f(x, latent=lat[sl], dlatent=2.0 * dirs[sl])
        for a, b in zip(twice[1], seven[1]):
            assert bits_equal(a, 2.0 * np.asarray(b)), name


# (latent= is not built under a mixed policy: test_mixed_policy_with_latents_is_refused_and_predict_works_afterwards)
@pytest.mark.parametrize("case,by", [(c, "p") for c in CASES] + [(c, "latent") for c in NETS])
def test_permuting_the_snapshots_permutes_the_results_bit_for_bit(case, by):
    d = _setup(case)
    perm = [3, 0, 5, 4, 2, 1]
    f = d["model"].predict_snapshot_parameter_derivatives
    if by == "p":
        kw = lambda idx: dict(p=d["p"][idx])
    else:
        lat = _latents(d)
        kw = lambda idx: dict(latent=lat[idx], dlatent=d["dirs"][idx])
    ident = list(range(len(RAGGED)))
    a = f(d["xs"], **kw(ident))
    b = f([d["xs"][i] for i in perm], **kw(perm))
    sa = f(d["xsh"], **kw(ident))
    sb = f(d["xsh"], **kw(perm))
    for k in range(2):
        for j, i in enumerate(perm):
            assert bits_equal(b[k][j], a[k][i]), (case, by, k, i)
        assert bits_equal(sb[k], sa[k][perm]), (case, by, k)


@pytest.mark.parametrize("case,by", [(c, "p") for c in CASES] + [(c, "latent") for c in NETS])
def test_chunked_calls_are_bit_identical_to_the_unchunked_call(case, by, monkeypatch):
    from nif_amd.model import Model
    d = _setup(case)
    f = d["model"].predict_snapshot_parameter_derivatives
    kw = dict(p=d["p"]) if by == "p" else dict(latent=_latents(d), dlatent=d["dirs"])
    whole = f(d["xs"], **kw)
    whole_s = f(d["xsh"], **kw)
    e, calls = d["e"], []
    orig = e.snapshot_param_derivatives_ragged
    monkeypatch.setattr(e, "snapshot_param_derivatives_ragged", lambda rows, dr, xs, *a: (calls.append([x.shape[0] for x in xs]), orig(rows, dr, xs, *a))[1])
    monkeypatch.setattr(Model, "_SNAPSHOT_CHUNK_BYTES", 100)                    # below one point's bytes ...
    e.set_option("snapshot_image_bytes", 1)                                     # ... and one snapshot image at a time inside the library
    try:
        parts = f(d["xs"], batch_size=100, **kw)                                # 100 points per chunk
        parts_s = f(d["xsh"], batch_size=250, **kw)                             # two whole snapshots per chunk
    finally:
        e.set_option("snapshot_image_bytes", 0)
    assert calls == [[1, 7, 64], [100], [100], [57, 33]]                        # T = 6 in four chunks, the long snapshot cut twice
    for k in range(2):
        for a, b in zip(parts[k], whole[k]):
            assert bits_equal(a, b)
        assert bits_equal(parts_s[k], whole_s[k])


def test_mixed_policy_with_p_equals_the_jacobian_layer_bit_for_bit():
    import nif_amd
    d = _setup(MIXED)
    spec = d["spec"]
    yi, cols = _all_idx(spec)
    layer = nif_amd.JacobianLayer(d["model"], yi, cols)
    f = d["model"].predict_snapshot_parameter_derivatives
    ragged = f(d["xs"], p=d["p"])
    shared = f(d["xsh"], p=d["p"][:SHARED_T])
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
    lat = _latents(d)
    for mesh in (d["xsh"], d["xs"]):
        with pytest.raises(NifError) as ei:
            d["model"].predict_snapshot_parameter_derivatives(mesh, latent=lat, dlatent=d["dirs"])
        assert "not built" in str(ei.value) and "mixed_bfloat16" in str(ei.value)
    assert np.array_equal(d["model"].predict(x), before)


def _i32(idx):
    return (C.c_int32 * len(idx))(*[int(i) for i in idx])


def _args(e, rows, drows, nd, T, x, offsets, M, yi, pi_, u, dudp):
    """nif_snapparam_args over raw pointers (host or device); the index arrays and offsets stay alive on the struct.  drows None: rows
    are p rows with the columns pi_; else latents with nd directions each"""
    from nif_amd import _lib
    a = _lib.nif_snapparam_args()
    a.abi_version, a.ctx = _lib.NIF_SNAPPARAM_ABI_VERSION, e.ctx
    a.rows, a.rows_are_latent, a.T, a.x, a.M = rows, 0 if drows is None else 1, T, x, M
    a._keep = (_i32(yi), None if pi_ is None else _i32(pi_), offsets)
    a.offsets_host = None if offsets is None else offsets.ctypes.data_as(C.POINTER(C.c_int64))
    a.y_idx, a.ny = a._keep[0], len(yi)
    if drows is None:
        a.p_idx, a.np = a._keep[1], len(pi_)
    else:
        a.drows, a.nd = drows, nd
    a.u, a.dudp = u, dudp
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
    yi, cols = list(range(s.so))[::-1], list(range(s.pi))
    lat, dirs = np.ascontiguousarray(_latents(d)), np.ascontiguousarray(d["dirs"])
    f = d["model"].predict_snapshot_parameter_derivatives
    for offsets, x, n in _forms(d):
        mesh = d["xsh"] if offsets is None else d["xs"]
        for by in ("p", "latent"):
            nd = len(cols) if by == "p" else ND
            u, dj = np.empty((n, s.so), np.float32), np.empty((n, len(yi), nd), np.float32)
            if by == "p":
                a = _args(e, ptr(d["p"]), None, 0, len(RAGGED), ptr(x), offsets, SHARED_M, yi, cols, ptr(u), ptr(dj))
                want = f(mesh, p=d["p"], y_index=yi)
            else:
                a = _args(e, ptr(lat), ptr(dirs), ND, len(RAGGED), ptr(x), offsets, SHARED_M, yi, None, ptr(u), ptr(dj))
                want = f(mesh, latent=lat, dlatent=dirs, y_index=yi)
            check(e.lib.nif_snapshot_param_derivatives(C.byref(a)))
            for got, w in zip((u, dj), want):
                assert bits_equal(got, np.concatenate(list(w)).reshape(got.shape)), (name, by, offsets is None)


@pytest.mark.parametrize("name", ["nif_pad_n30_tanh_r2_so2", "ms_cfg3_128x3", "ll_cfg4_128x2_r10_so3", WIDE])
def test_dev_entry_writes_inside_its_outputs(name):
    """u and dudp at float offsets 1 and 2 from a 16-byte boundary, each with 32 of its rows of sentinel behind it (a tile's tail past a
    snapshot's last point would land in the next snapshot or there): every pad word untouched, the results the model's"""
    from nif_amd.engine import DeviceArray
    d = _setup(name)
    e, s = d["e"], d["spec"]
    yi, cols = _all_idx(s)
    lat, dirs = _latents(d), d["dirs"]
    f = d["model"].predict_snapshot_parameter_derivatives
    for offsets, x, n in _forms(d):
        mesh = d["xsh"] if offsets is None else d["xs"]
        for by in ("p", "latent"):
            nd = len(cols) if by == "p" else ND
            rows = d["p"] if by == "p" else lat
            d_r, d_d, d_x = DeviceArray(e, rows.size), DeviceArray(e, dirs.size), DeviceArray(e, x.size)
            d_r.upload(rows); d_d.upload(dirs); d_x.upload(x)
            fu, fj = Fenced(e, n, s.so, 1), Fenced(e, n, len(yi) * nd, 2)
            try:
                a = _args(e, d_r.at(0), None if by == "p" else d_d.at(0), nd, len(RAGGED), d_x.at(0), offsets, SHARED_M, yi,
                          cols if by == "p" else None, fu.at(), fj.at())
                rc = e.lib.nif_snapshot_param_derivatives_dev(C.byref(a))
                e.sync()
            finally:
                u, oku = fu.take((n, s.so))
                J, okj = fj.take((n, len(yi), nd))
                d_r.free(); d_d.free(); d_x.free()
            assert rc == 0, e.lib.nif_last_error()
            assert (oku, okj) == (True, True), (name, by, offsets is None, "wrote outside (u, dudp)")
            assert not np.any(u.view(np.uint32) == SENT.view(np.uint32)) and not np.any(J.view(np.uint32) == SENT.view(np.uint32))
            want = f(mesh, p=d["p"]) if by == "p" else f(mesh, latent=lat, dlatent=dirs)
            for got, w in zip((u, J), want):
                assert bits_equal(got, np.concatenate(list(w)).reshape(got.shape))


def test_the_c_abi_refuses_what_the_header_says_it_refuses():
    from nif_amd._lib import ptr
    d = _setup("ms_res_48x2_pres")
    e, s = d["e"], d["spec"]
    yi, cols = _all_idx(s)
    T, n = len(RAGGED), len(RAGGED) * SHARED_M
    lat, dirs = np.ascontiguousarray(_latents(d)), np.ascontiguousarray(d["dirs"])
    u, dj = np.empty((n, s.so), np.float32), np.empty((n, s.so, max(s.pi, ND)), np.float32)

    def call(latent=False, yi=yi, pi_=cols, **fields):
        if latent:
            a = _args(e, ptr(lat), ptr(dirs), ND, T, ptr(d["xsh"]), None, SHARED_M, yi, None, ptr(u), ptr(dj))
        else:
            a = _args(e, ptr(d["p"]), None, 0, T, ptr(d["xsh"]), None, SHARED_M, yi, pi_, ptr(u), ptr(dj))
        for k, v in fields.items():
            setattr(a, k, v)
        rc = e.lib.nif_snapshot_param_derivatives(C.byref(a))
        return rc, e.lib.nif_last_error().decode()

    assert call()[0] == 0
    flat = lambda: dj.reshape(-1)[:n * s.so * s.pi].copy()                      # (the p= call fills [n, so, pi] at the front of dj)
    good = u.copy(), flat()
    assert call(latent=True)[0] == 0
    keep = _i32([0])
    refused = [
        (dict(abi_version=2), "abi_version"),
        (dict(reserved0=1), "reserved"),
        (dict(latent=True, reserved0=1), "reserved"),
        (dict(latent=True, drows=None), "need drows"),                           # latents without directions
        (dict(drows=ptr(dirs)), "go with latent rows"),                          # directions with p rows
        (dict(nd=1), "go with latent rows"),
        (dict(latent=True, p_idx=keep, np=1), "not with latents"),               # parameter columns with latents
        (dict(latent=True, nd=0), "1 to 16 directions"),
        (dict(latent=True, nd=17), "1 to 16 directions"),
        (dict(np=0), "1 to 16 parameter columns"),
        (dict(np=17), "1 to 16 parameter columns"),
        (dict(p_idx=None), "1 to 16 parameter columns"),
        (dict(pi_=[s.pi]), "p_index out of range"),
        (dict(pi_=[-1]), "p_index out of range"),
        (dict(pi_=[0, 0]), "repeated"),
        (dict(yi=[s.so]), "y_index out of range"),
        (dict(yi=[-1]), "y_index out of range"),
        (dict(yi=[0] * 17), "at most 16 entries"),
    ]
    for kw, msg in refused:
        rc, err = call(**kw)
        assert rc == NIF_ERR_INVALID and msg in err, (kw, rc, err)
    a = _args(e, ptr(d["p"]), None, 0, T, ptr(d["xsh"]), None, SHARED_M, yi, cols, ptr(u), ptr(dj))
    a.reserved[3] = 7
    assert e.lib.nif_snapshot_param_derivatives(C.byref(a)) == NIF_ERR_INVALID
    assert call()[0] == 0 and bits_equal(u, good[0]) and bits_equal(flat(), good[1])
    x = d["table"](0, d["xsh"])
    assert d["model"].predict(x).shape == (SHARED_M, s.so)                       # the context is as usable as before


STATE_NETS = ["ms_res_48x2_pres", "ll_plain_32x2_r3"]


@pytest.mark.parametrize("name", STATE_NETS)
def test_call_behind_a_deferred_optimizer_tail_and_after_set_weights_sees_the_new_weights(name):
    """Adam(1e-3), the step tests/test_gpu_snapshots.py takes for the same call order (its docstring: why not 1e-2)"""
    import nif_amd
    m, model, spec, ws, x, y, sw = _make(name, boost=1.0)          # a model of its own: this test writes weights
    d = _setup(name)
    yi, cols = _all_idx(spec)
    e = m._engine
    f = model.predict_snapshot_parameter_derivatives
    u0 = f(d["xsh"], p=d["p"][:SHARED_T])
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    e.loss_grad_dev(d_x.at(0), d_y.at(0), None, x.shape[0], x.shape[0])          # fused tail on (the default): the reduction waits
    e.adam_step_dev(nif_amd.Adam(1e-3).as_struct())
    u1 = f(d["xsh"], p=d["p"][:SHARED_T])
    ws_now = [w.astype(np.float64) for w in model.get_weights()]
    assert not np.array_equal(O.flatten(ws_now), O.flatten(ws)) and not bits_equal(u1[1], u0[1])
    for t in range(SHARED_T):
        _check("%s behind the tail, snapshot %d" % (name, t), spec, Ref(spec, ws_now, d["table"](t, d["xsh"])), yi, cols, [o[t] for o in u1])
    ws2 = [(w * 1.125).astype(np.float32) for w in ws]
    model.set_weights(ws2)
    u2 = f(d["xsh"], p=d["p"][:1])
    _check("%s after set_weights" % name, spec, Ref(spec, [w.astype(np.float64) for w in ws2], d["table"](0, d["xsh"])), yi, cols, [o[0] for o in u2])


def test_call_inside_a_graph_capture_is_refused_and_the_context_stays_usable():
    from nif_amd._lib import NifError
    m, model, spec, ws, x, y, sw = _make("ms_res_48x2_pres", boost=1.0)
    d = _setup("ms_res_48x2_pres")
    yi, cols = _all_idx(spec)
    f = model.predict_snapshot_parameter_derivatives
    good = f(d["xsh"], p=d["p"][:1])                                # (planes packed, workspaces sized before the capture)
    e = m._engine
    n = len(RAGGED) * SHARED_M
    d_p, d_x, d_o = e.alloc(d["p"].size), e.alloc(d["xsh"].size), e.alloc(n * (spec.so + len(yi) * len(cols)))
    d_p.upload(d["p"]); d_x.upload(d["xsh"])
    off = np.array([0, 30, 60, 80, 90, 95, 100], dtype=np.int64)
    e.graph_begin()
    try:
        with pytest.raises(NifError):
            f(d["xsh"], p=d["p"])
        with pytest.raises(NifError):
            f(d["xs"], p=d["p"])
        # the library's own refusal, on operands that were resident before the capture began
        for offsets in (None, off):
            a = _args(e, d_p.at(0), None, 0, len(RAGGED), d_x.at(0), offsets, SHARED_M, yi, cols, d_o.at(0), d_o.at(n * spec.so))
            assert e.lib.nif_snapshot_param_derivatives_dev(C.byref(a)) == NIF_ERR_STATE
            assert b"not capturable" in e.lib.nif_last_error()
    finally:
        e.graph_end()
    again = f(d["xsh"], p=d["p"][:1])
    assert all(bits_equal(a, b) for a, b in zip(again, good))


@pytest.mark.parametrize("name", ["ms_res_48x2_pres", "ms_cfg3_128x3", "ll_cfg4_128x2_r10_so3"])
def test_the_neighbours_give_bit_identical_results_before_and_after_a_call(name):
    """predict, predict_snapshots, predict_snapshot_derivatives, the derivative layers and one training step (loss and gradient
    norms of a step from the same weights)"""
    import nif_amd
    m, model, spec, ws, x, y, sw = _make(name, boost=1.0)          # a model of its own: the training steps write weights
    d = _setup(name)
    yi = list(range(spec.so))
    cols = list(range(spec.pi + spec.si))
    tab = d["table"](1, d["xsh"])
    lat = m.model_p_to_lr().predict(d["p"])
    ws32 = [np.asarray(w, dtype=np.float32) for w in model.get_weights()]
    e = m._engine

    def neighbours():
        model.set_weights(ws32)
        outs = ([model.predict(tab), model.predict_snapshots(d["xs"], p=d["p"])[3]] + list(model.predict_snapshot_derivatives(d["xsh"], p=d["p"], order=2))
                + list(nif_amd.JacobianLayer(model, yi, cols)(tab)) + list(nif_amd.HessianLayer(model, yi, cols)(tab)))
        d_x, d_y = e.alloc(x.size), e.alloc(y.size)
        d_x.upload(x); d_y.upload(y)
        e.set_opt_state(np.zeros(e.n_params, np.float32), np.zeros(e.n_params, np.float32), 0)      # the same first step every time
        e.loss_grad_dev(d_x.at(0), d_y.at(0), None, x.shape[0], x.shape[0])
        e.adam_step_dev(nif_amd.Adam(1e-3).as_struct())
        outs += [np.asarray(w) for w in model.get_weights()]
        d_x.free(); d_y.free()
        model.set_weights(ws32)
        return outs

    before = neighbours()
    f = model.predict_snapshot_parameter_derivatives
    for kw in (dict(p=d["p"]), dict(latent=lat, dlatent=d["dirs"])):
        f(d["xs"], **kw)
        f(d["xsh"], **kw)
        after = neighbours()
        assert len(before) == len(after) and all(bits_equal(a, b) for a, b in zip(before, after)), (name, sorted(kw))


def test_the_wide_last_layer_net_runs_where_the_coordinate_call_refuses():
    """the coordinate derivatives refuse ShapeNets wider than 128 units (they need phi'); du/dp of the last-layer class needs phi alone"""
    from nif_amd._lib import NifError
    d = _setup(WIDE)
    with pytest.raises(NifError):
        d["model"].predict_snapshot_derivatives(d["xsh"], p=d["p"])
    u, dudp = d["model"].predict_snapshot_parameter_derivatives(d["xsh"], p=d["p"][:SHARED_T])
    assert bits_equal(u, d["model"].predict_snapshots(d["xsh"], p=d["p"][:SHARED_T]))
