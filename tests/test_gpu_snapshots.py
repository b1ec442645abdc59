"""Model.predict_snapshots on the device: T snapshots, one ParameterNet input (or one latent vector) per mesh, against the fp64 oracle on
the expanded table -- per snapshot, at the project's forward bar (test_forward_matches_oracle: rel-L2 < 1e-5) -- and against
model.predict, plus the call's neighbours in the C-ABI (weights, a deferred optimizer tail, a graph capture)."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from tests.test_gpu_parity import _make, _make_policy, _rel

pytestmark = pytest.mark.gpu

BAR = 1e-5
NETS = ["nif_cfg1_32x2", "nif_pad_n30_tanh_r2_so2", "ms_cfg2_64x4", "ms_64x2_mlp_pnet_r3", "ms_32x2_r7_si3", "ms_res_48x2_pres",
        "ms_cfg3_128x3", "ll_plain_32x2_r3", "ll_cfg4_128x2_r10_so3"]
CASES = NETS + ["ms_cfg2_64x4/mixed_bfloat16"]
RAGGED = [1, 7, 64, 257, 33]       # a single point, partial tiles, an exact tile multiple, tile + 1
SHARED_T, SHARED_M = 3, 100

_cache = {}


def _setup(case):
    """model + inputs + fp64 references of a case, built once and shared by the tests (nothing below writes into them)"""
    if case in _cache:
        return _cache[case]
    name, _, policy = case.partition("/")
    m, model, spec, ws, _, _, _ = _make_policy(name, policy, boost=2.0) if policy else _make(name)
    rng = np.random.default_rng(7)
    T = len(RAGGED)
    p = rng.uniform(-1, 1, size=(T, spec.pi)).astype(np.float32)              # distinct per snapshot: a mixed-up image is an O(1) error
    xs = [rng.uniform(-1, 1, size=(n, spec.si)).astype(np.float32) for n in RAGGED]
    xsh = rng.uniform(-1, 1, size=(SHARED_M, spec.si)).astype(np.float32)

    def table(t, x):
        return np.hstack([np.tile(p[t], (x.shape[0], 1)), x])

    d = dict(m=m, model=model, spec=spec, ws=ws, p=p, xs=xs, xsh=xsh, table=table)
    if not policy:
        d["ref_ragged"] = [O.forward(spec, ws, table(t, xs[t]).astype(np.float64)) for t in range(T)]
        d["ref_shared"] = [O.forward(spec, ws, table(t, xsh).astype(np.float64)) for t in range(SHARED_T)]
    _cache[case] = d
    return d


def _latent_ref(spec, ws, lat, x):
    lat64 = np.tile(lat.astype(np.float64), (x.shape[0], 1))
    if spec.kind == "NIFMultiScaleLastLayerParameterized":
        return np.einsum("bsj,bj->bs", O.model_x_to_phi(spec, ws, x.astype(np.float64)), lat64) + ws[-1]
    return O.shapenet_given_w(spec, x.astype(np.float64), O.model_lr_to_w(spec, ws, lat64))


@pytest.mark.parametrize("name", NETS)
def test_p_path_matches_the_oracle_snapshot_by_snapshot(name):
    d = _setup(name)
    ragged = d["model"].predict_snapshots(d["xs"], p=d["p"])
    shared = d["model"].predict_snapshots(d["xsh"], p=d["p"][:SHARED_T])
    assert shared.shape == (SHARED_T, SHARED_M, d["spec"].so) and shared.dtype == np.float32
    errs = [_rel(u, ref) for u, ref in zip(ragged, d["ref_ragged"])] + [_rel(shared[t], d["ref_shared"][t]) for t in range(SHARED_T)]
    print("snapshots p= %s: worst rel-L2 %.3g  (per snapshot: %s)" % (name, max(errs), " ".join("%.2g" % e for e in errs)))
    for t, u in enumerate(ragged):
        assert u.shape == (RAGGED[t], d["spec"].so) and u.dtype == np.float32
    assert max(errs) < BAR, errs


@pytest.mark.parametrize("name", NETS)
def test_latent_path_matches_the_oracle_on_the_same_float32_latents(name):
    d = _setup(name)
    spec, ws = d["spec"], d["ws"]
    lat = d["m"].model_p_to_lr().predict(d["p"])
    assert lat.shape == (len(RAGGED), spec.r) and lat.dtype == np.float32
    ragged = d["model"].predict_snapshots(d["xs"], latent=lat)
    shared = d["model"].predict_snapshots(d["xsh"], latent=lat[:SHARED_T])
    errs = [_rel(ragged[t], _latent_ref(spec, ws, lat[t], d["xs"][t])) for t in range(len(RAGGED))]
    errs += [_rel(shared[t], _latent_ref(spec, ws, lat[t], d["xsh"])) for t in range(SHARED_T)]
    print("snapshots latent= %s: worst rel-L2 %.3g  (per snapshot: %s)" % (name, max(errs), " ".join("%.2g" % e for e in errs)))
    assert max(errs) < BAR, errs


def test_mixed_policy_falls_back_to_the_point_kernels_bit_for_bit():
    d = _setup("ms_cfg2_64x4/mixed_bfloat16")
    ragged = d["model"].predict_snapshots(d["xs"], p=d["p"])
    shared = d["model"].predict_snapshots(d["xsh"], p=d["p"][:SHARED_T])
    for t in range(len(RAGGED)):
        assert np.array_equal(ragged[t], d["model"].predict(d["table"](t, d["xs"][t])))
    for t in range(SHARED_T):
        assert np.array_equal(shared[t], d["model"].predict(d["table"](t, d["xsh"])))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("by", ["p", "latent"])
def test_permuting_the_snapshots_permutes_the_results_bit_for_bit(case, by):
    d = _setup(case)
    rows = d["p"] if by == "p" else d["m"].model_p_to_lr().predict(d["p"])
    perm = [3, 0, 4, 2, 1]
    kw = lambda r: {by: r}
    a = d["model"].predict_snapshots(d["xs"], **kw(rows))
    b = d["model"].predict_snapshots([d["xs"][i] for i in perm], **kw(rows[perm]))
    for j, i in enumerate(perm):
        assert np.array_equal(b[j], a[i]), (case, by, i)
    sa = d["model"].predict_snapshots(d["xsh"], **kw(rows))
    sb = d["model"].predict_snapshots(d["xsh"], **kw(rows[perm]))
    assert np.array_equal(sb, sa[perm])


@pytest.mark.parametrize("case", CASES)
def test_chunked_calls_are_bit_identical_to_the_unchunked_call(case, monkeypatch):
    from nif_amd.model import Model
    d = _setup(case)
    whole = d["model"].predict_snapshots(d["xs"], p=d["p"])
    whole_s = d["model"].predict_snapshots(d["xsh"], p=d["p"])
    e, calls = d["m"]._engine, []
    orig = e.forward_snapshots_ragged
    monkeypatch.setattr(e, "forward_snapshots_ragged", lambda rows, lat, xs: (calls.append([a.shape[0] for a in xs]), orig(rows, lat, xs))[1])
    s = d["spec"]
    per_point = 4 * (s.pi + s.si + s.so + s.r * (1 + (s.so if s.kind == "NIFMultiScaleLastLayerParameterized" else 0)))
    monkeypatch.setattr(Model, "_SNAPSHOT_CHUNK_BYTES", 100 * per_point)       # 100 points per chunk
    e.set_option("snapshot_image_bytes", 1)                                     # ... and one snapshot image at a time inside the library
    try:
        parts = d["model"].predict_snapshots(d["xs"], p=d["p"])
        parts_s = d["model"].predict_snapshots(d["xsh"], p=d["p"])
    finally:
        e.set_option("snapshot_image_bytes", 0)
    assert calls == [[1, 7, 64], [100], [100], [57, 33]]                        # T = 5 in four chunks, the long snapshot cut twice
    for a, b in zip(parts, whole):
        assert np.array_equal(a, b)
    assert np.array_equal(parts_s, whole_s)


STATE_NETS = ["nif_cfg1_32x2", "ms_cfg2_64x4", "ms_64x2_mlp_pnet_r3", "ll_plain_32x2_r3"]


@pytest.mark.parametrize("name", STATE_NETS)
def test_predict_is_untouched_and_new_weights_are_followed(name):
    m, model, spec, ws, x, y, sw = _make(name)           # a model of its own: this test writes weights
    d = _setup(name)
    before = model.predict(x)
    u0 = model.predict_snapshots(d["xs"], p=d["p"])
    assert np.array_equal(model.predict(x), before)
    assert np.array_equal(O.flatten(model.get_weights()), O.flatten([w.astype(np.float32) for w in ws]))
    ws2 = [(w * 1.25).astype(np.float32) for w in ws]
    model.set_weights(ws2)
    u1 = model.predict_snapshots(d["xs"], p=d["p"])
    ws2_64 = [w.astype(np.float64) for w in ws2]
    for t in range(len(RAGGED)):
        ref = O.forward(spec, ws2_64, d["table"](t, d["xs"][t]).astype(np.float64))
        assert _rel(u1[t], ref) < BAR, (t, _rel(u1[t], ref))
    assert not np.array_equal(u1[3], u0[3])


@pytest.mark.parametrize("name", STATE_NETS)
def test_call_behind_a_deferred_optimizer_tail_sees_the_updated_weights(name):
    """Adam(1e-3), the step tests/test_gpu_tail.py takes for the same call order.  A 1e-2 step moves every weight of the omega_0 = 30
    SIREN nets by 1e-2 and leaves the regime the forward bar is stated for: at those weights model.predict itself measured 1.8e-4 /
    2.5e-5 against the oracle on ms_cfg2_64x4 (this call 2.1e-5); at 1e-3 both are <= 2.1e-6 on every net here."""
    import nif_amd
    m, model, spec, ws, x, y, sw = _make(name)
    d = _setup(name)
    e = m._engine
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    e.loss_grad_dev(d_x.at(0), d_y.at(0), None, x.shape[0], x.shape[0])          # fused tail on (the default): the reduction waits
    e.adam_step_dev(nif_amd.Adam(1e-3).as_struct())
    u = model.predict_snapshots(d["xs"], p=d["p"])
    ws_now = [w.astype(np.float64) for w in model.get_weights()]
    assert not np.array_equal(O.flatten(ws_now), O.flatten(ws))
    for t in range(len(RAGGED)):
        ref = O.forward(spec, ws_now, d["table"](t, d["xs"][t]).astype(np.float64))
        assert _rel(u[t], ref) < BAR, (t, _rel(u[t], ref))


def test_call_inside_a_graph_capture_is_refused():
    from nif_amd._lib import NifError
    m, model, spec, ws, x, y, sw = _make("ms_cfg2_64x4")
    d = _setup("ms_cfg2_64x4")
    import ctypes as C
    model.predict(x)                                     # (planes packed, workspaces sized: the capture itself has nothing to refuse)
    e, s = m._engine, spec
    d_p, d_x, d_u = e.alloc(d["p"].size), e.alloc(d["xsh"].size), e.alloc(len(RAGGED) * SHARED_M * s.so)
    d_p.upload(d["p"]); d_x.upload(d["xsh"])
    off = np.array([0, 30, 60, 80, 90, 100], dtype=np.int64)
    e.graph_begin()
    try:
        with pytest.raises(NifError):
            model.predict_snapshots(d["xsh"], p=d["p"])
        with pytest.raises(NifError):
            model.predict_snapshots(d["xs"], p=d["p"])
        # the library's own refusal, on operands that were resident before the capture began
        assert e.lib.nif_forward_snapshots_dev(e.ctx, d_p.at(0), 0, len(RAGGED), d_x.at(0), None, SHARED_M, d_u.at(0)) == -4
        assert e.lib.nif_forward_snapshots_dev(e.ctx, d_p.at(0), 0, len(RAGGED), d_x.at(0), off.ctypes.data_as(C.POINTER(C.c_int64)), 0,
                                               d_u.at(0)) == -4
    finally:
        e.graph_end()
    assert _rel(model.predict_snapshots(d["xsh"], p=d["p"][:1])[0], d["ref_shared"][0]) < BAR


FRONT_T, FRONT_M = 2, 3
# the geometry faults every snapshot entry refuses in its shared front end: (rows, T, x, offsets) as the entry sees them -> the return
# code and the message, {who} the entry's name
FRONT_FAULTS = {
    "no_snapshots": (dict(T=0), -1, "bad argument"),
    "offsets_start_at_one": (dict(offsets=[1, 3, 6]), -1, "bad argument"),
    "offsets_decrease": (dict(offsets=[0, 2, 1]), -1, "offsets must not decrease"),
    "null_rows": (dict(rows=None), -1, "bad argument"),
    "points_without_coordinates": (dict(x=None), -1, "bad argument"),
    "inside_a_capture": (dict(capture=True), -4, "{who}: not capturable (inside nif_graph_begin / nif_graph_end)"),
}


@pytest.mark.parametrize("entry", ["nif_forward_snapshots", "nif_snapshot_normal_eq", "nif_snapshot_derivatives",
                                   "nif_snapshot_param_derivatives"])
def test_every_device_entry_refuses_the_same_geometry_faults_alike(entry):
    """host-side refusals of the four *_dev entries: nothing is launched between the valid call in front and the one behind"""
    import ctypes as C
    from nif_amd import _lib
    m, model, spec, ws, _, _, _ = _make("ms_32x2_r7_si3")
    e, n = m._engine, FRONT_T * FRONT_M
    rng = np.random.default_rng(11)
    latent = entry == "nif_snapshot_normal_eq"               # (its rows are latents; the others are given p)
    d_rows, d_x, d_y = e.alloc(FRONT_T * max(spec.pi, spec.r)), e.alloc(6 * spec.si), e.alloc(6 * spec.so)
    d_out, d_s = e.alloc(6 * spec.so * 4), e.alloc(2 * FRONT_T * (spec.r + 1) ** 2)        # (d_s: float64 [T, r + 1, r + 1])
    d_rows.upload(rng.uniform(-1, 1, size=FRONT_T * (spec.r if latent else spec.pi)))
    d_x.upload(rng.uniform(-1, 1, size=6 * spec.si)); d_y.upload(rng.uniform(-1, 1, size=6 * spec.so))
    idx = (C.c_int32 * 1)(0)

    def call(rows=d_rows.at(0), T=FRONT_T, x=d_x.at(0), offsets=None, capture=False):
        off = None if offsets is None else np.array(offsets, dtype=np.int64)
        off_p = None if off is None else off.ctypes.data_as(C.POINTER(C.c_int64))
        M = 0 if offsets is not None else FRONT_M
        if entry == "nif_forward_snapshots":
            return e.lib.nif_forward_snapshots_dev(e.ctx, rows, 0, T, x, off_p, M, d_out.at(0))
        if entry == "nif_snapshot_normal_eq":
            a = _lib.nif_encode_args()
            a.abi_version, a.latents, a.y, a.S_out = _lib.NIF_ENCODE_ABI_VERSION, rows, d_y.at(0), d_s.at(0)
        elif entry == "nif_snapshot_derivatives":
            a = _lib.nif_snapderiv_args()
            a.abi_version, a.order, a.rows = _lib.NIF_SNAPDERIV_ABI_VERSION, 1, rows
            a.y_idx, a.ny, a.x_idx, a.nx, a.u, a.dudx = idx, 1, idx, 1, d_out.at(0), d_out.at(6 * spec.so)
        else:
            a = _lib.nif_snapparam_args()
            a.abi_version, a.rows = _lib.NIF_SNAPPARAM_ABI_VERSION, rows
            a.y_idx, a.ny, a.p_idx, a.np, a.u, a.dudp = idx, 1, idx, 1, d_out.at(0), d_out.at(6 * spec.so)
        a.ctx, a.T, a.x, a.offsets_host, a.M = e.ctx, T, x, off_p, M
        return getattr(e.lib, entry + "_dev")(C.byref(a))

    assert call() == 0 and call(offsets=[0, 2, 6]) == 0     # (planes packed, workspaces sized: a capture has nothing else to refuse)
    for name, (fault, code, message) in FRONT_FAULTS.items():
        if fault.get("capture"):
            e.graph_begin()
        try:
            rc = call(**{k: v for k, v in fault.items() if k != "capture"})
            said = e.lib.nif_last_error().decode()
        finally:
            if fault.get("capture"):
                e.graph_end()
        assert (rc, said) == (code, message.format(who=entry)), (entry, name)
    assert call() == 0 and call(offsets=[0, 2, 6]) == 0
    e.sync()


def test_host_pointer_entry_equals_the_device_pointer_entry():
    import ctypes as C
    from nif_amd._lib import check, ptr
    d = _setup("ms_64x2_mlp_pnet_r3")
    e, s = d["m"]._engine, d["spec"]
    for offsets, x, n in ((None, d["xsh"], len(RAGGED) * SHARED_M),
                          (np.concatenate([[0], np.cumsum(RAGGED)]).astype(np.int64), np.concatenate(d["xs"]), sum(RAGGED))):
        out = np.empty((n, s.so), dtype=np.float32)
        check(e.lib.nif_forward_snapshots(e.ctx, ptr(d["p"]), 0, len(RAGGED), ptr(np.ascontiguousarray(x)),
                                          None if offsets is None else offsets.ctypes.data_as(C.POINTER(C.c_int64)), SHARED_M, ptr(out)))
        want = d["model"].predict_snapshots(d["xsh"] if offsets is None else d["xs"], p=d["p"])
        assert np.array_equal(out, np.concatenate(list(want)).reshape(n, s.so))
