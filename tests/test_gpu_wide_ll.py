"""The last-layer class with a ShapeNet of 129..512 units (csrc/k_wide.hip: one dense layer per launch, tiled over a workgroup)
against the fp64 NumPy oracle, at the bars of tests/test_gpu_parity.py for the same quantities, plus the neighbours of the new path in
the C-ABI: deferred optimizer tail, set_weights, graph capture, snapshots, and the refusals at nif_create and of the derivative
layers.  Figures of an MI355X run: DESIGN 5.12."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from tests.snet6_domain import check_tensor_bars
from tests.test_gpu_parity import _cfg, _rel
from tests.wide_ll_cases import CASES, SMALL, fresh, make, ref_loss_grad

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_phi_and_submodels_match_oracle(name):
    m, model, spec, ws, x, y, sw = make(name)
    x64 = x.astype(np.float64)
    p, xs = x[:, :spec.pi], x[:, spec.pi:]
    u = model.predict(x)
    ref = O.forward(spec, ws, x64)
    phi = m.model_x_to_phi().predict(xs)
    phi_ref = O.model_x_to_phi(spec, ws, xs.astype(np.float64))
    lr = m.model_p_to_lr().predict(p)
    u3 = m.model_x_to_u_given_w().predict([xs, lr])
    ref3 = np.einsum("bsj,bj->bs", phi_ref, lr.astype(np.float64)) + ws[-1]
    print("%s: predict %.2e, x_to_phi %.2e, x_to_u_given_w %.2e" % (name, _rel(u, ref), _rel(phi, phi_ref), _rel(u3, ref3)))
    assert u.shape == ref.shape and u.dtype == np.float32
    assert phi.shape == (x.shape[0], spec.so, spec.r)
    assert _rel(u, ref) < 1e-5
    assert _rel(phi, phi_ref) < 1e-5
    assert _rel(u3, ref3) < 1e-5


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("weighted", [False, True])
def test_loss_and_grad_match_oracle(name, weighted):
    m, model, spec, ws, x, y, sw = make(name)
    loss, g = m._engine.loss_and_grad(x, y, sw if weighted else None)
    lref, gref = ref_loss_grad(name, weighted)
    check_tensor_bars(spec, loss, g, lref, gref, "%s %s" % (name, "weighted" if weighted else "plain"))


@pytest.mark.parametrize("loss", ["mae", "huber", "log_cosh"])
def test_the_other_keras_losses(loss):
    """the bars of test_compile_with_the_other_keras_losses, on the plain step (the Sobolev step is refused on a wide net)"""
    import nif_amd
    m, model, spec, ws, x, y, sw = fresh("w144x2")
    y = (3.0 * y).astype(np.float32)                       # |e| on both sides of Huber's delta
    model.compile(nif_amd.Adam(1e-3), loss)
    rl, rg = O.loss_and_grad(spec, ws, x.astype(np.float64), y.astype(np.float64), sw.astype(np.float64), loss=loss)
    ev = model.evaluate(x, y, sample_weight=sw)
    m._engine.set_loss(loss)
    l_, g_ = m._engine.loss_and_grad(x, y, sw)
    m._engine.set_loss("mse")
    print("%s: evaluate %.2e, loss %.2e" % (loss, abs(ev - rl) / abs(rl), abs(l_ - rl) / abs(rl)))
    assert abs(ev - rl) < 2e-5 * abs(rl)
    assert abs(l_ - rl) < 2e-5 * abs(rl), (l_, rl)
    ref, bar = O.flatten(rg), (3e-4 if loss != "mae" else 6e-4)
    off, gn = 0, np.linalg.norm(ref)
    for nm, shp in spec.param_shapes():
        k = int(np.prod(shp))
        err = np.linalg.norm(g_[off:off + k].astype(np.float64) - ref[off:off + k])
        assert err <= bar * np.linalg.norm(ref[off:off + k]) + 2e-6 * gn, (nm, err, np.linalg.norm(ref[off:off + k]), gn)
        off += k


@pytest.mark.parametrize("name", ["w144x2", "w256x3", "w320x0"])
def test_two_evaluations_are_bit_identical_and_halves_add_up(name):
    m, model, spec, ws, x, y, sw = make(name)
    e, B = m._engine, x.shape[0]
    l1, g1 = e.loss_and_grad(x, y, sw)
    l2, g2 = e.loss_and_grad(x, y, sw)
    assert l1 == l2 and np.array_equal(g1, g2)
    d_x, d_y, d_s = e.alloc(x.size), e.alloc(y.size), e.alloc(sw.size)
    d_x.upload(x); d_y.upload(y); d_s.upload(sw)
    h = B // 2
    parts = []
    for lo, hi in ((0, h), (h, B)):
        e.loss_grad_dev(d_x.at(lo * x.shape[1]), d_y.at(lo * y.shape[1]), d_s.at(lo), hi - lo, B)
        parts.append(e.grad_read())
    lsum, gsum = parts[0][0] + parts[1][0], parts[0][1].astype(np.float64) + parts[1][1]
    print("%s: halves against the whole: loss %.2e, flat gradient %.2e" % (name, abs(lsum - l1) / abs(l1), _rel(gsum, g1.astype(np.float64))))
    assert abs(lsum - l1) <= 2e-6 * abs(l1)
    assert _rel(gsum, g1.astype(np.float64)) < 3e-5


def test_adam_steps_follow_oracle():
    """test_adam_steps_follow_oracle of tests/test_gpu_parity.py on w144x2: three full-batch steps, each teacher-forced"""
    import nif_amd
    LR = 2e-3
    m, model, spec, ws, x, y, sw = fresh("w144x2")
    model.compile(nif_amd.Adam(learning_rate=LR), loss="mse")
    e = m._engine
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    f32 = lambda a: float(np.float32(a))
    worst = 0.0
    for t in range(1, 4):
        th0 = O.flatten(model.get_weights()).astype(np.float64)
        m0, v0, step0 = e.get_opt_state()
        assert step0 == t - 1
        hist = model.fit(x, y, epochs=1, batch_size=x.shape[0], shuffle=False, verbose=0)
        l, g = O.loss_and_grad(spec, O.unflatten(spec, th0), x64, y64)
        assert abs(hist.history["loss"][0] - l) <= 2e-5 * abs(l), (t, hist.history["loss"][0], l)
        gf = O.flatten(g)
        th1, m1, v1 = O.adam_step(th0, gf, m0.astype(np.float64), v0.astype(np.float64), t, lr=f32(LR), b1=f32(0.9), b2=f32(0.999),
                                  eps=f32(1e-7))
        got = O.flatten(model.get_weights())
        gm, gv, step1 = e.get_opt_state()
        assert step1 == t
        solid = np.ones_like(th0, dtype=bool)
        off = 0
        for gt in g:
            rms = np.sqrt(np.mean(gt ** 2)) + 1e-300
            solid[off:off + gt.size] = np.abs(gt.ravel()) > 0.02 * rms
            off += gt.size
        assert solid.mean() > 0.8
        d = np.abs(got - th1)
        worst = max(worst, d[solid].max() / LR)
        assert d[solid].max() < 0.01 * LR, (t, d[solid].max() / LR)
        assert d.max() <= 2.0 * LR * 1.001
        assert _rel(gm, m1) < 1e-3
        assert _rel(gv, v1) < 1e-3
    print("w144x2: worst solid-entry distance after a step %.4f lr" % worst)


def test_fit_batches_partial_last_batch_and_sample_weight():
    """the method of the test of that name in tests/test_gpu_parity.py: 257 rows in batches of 128, 128 and 1"""
    m, model, spec, ws, x, y, sw = fresh("w144x2")
    model.compile("adam", loss="mse")
    hist = model.fit(x, y, epochs=2, batch_size=128, shuffle=False, verbose=0, sample_weight=sw)
    th = O.flatten(ws); mm = np.zeros_like(th); vv = np.zeros_like(th)
    t = 0
    ep_losses = []
    for ep in range(2):
        tot = 0.0
        for b0 in range(0, x.shape[0], 128):
            xb, yb, sb = x[b0:b0 + 128], y[b0:b0 + 128], sw[b0:b0 + 128]
            l, g = O.loss_and_grad(spec, O.unflatten(spec, th), xb.astype(np.float64), yb.astype(np.float64), sb.astype(np.float64))
            t += 1
            th, mm, vv = O.adam_step(th, O.flatten(g), mm, vv, t)
            tot += l * xb.shape[0]
        ep_losses.append(tot / x.shape[0])
    assert np.allclose(hist.history["loss"], ep_losses, rtol=5e-4), (hist.history["loss"], ep_losses)


def _dev_batch(e, x, y):
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    return d_x, d_y


def test_forward_behind_a_deferred_tail_and_behind_set_weights_sees_the_new_weights():
    import nif_amd
    m, model, spec, ws, x, y, sw = fresh("w144x2")
    e, B = m._engine, x.shape[0]
    e.set_option("fuse_tail", 1)
    d_x, d_y = _dev_batch(e, x, y)
    d_u = e.alloc(B * spec.so)
    e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
    e.opt_step_dev(nif_amd.Adam(1e-3).as_opt())
    e.forward_dev(d_x.at(0), B, d_u.at(0))
    u = d_u.download(B * spec.so).reshape(B, spec.so)
    ws_now = [w.astype(np.float64) for w in model.get_weights()]
    assert not np.array_equal(O.flatten(ws_now), O.flatten(ws))
    assert _rel(u, O.forward(spec, ws_now, x.astype(np.float64))) < 1e-5
    ws2 = [(w * 1.25).astype(np.float32) for w in model.get_weights()]
    model.set_weights(ws2)
    e.forward_dev(d_x.at(0), B, d_u.at(0))
    u2 = d_u.download(B * spec.so).reshape(B, spec.so)
    assert _rel(u2, O.forward(spec, [w.astype(np.float64) for w in ws2], x.astype(np.float64))) < 1e-5


def test_a_captured_step_equals_the_eager_step_bit_for_bit():
    import nif_amd
    adam = nif_amd.Adam(1e-3).as_struct()
    out = []
    for captured in (False, True):
        m, model, spec, ws, x, y, sw = fresh("w144x2")
        e, B = m._engine, x.shape[0]
        e.reserve(B)
        d_x, d_y = _dev_batch(e, x, y)
        if captured:
            e.graph_begin()
            e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
            e.adam_step_dev(adam)
            gid = e.graph_end()
            e.graph_launch(gid, adam)
            e.graph_destroy(gid)
        else:
            e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
            e.adam_step_dev(adam)
        out.append((e.get_flat(), e.last_loss()))
        assert e.get_opt_state()[2] == 1
    assert not np.array_equal(out[0][0], O.flatten(ws).astype(np.float32))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]


def test_a_capture_that_would_grow_a_workspace_is_refused_and_leaves_the_context_usable():
    from nif_amd._lib import NifError
    m, model, spec, ws, x, y, sw = fresh("w129x1")
    e, B = m._engine, x.shape[0]
    d_x, d_y = _dev_batch(e, x, y)
    model.predict(x[:1])                      # (nothing reserved for a training step)
    e.graph_begin()
    try:
        assert e.lib.nif_loss_grad_dev(e.ctx, d_x.at(0), d_y.at(0), None, B, B) == -4      # NIF_ERR_STATE
    finally:
        try:
            e.graph_destroy(e.graph_end())
        except NifError:
            pass
    assert _rel(model.predict(x), O.forward(spec, ws, x.astype(np.float64))) < 1e-5


MESHES = [1, 7, 0, 64, 257, 33]       # a single point, an empty mesh, partial tiles, an exact tile multiple, tile + 1


@pytest.mark.parametrize("name", ["w144x2", "w512x1"])      # (r, so) = (5, 3): the shared mesh on one phi pass; (16, 4)
@pytest.mark.parametrize("by", ["p", "latent"])
def test_snapshots_match_the_oracle_field_by_field(name, by):
    m, model, spec, ws, x, y, sw = make(name)
    rng = np.random.default_rng(7)
    T = len(MESHES)
    p = rng.uniform(-1, 1, size=(T, spec.pi)).astype(np.float32)
    xs = [rng.uniform(-1, 1, size=(n, spec.si)).astype(np.float32) for n in MESHES]
    xsh = xs[4]
    rows = p if by == "p" else m.model_p_to_lr().predict(p)

    def ref(t, xm):
        if by == "p":
            return O.forward(spec, ws, np.hstack([np.tile(p[t], (xm.shape[0], 1)), xm]).astype(np.float64))
        lat = np.tile(rows[t].astype(np.float64), (xm.shape[0], 1))
        return np.einsum("bsj,bj->bs", O.model_x_to_phi(spec, ws, xm.astype(np.float64)), lat) + ws[-1]

    ragged = model.predict_snapshots(xs, **{by: rows})
    shared = model.predict_snapshots(xsh, **{by: rows})
    assert shared.shape == (T, xsh.shape[0], spec.so)
    errs = [_rel(ragged[t], ref(t, xs[t])) for t in range(T) if MESHES[t]] + [_rel(shared[t], ref(t, xsh)) for t in range(T)]
    print("snapshots %s= %s: worst rel-L2 %.3g" % (by, name, max(errs)))
    assert ragged[2].shape == (0, spec.so)
    assert max(errs) < 1e-5, errs
    if by == "p":
        for t in range(T):
            table = np.hstack([np.tile(p[t], (xsh.shape[0], 1)), xsh])
            assert _rel(shared[t], model.predict(table).astype(np.float64)) < 2e-5


def _ll(n, **kw):
    return _cfg("LL", n, 1, 32, 1, 2, 2, 1, 1, **kw)


def test_refusals_at_construction():
    import nif_amd
    from nif_amd._lib import NifError

    def build(cfg, **kw):      # (the constructor needs no GPU: the context, hence nif_create, comes with the first use)
        kind, cs, cp = cfg
        m = getattr(nif_amd, kind)(cs, cp, **kw)
        return m.build().get_weights()

    with pytest.raises(NifError, match="only the last-layer class goes wider"):
        build(_cfg("NIFMultiScale", 129, 1, 32, 1, 1, 2, 1, 1))
    with pytest.raises(NifError, match="only the last-layer class goes wider"):
        build(_cfg("NIF", 129, 1, 32, 1, 1, 2, 1, 1))
    with pytest.raises(NifError, match=r"\[1,512\]"):
        build(_ll(513))
    with pytest.raises(NifError, match="use_resblock stops at 128 units"):
        build(_ll(144, s_res=True))
    with pytest.raises(NifError, match="mixed policies stop at 128 units"):
        build(_ll(144), mixed_policy="mixed_bfloat16")
    with pytest.raises(NifError, match="mixed policies stop at 128 units"):
        build(_ll(144), mixed_policy="mixed_float16")
    with pytest.raises(NifError, match=r"ParameterNet units must be in \[1,128\]"):
        build(_cfg("LL", 144, 1, 129, 1, 2, 2, 1, 1))
    build(_ll(128, s_res=True))      # the cap itself is as it was


def test_derivative_layers_refuse_a_wide_net_and_leave_it_usable():
    import nif_amd
    from nif_amd._lib import NifError
    m, model, spec, ws, x, y, sw = fresh("w129x1")
    yi, xi = list(range(spec.so)), list(range(spec.pi, spec.pi + spec.si))
    ref = O.forward(spec, ws, x.astype(np.float64))
    gt = np.zeros((x.shape[0], spec.so, len(xi)), np.float32)
    msg = "up to 128 units"

    def usable():
        assert _rel(model.predict(x), ref) < 1e-5

    with pytest.raises(NifError, match=msg):
        nif_amd.JacobianLayer(model, yi, xi)(x)
    usable()
    with pytest.raises(NifError, match=msg):
        nif_amd.HessianLayer(model, yi, xi)(x)
    usable()
    sm = nif_amd.SobolevModel(nif_amd.JacobianLayer(model, yi, xi))
    sm.compile(nif_amd.Adam(1e-4), "mse", loss_weights=[1.0, 0.1])
    with pytest.raises(NifError, match=msg):
        sm.fit(x, [y, gt], batch_size=x.shape[0], epochs=1, shuffle=False, verbose=0)
    usable()
    with pytest.raises(NifError, match=msg):
        sm.predict(x)
    usable()
    with pytest.raises(NifError, match=msg):
        m._engine.sobolev_forward(x, xi)
    usable()
