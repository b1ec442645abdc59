"""The snapshot-wise training step of the last-layer class on the device (include/nif_hip_snapfit.h, csrc/k_snapfit.hip,
Model.fit_snapshots) against the fp64 oracle on the expanded table [repeat(p, M) | tile(x, T)] and against the point-wise step on the
same table.  The bars are the ones this class's step already has (tests/test_gpu_parity.py::test_loss_and_grad_match_oracle,
tests/test_gpu_wide_ll.py): loss 2e-6 relative, flat gradient 3e-5 rel-L2, each tensor 5e-5 of its norm (+ 2.5e-7 of the whole
gradient's); the two device paths are each within one bar of the oracle, so within two of each other.

Nets: ll_plain_32x2_r3 (the 32-point MLP route), a 32 x 2 net with r = 10, so = 3, pi = 2, si = 2 (tests/snapfit_ref.py) and the
129-unit net of tests/wide_ll_cases.py (the layer-by-layer route).  Shapes (T, M): (1, 1) one group and one tile; (1, 33) a tile
edge; (7, 64) fewer than the eight point groups of a workgroup; (9, 65) more than eight; (40, 257) more than one 32-row ParameterNet
tile and several mesh tiles with a ragged last one.  One more net, ll_res_48x2_r4, takes resblocks and the ParameterNet's stash-path
adjoint through two of the shapes.  The CPU side is tests/test_fit_snapshots.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import snapfit_ref as R
from tests.test_gpu_parity import CONFIGS, _make, _make_policy, _rel
from tests.wide_ll_cases import CASES as WIDE_CASES

pytestmark = pytest.mark.gpu

NETS = {
    "ll_plain_32x2_r3": CONFIGS["ll_plain_32x2_r3"][0],
    "ll_32x2_r10_so3": R.NET_R10_SO3,
    "w129x1": WIDE_CASES["w129x1"][0],
}
EXTRA_NETS = {"ll_res_48x2_r4": CONFIGS["ll_res_48x2_r4"][0]}      # (one test's: resblocks, a ParameterNet on the stash path)
LOSS_BAR, FLAT_BAR, TENSOR_BAR, TENSOR_FLOOR = 2e-6, 3e-5, 5e-5, 2.5e-7

_models, _refs = {}, {}


def _net(name):
    """(m, model, spec, ws64) of a net, built once: the tests that change weights or engine state build their own with _fresh()"""
    if name not in _models:
        _models[name] = _fresh(name)
    return _models[name]


def _fresh(name):
    return _make((NETS[name] if name in NETS else EXTRA_NETS[name], 1))[:4]


def _ref(name, T, M, weighted, loss="mse", yscale=1.0):
    """the oracle's (loss, flat gradient) on the expanded table in float64, computed once"""
    key = (name, T, M, weighted, loss, yscale)
    if key not in _refs:
        spec, ws = _net(name)[2:]
        p, x, y, sw = R.problem(spec, T, M)
        l, g = O.loss_and_grad(spec, ws, R.expanded_table(p, x).astype(np.float64), (yscale * y).astype(np.float64).reshape(T * M, spec.so),
                               sw.astype(np.float64).reshape(-1) if weighted else None, loss=loss)
        _refs[key] = (l, O.flatten(g))
    return _refs[key]


def _shares(spec, loss, g, lref, gref):
    """the shares of the three bars a result uses: (loss, flat gradient, worst tensor)"""
    g = np.asarray(g, dtype=np.float64)
    gn, off, worst = np.linalg.norm(gref), 0, 0.0
    for nm, shp in spec.param_shapes():
        k = int(np.prod(shp))
        err = np.linalg.norm(g[off:off + k] - gref[off:off + k])
        worst = max(worst, err / (TENSOR_BAR * np.linalg.norm(gref[off:off + k]) + TENSOR_FLOOR * gn))
        off += k
    return abs(loss - lref) / (LOSS_BAR * abs(lref)), _rel(g, gref) / FLAT_BAR, worst


def _within(spec, loss, g, lref, gref, bars=1.0, what=""):
    s = _shares(spec, loss, g, lref, gref)
    print("%s: share of the bars: loss %.3f, flat gradient %.3f, worst tensor %.3f" % ((what,) + s))
    assert max(s) <= bars, (what, s)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("T,M", R.SHAPES)
@pytest.mark.parametrize("name", sorted(NETS))
def test_step_matches_the_oracle_and_the_pointwise_step_on_the_expanded_table(name, T, M, weighted):
    m, model, spec, ws = _net(name)
    e = m._engine
    p, x, y, sw = R.problem(spec, T, M)
    assert not weighted or T * M < 20 or (sw == 0).any()
    s = sw if weighted else None
    loss, g = e.snapshot_loss_grad(p, x, y, s)
    lref, gref = _ref(name, T, M, weighted)
    _within(spec, loss, g, lref, gref, 1.0, "%s (%d, %d) vs oracle" % (name, T, M))
    lp, gp = e.loss_and_grad(R.expanded_table(p, x), y.reshape(T * M, spec.so), None if s is None else s.reshape(-1))
    _within(spec, loss, g, lp, gp.astype(np.float64), 2.0, "%s (%d, %d) vs point-wise" % (name, T, M))
    # batch_global: the divisor of the mean alone
    l3, g3 = e.snapshot_loss_grad(p, x, y, s, batch_global=3 * T * M)
    _within(spec, 3.0 * l3, 3.0 * g3.astype(np.float64), lref, gref, 1.0, "batch_global")


@pytest.mark.parametrize("T,M", [(9, 65), (40, 257)])
def test_resblock_nets_and_a_parameternet_on_the_stash_path(T, M):
    """ll_res_48x2_r4 of tests/test_gpu_parity.py: a resblock ShapeNet on the MLP route, and a 40-unit resblock ParameterNet with two
    inputs, whose adjoint goes through the HBM stash and the k_gw_* stack (rows of p alone, pi columns) instead of k_pnet_bwg"""
    m, model, spec, ws = _net("ll_res_48x2_r4")
    p, x, y, sw = R.problem(spec, T, M)
    loss, g = m._engine.snapshot_loss_grad(p, x, y, sw)
    lref, gref = _ref("ll_res_48x2_r4", T, M, True)
    _within(spec, loss, g, lref, gref, 1.0, "ll_res_48x2_r4 (%d, %d) vs oracle" % (T, M))


@pytest.mark.parametrize("loss", R.LOSSES)
def test_every_loss_of_set_loss(loss):
    name, (T, M) = "ll_32x2_r10_so3", (9, 65)
    m, model, spec, ws = _net(name)
    e = m._engine
    p, x, y, sw = R.problem(spec, T, M)
    y3 = (3.0 * y).astype(np.float32)                      # |e| on both sides of Huber's delta
    e.set_loss(loss)
    try:
        l, g = e.snapshot_loss_grad(p, x, y3, sw)
    finally:
        e.set_loss("mse")
    lref, gref = _ref(name, T, M, True, loss, 3.0)
    _within(spec, l, g, lref, gref, 1.0, loss)


def test_two_calls_are_bit_identical_and_a_permutation_of_the_snapshots_stays_within_the_bar():
    for name, (T, M) in (("ll_32x2_r10_so3", (40, 257)), ("w129x1", (9, 65))):
        m, model, spec, ws = _net(name)
        e = m._engine
        p, x, y, sw = R.problem(spec, T, M)
        l1, g1 = e.snapshot_loss_grad(p, x, y, sw)
        e.loss_and_grad(R.expanded_table(p, x)[:40], y.reshape(T * M, spec.so)[:40])      # (other work on the workspaces in between)
        l2, g2 = e.snapshot_loss_grad(p, x, y, sw)
        assert l1 == l2 and np.array_equal(g1, g2)
        perm = np.random.default_rng(11).permutation(T)
        lq, gq = e.snapshot_loss_grad(p[perm], x, y[perm], sw[perm])
        lref, gref = _ref(name, T, M, True)
        _within(spec, lq, gq, lref, gref, 1.0, "%s permuted" % name)      # (the order of a float32 sum over t changes: no bit equality)


def test_empty_calls_give_a_zero_gradient_and_loss():
    m, model, spec, ws = _net("ll_plain_32x2_r3")
    e = m._engine
    p, x, y, sw = R.problem(spec, 3, 5)
    e.snapshot_loss_grad(p, x, y)
    for pp, xx, yy in ((p[:0], x, y[:0]), (p, x[:0], y[:, :0])):
        l, g = e.snapshot_loss_grad(pp, xx, yy)
        assert l == 0.0 and not g.any()


def test_with_weight_regularisers_set():
    """cfg_shape_net / cfg_parameter_net l2_reg: the term joins behind the step through the tail the point-wise step uses (bars of
    tests/test_gpu_parity.py::test_last_layer_class_shapenet_regularisers: loss 1e-5, flat gradient 2e-4)"""
    import nif_amd
    kind, cs, cp = NETS["ll_plain_32x2_r3"]
    cs2, cp2 = dict(cs, l2_reg=5e-4), dict(cp, l2_reg=2e-3)
    spec, ws = _net("ll_plain_32x2_r3")[2:]
    m = nif_amd.NIFMultiScaleLastLayerParameterized(cs2, cp2)
    model = m.build(); model.set_weights([w.astype(np.float32) for w in ws])
    T, M = 9, 65
    p, x, y, sw = R.problem(spec, T, M)
    loss, g = m._engine.snapshot_loss_grad(p, x, y, sw)
    lref, gref = _ref("ll_plain_32x2_r3", T, M, True)
    preg, sreg = O.weight_regularizer_coefficients(cs2, cp2, spec.kind)
    lreg, greg = O.weight_regularizer_term(spec, ws, preg, sreg)
    assert preg != (0.0, 0.0) and sreg != (0.0, 0.0) and lreg > 0.05 * abs(lref)
    assert abs(loss - (lref + lreg)) < 1e-5 * abs(lref + lreg)
    assert _rel(g, gref + O.flatten(greg)) < 2e-4
    lp, gp = m._engine.loss_and_grad(R.expanded_table(p, x), y.reshape(T * M, spec.so), sw.reshape(-1))
    _within(spec, loss, g, lp, gp.astype(np.float64), 2.0, "regularised vs point-wise")


def test_three_adam_steps_of_fit_snapshots_against_fit_on_the_expanded_table():
    """the Adam bar of tests/test_gpu_parity.py::test_adam_steps_follow_oracle, every step checked on its own from the same weights
    and slots: where the gradient entry is solid the two updates sit within 1 % of lr of each other, elsewhere within one sign flip
    of a normalised step; the logged losses are the oracle's"""
    import nif_amd
    LR, k, M = 2e-3, 3, 65
    m, model, spec, ws = _fresh("ll_32x2_r10_so3")
    e = m._engine
    model.compile(nif_amd.Adam(learning_rate=LR), loss="mse")
    p, x, u, sw = R.problem(spec, 3 * k, M)
    for i in range(3):
        ps, us, ws_ = p[i * k:(i + 1) * k], u[i * k:(i + 1) * k], sw[i * k:(i + 1) * k]
        table, y = R.expanded_table(ps, x), us.reshape(k * M, spec.so)
        if i == 0:
            ha = model.fit_snapshots(x, us[:1], ps[:1], epochs=0)      # (zero epochs: the freshly compiled optimizer's slots exist)
        th0 = O.flatten(model.get_weights()).astype(np.float64)
        m0, v0, step0 = e.get_opt_state()
        ha = model.fit_snapshots(x, us, ps, sample_weight=ws_, epochs=1, shuffle=False)
        wa = O.flatten(model.get_weights()).astype(np.float64)
        model.set_weights([w.astype(np.float32) for w in O.unflatten(spec, th0)])
        e.set_opt_state(m0, v0, step0)
        hb = model.fit(table, y, sample_weight=ws_.reshape(-1), batch_size=k * M, epochs=1, shuffle=False, verbose=0)
        wb = O.flatten(model.get_weights()).astype(np.float64)
        assert e.get_opt_state()[2] == step0 + 1
        l, g = O.loss_and_grad(spec, O.unflatten(spec, th0), table.astype(np.float64), y.astype(np.float64), ws_.reshape(-1).astype(np.float64))
        for h in (ha, hb):
            assert abs(h.history["loss"][0] - l) <= 2e-5 * abs(l), (i, h.history["loss"][0], l)
        solid, off = np.ones_like(th0, dtype=bool), 0
        for gt in g:
            rms = np.sqrt(np.mean(gt ** 2)) + 1e-300
            solid[off:off + gt.size] = np.abs(gt.ravel()) > 0.02 * rms
            off += gt.size
        assert solid.mean() > 0.8
        d = np.abs(wa - wb)
        print("step %d: worst solid entry %.4f of lr" % (i, d[solid].max() / LR))
        assert d[solid].max() < 0.01 * LR, (i, d[solid].max() / LR)
        assert d.max() <= 2.0 * LR * 1.001


def test_fit_snapshots_shuffled_epochs_with_steps_of_whole_snapshots_reduce_the_loss():
    import nif_amd
    m, model, spec, ws = _fresh("ll_plain_32x2_r3")
    model.compile(nif_amd.Adam(learning_rate=1e-3), loss="mse")
    T, M = 10, 33
    p, x, _, sw = R.problem(spec, T, M)
    u = np.stack([np.sin(3.0 * x[:, :1] + pt[0]) * np.ones((1, spec.so), np.float32) for pt in p]).astype(np.float32)
    model._shuffle_seed = 4
    h = model.fit_snapshots(x, u, p, sample_weight=sw[0], epochs=12, snapshots_per_step=4)
    assert len(h.history["loss"]) == 12 and h.history["loss"][-1] < 0.9 * h.history["loss"][0]
    assert m._engine.get_opt_state()[2] == 36      # 4 + 4 + 2 snapshots: three steps an epoch


def _pointwise_still_right(m, spec, ws, what):
    rng = np.random.default_rng(21)
    x = rng.uniform(-1, 1, size=(70, spec.pi + spec.si)).astype(np.float32)
    y = rng.uniform(-1, 1, size=(70, spec.so)).astype(np.float32)
    loss, g = m._engine.loss_and_grad(x, y)
    lref, gref = O.loss_and_grad(spec, ws, x.astype(np.float64), y.astype(np.float64))
    _within(spec, loss, g, lref, O.flatten(gref), 1.0, "point-wise step behind the refusal (%s)" % what)


def test_every_refusal_has_its_message_and_leaves_the_context_usable():
    from nif_amd import _lib
    # the two hypernetwork classes
    for name in ("ms_64x2_mlp_pnet_r3", "nif_cfg1_32x2"):
        m, model, spec, ws, _, _, _ = _make(name)
        p, x, y, sw = R.problem(spec, 3, 5)
        with pytest.raises(_lib.NifError, match="not built for the hypernetwork classes"):
            m._engine.snapshot_loss_grad(p, x, y)
        _pointwise_still_right(m, spec, ws, name)
    # a mixed policy
    m, model, spec, ws, xx, yy, _ = _make_policy("ll_plain_32x2_r3", "mixed_bfloat16")
    p, x, y, sw = R.problem(spec, 3, 5)
    before = m._engine.loss_and_grad(xx, yy)
    with pytest.raises(_lib.NifError, match="not built for the mixed_bfloat16 policy"):
        m._engine.snapshot_loss_grad(p, x, y)
    after = m._engine.loss_and_grad(xx, yy)
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    # the two regularisers, so r > 64, the struct's version and reserved fields, a capture
    m, model, spec, ws = _fresh("ll_plain_32x2_r3")
    e = m._engine
    p, x, y, sw = R.problem(spec, 3, 5)
    e.set_activity_regularizer(1e-3, 0.0)
    with pytest.raises(_lib.NifError, match="activity regulariser"):
        e.snapshot_loss_grad(p, x, y)
    e.set_activity_regularizer(0.0, 0.0)
    e.set_jac_regularizer(1e-3)
    with pytest.raises(_lib.NifError, match="latent Jacobian regulariser"):
        e.snapshot_loss_grad(p, x, y)
    e.set_jac_regularizer(0.0)
    d = [e.alloc(a.size) for a in (p, x, y)]
    for buf, a in zip(d, (p, x, y)):
        buf.upload(a)
    def args():
        return e._snapfit_args(d[0].at(0), 3, d[1].at(0), 5, d[2].at(0), None, 0)
    for change, msg in ((lambda a: setattr(a, "abi_version", 2), "abi_version 2 != 1"), (lambda a: setattr(a, "reserved0", 1), "reserved fields"),
                        (lambda a: a.reserved.__setitem__(3, 7), "reserved fields")):
        a = args(); change(a)
        for fn in (e.lib.nif_snapshot_loss_grad_dev, e.lib.nif_snapshot_loss_grad):
            assert fn(C.byref(a)) == -1
            assert msg in e.lib.nif_last_error().decode()
    a = args()
    e.graph_begin()
    try:
        assert e.lib.nif_snapshot_loss_grad_dev(C.byref(a)) == -4
        assert "not capturable" in e.lib.nif_last_error().decode()
        assert e.lib.nif_snapshot_loss_grad(C.byref(a)) == -4
    finally:
        e.graph_end()
    assert e.lib.nif_snapshot_loss_grad_dev(C.byref(a)) == 0
    l1, g1 = e.grad_read()
    l2, g2 = e.snapshot_loss_grad(p, x, y)
    assert l1 == l2 and np.array_equal(g1, g2)
    for buf in d:
        buf.free()
    _pointwise_still_right(m, spec, ws, "regularisers, struct, capture")
    # so * latent_dim > 64 (the bound of the head's register sums, stated in the entry as well): no context of this class exists
    # beyond it -- nif_create refuses the net
    import nif_amd
    kind, cs, cp = R.cfg_ll(n=32, L=1, nst=32, lst=1, r=22, si=2, so=3, pi=1)
    with pytest.raises(_lib.NifError, match=r"latent_dim \* output_dim must be <= 64"):
        nif_amd.NIFMultiScaleLastLayerParameterized(cs, cp)._engine
