"""Host logic of low-magnitude pruning (nif_amd.sparsity) without a GPU: the schedules and the keep count, validation, the table of
pruned tensors, the step numbering of UpdatePruningStep, the order of the calls Model.fit makes (on the oracle engine double with
NumPy pruning), checkpoints, and a gloo world-2 fit in which both ranks make the same pruning decisions."""
import os
import socket
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import prune_ref as R
from tests.cfgs import ALL_SMALL
from tests.doubles import OracleEngine

f32 = np.float32


class PruneEngine(OracleEngine):
    """OracleEngine + the nif_prune_* calls restated in NumPy (tests/prune_ref.py), every call recorded"""

    def __init__(self, spec_oracle, weights, reg=(0.0, 0.0, 0, 0)):
        OracleEngine.__init__(self, spec_oracle, weights, reg)
        self.shapes = spec_oracle.param_shapes()
        self.segs, self.masks, self.thr = [], [], []

    def prune_config(self, offsets, sizes):
        self.segs = list(zip([int(o) for o in offsets], [int(n) for n in sizes]))
        self.masks = [np.ones((n,), f32) for _, n in self.segs]
        self.thr = [f32(0.0) for _ in self.segs]
        self.calls.append(("prune_config", len(self.segs)))

    def prune_update(self, ks):
        assert self.segs, "not configured"
        for i, ((off, n), k) in enumerate(zip(self.segs, ks)):
            w = self.theta[off:off + n].astype(f32)
            self.thr[i] = R.threshold(w, int(k))
            self.masks[i] = R.mask(w, self.thr[i])
        self.calls.append(("prune_update", tuple(int(k) for k in ks)))

    def prune_apply(self):
        assert self.segs, "not configured"
        for (off, n), mk in zip(self.segs, self.masks):
            self.theta[off:off + n] = self.theta[off:off + n] * mk
        self.calls.append(("prune_apply",))

    def get_prune_state(self):
        return [m.copy() for m in self.masks], np.array(self.thr, f32)

    def set_prune_state(self, masks, thr):
        self.masks = [np.asarray(m, f32).copy() for m in masks]
        self.thr = [f32(t) for t in thr]

    def get_weights(self):
        return [w.astype(f32) for w in O.unflatten(self.o, self.theta)]

    def set_weights(self, weights):
        self.theta = O.flatten([np.asarray(w, np.float64) for w in weights])


def _problem(name="ms_plain", n=72, seed=0):
    kind, cs, cp = ALL_SMALL[name]
    spec = O.Spec(kind, cs, cp)
    rng = np.random.default_rng(seed)
    ws = O.init_weights(spec, rng)
    x = rng.uniform(-1, 1, size=(n, spec.pi + spec.si)).astype(f32)
    y = rng.uniform(-1, 1, size=(n, spec.so)).astype(f32)
    return kind, cs, cp, spec, ws, x, y


def _model(eng, kind, cs, cp):
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    return Model(types.SimpleNamespace(_spec=Spec(kind, cs, cp), _engine=eng), "full")


# ---- schedules ------------------------------------------------------------------------------------------------------------------
def test_polynomial_decay_values_and_turns():
    from nif_amd.sparsity import PolynomialDecay
    s = PolynomialDecay(0.2, 0.8, begin_step=10, end_step=110, power=3, frequency=10)
    at_begin = f32(f32(-0.6) + f32(0.8))                 # 0.19999999: float32, not 0.2
    assert at_begin != f32(0.2)
    for step, sp in ((0, at_begin), (10, at_begin), (60, f32(f32(-0.6) * f32(0.125) + f32(0.8))), (110, f32(0.8)), (500, f32(0.8))):
        assert s.sparsity(step) == sp, (step, s.sparsity(step))
        assert isinstance(s.sparsity(step), np.float32)
    # float32 throughout: p = 30 / 100, (1 - p)^3 = 0.343, -0.6 * 0.343 + 0.8
    assert s.sparsity(40) == f32(f32(-0.6) * np.power(f32(1) - f32(30) / f32(100), f32(3)) + f32(0.8))
    turns = [st for st in range(0, 140) if s(st)[0]]
    assert turns == list(range(10, 111, 10))
    for st in range(0, 140):
        assert s.should_prune(st) == R.should_prune(st, 10, 110, 10)


def test_constant_sparsity_turns():
    from nif_amd.sparsity import ConstantSparsity
    s = ConstantSparsity(0.5, begin_step=3, frequency=4)
    assert [st for st in range(30) if s(st)[0]] == [3, 7, 11, 15, 19, 23, 27]
    assert s(100) == (False, f32(0.5)) and s(103) == (True, f32(0.5))
    e = ConstantSparsity(0.25, begin_step=0, end_step=5, frequency=1)
    assert [st for st in range(10) if e.should_prune(st)] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("size, sparsity, k", [
    (15, 0.7, 4),      # float32 product 4.5 exactly -> half to even; float64 gives 4.500000000000001 -> 5
    (10, 0.85, 1),     # float32 1.4999998; float64 1.5000000000000002 -> 2
    (30, 0.65, 11),    # float32 10.500001; float64 10.5 -> 10
    (30, 0.55, 14),    # float32 13.5 -> 14 (even); float64 13.499999999999998 -> 13
    (5, 0.9, 1),
    (1, 0.99, 1),      # at least one entry stays
    (7, 0.0, 7),
    (2, 0.5, 1),       # 1.0
    (6, 0.5, 3),
])
def test_keep_count_rounds_in_float32_half_to_even(size, sparsity, k):
    from nif_amd.sparsity import keep_count
    assert keep_count(size, sparsity) == k == R.keep(size, sparsity)


def test_schedule_validation():
    from nif_amd.sparsity import ConstantSparsity, PolynomialDecay
    bad = [lambda: PolynomialDecay(-0.1, 0.5, 0, 10), lambda: PolynomialDecay(0.1, 1.0, 0, 10),
           lambda: PolynomialDecay(0.1, 0.5, -1, 10), lambda: PolynomialDecay(0.1, 0.5, 5, 4),
           lambda: PolynomialDecay(0.1, 0.5, 0, -1), lambda: PolynomialDecay(0.1, 0.5, 0, 10, frequency=0),
           lambda: ConstantSparsity(1.0, 0), lambda: ConstantSparsity(-0.5, 0), lambda: ConstantSparsity(0.5, -2),
           lambda: ConstantSparsity(0.5, 5, end_step=4), lambda: ConstantSparsity(0.5, 0, end_step=-3),
           lambda: ConstantSparsity(0.5, 0, frequency=-1)]
    for mk in bad:
        with pytest.raises(ValueError):
            mk()
    ConstantSparsity(0.0, 0, end_step=-1)
    PolynomialDecay(0.0, 0.9, 3, 3)


# ---- the table of pruned tensors ------------------------------------------------------------------------------------------------
EXPECTED = {
    "nif_swish": ["pnet_first_w", "pnet_h0_w", "pnet_h0_b", "pnet_h1_w", "pnet_h1_b", "pnet_bottleneck_w", "pnet_last_w"],
    "ms_plain": ["pnet_first_w", "pnet_h0_w", "pnet_h1_w", "pnet_bottleneck_w", "pnet_last_w"],
    "ms_res_pres": ["pnet_first_w", "pnet_h0_w", "pnet_h0_w2", "pnet_h1_w", "pnet_h1_w2", "pnet_bottleneck_w", "pnet_last_w"],
    "ms_mlp_pnet": ["pnet_first_w", "pnet_h0_w", "pnet_h0_b", "pnet_h1_w", "pnet_h1_b", "pnet_bottleneck_w", "pnet_last_w"],
    "ms_mlp_pres": ["pnet_first_w", "pnet_h0_w", "pnet_h0_b", "pnet_h0_w2", "pnet_h0_b2", "pnet_h1_w", "pnet_h1_b", "pnet_h1_w2",
                    "pnet_h1_b2", "pnet_bottleneck_w", "pnet_last_w"],
    "ll_plain": ["pnet_first_w", "pnet_h0_w", "pnet_h1_w", "pnet_bottleneck_w", "pnet_last_w", "snet_first_w", "snet_h0_w",
                 "snet_h1_w", "snet_bottleneck_w"],
    "ll_res": ["pnet_first_w", "pnet_h0_w", "pnet_h0_w2", "pnet_h1_w", "pnet_h1_w2", "pnet_bottleneck_w", "pnet_last_w",
               "snet_first_w", "snet_h0_w", "snet_h0_w2", "snet_h1_w", "snet_h1_w2", "snet_bottleneck_w"],
}


@pytest.mark.parametrize("name", sorted(ALL_SMALL))
def test_prunable_tensor_table(name):
    from nif_amd.sparsity import prunable_weights
    kind, cs, cp = ALL_SMALL[name]
    spec = O.Spec(kind, cs, cp)
    model = _model(PruneEngine(spec, O.init_weights(spec, np.random.default_rng(0))), kind, cs, cp)
    names = prunable_weights(model)
    if name in EXPECTED:
        assert names == EXPECTED[name]
    all_names = [nm for nm, _ in model._owner._spec.param_shapes()]
    assert set(names) <= set(all_names) and "pnet_last_b" not in names and "last_layer_bias" not in names
    assert [nm for nm in all_names if nm in names] == names      # flat order


def test_prune_low_magnitude_refusals():
    import nif_amd
    from nif_amd import sparsity as S
    kind, cs, cp, spec, ws, x, y = _problem()
    model = _model(PruneEngine(spec, ws), kind, cs, cp)
    for kw, word in (({"block_size": (1, 2)}, "block_size"), ({"block_pooling_type": "MAX"}, "block_pooling_type"),
                     ({"pruning_policy": object()}, "pruning_policy"), ({"sparsity_m_by_n": (2, 4)}, "sparsity_m_by_n")):
        with pytest.raises(NotImplementedError, match=word):
            S.prune_low_magnitude(model, **kw)
    p = S.prune_low_magnitude(model)
    assert isinstance(p.pruning_schedule, S.ConstantSparsity) and p.pruning_schedule.target_sparsity == 0.5
    assert p.optimizer is None and p.pruning_step == -1
    with pytest.raises(ValueError, match="already pruned"):
        S.prune_low_magnitude(p)
    with pytest.raises(ValueError, match="already pruned"):
        S.prune_low_magnitude(model)           # the same weights, a second wrapper
    nif = nif_amd.NIFMultiScale(cs, dict(cp, jac_reg=1e-3))
    with pytest.raises(NotImplementedError, match="jac_reg"):
        S.prune_low_magnitude(nif.build())
    with pytest.raises(NotImplementedError):
        S.prune_low_magnitude(nif.model_p_to_lr())
    with pytest.raises(NotImplementedError):
        S.prune_low_magnitude(nif_amd.SobolevModel(nif_amd.JacobianLayer(nif.model(), [0], [1])))
    p.compile(nif_amd.Adam(1e-3), "mse")
    with pytest.raises(NotImplementedError, match="pruned"):
        nif_amd.optimizers.TFPLBFGS(p, "mse", x, y)


# ---- fit ------------------------------------------------------------------------------------------------------------------------
def _pruned(eng, kind, cs, cp, schedule):
    import nif_amd
    from nif_amd import sparsity as S
    p = S.prune_low_magnitude(_model(eng, kind, cs, cp), pruning_schedule=schedule)
    p.compile(nif_amd.Adam(1e-2), "mse")
    return p


def test_fit_without_the_callback_raises_until_the_step_is_set():
    from nif_amd import sparsity as S
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = PruneEngine(spec, ws)
    p = _pruned(eng, kind, cs, cp, S.ConstantSparsity(0.5, 0, frequency=1))
    th0 = eng.theta.copy()
    with pytest.raises(ValueError, match="UpdatePruningStep"):
        p.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
    assert np.array_equal(eng.theta, th0)
    p.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    assert p.pruning_step == 4
    n_upd = sum(1 for c in eng.calls if c[0] == "prune_update")
    p.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)          # no callback: the step stays at 4
    assert p.pruning_step == 4
    assert sum(1 for c in eng.calls if c[0] == "prune_update") == n_upd + 5   # (step 4 is a turn of frequency 1: every batch)


def test_step_numbering_across_two_fit_calls():
    """TF-MOT: on_train_begin takes the model's step, every batch sets it and counts on: the second call repeats the last number"""
    from nif_amd import sparsity as S
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = PruneEngine(spec, ws)
    p = _pruned(eng, kind, cs, cp, S.ConstantSparsity(0.5, 0, frequency=1))
    seen = []
    orig = S.PrunedModel._batch_hook

    def spy(self, e, cbs):
        run = orig(self, e, cbs)

        def wrapped():
            run()
            seen.append(self.pruning_step)
        return wrapped
    S.PrunedModel._batch_hook = spy
    try:
        cb = S.UpdatePruningStep()
        p.fit(x, y, batch_size=16, epochs=2, shuffle=False, verbose=0, callbacks=[cb])
        assert seen == list(range(10)) and p.pruning_step == 9 and cb.step == 10
        p.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
        assert seen[10:] == [9, 10, 11, 12, 13] and p.pruning_step == 13
    finally:
        S.PrunedModel._batch_hook = orig


def test_epoch_end_masking_follows_the_callback_order():
    from nif_amd import sparsity as S
    from nif_amd.callbacks import Callback
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = PruneEngine(spec, ws)
    p = _pruned(eng, kind, cs, cp, S.ConstantSparsity(0.5, 0, frequency=100))

    class Probe(Callback):
        def __init__(self):
            Callback.__init__(self)
            self.zeros = []

        def on_epoch_end(self, epoch, logs=None):
            o, k = eng.segs[-1]
            self.zeros.append(int(np.count_nonzero(eng.theta[o:o + k] == 0)))

    before, after = Probe(), Probe()
    p.fit(x, y, batch_size=16, epochs=2, shuffle=False, verbose=0, callbacks=[before, S.UpdatePruningStep(), after])
    o, k = eng.segs[-1]
    want = k - R.keep(k, 0.5)
    assert after.zeros == [want, want]                   # masked by the callback before this one ran
    assert all(z < want for z in before.zeros)            # the last batch's update moved the pruned entries again


def _numpy_pruned_training(spec, ws, x, y, segs, schedule, bs, epochs, lr):
    """the order of nif_amd/sparsity.py by hand: step number, mask update on a turn, w *= mask, loss / gradient, Adam; masks at
    every epoch end"""
    th = O.flatten(ws)
    m = np.zeros_like(th); v = np.zeros_like(th); t = 0
    masks = [np.ones((n,), f32) for _, n in segs]
    step = 0
    for _ in range(epochs):
        for b0 in range(0, x.shape[0], bs):
            should, sp = schedule(step)
            if should:
                for i, (off, n) in enumerate(segs):
                    w = th[off:off + n].astype(f32)
                    masks[i] = R.mask(w, R.threshold(w, R.keep(n, sp)))
            for (off, n), mk in zip(segs, masks):
                th[off:off + n] = th[off:off + n] * mk
            xb, yb = x[b0:b0 + bs].astype(np.float64), y[b0:b0 + bs].astype(np.float64)
            _, g = O.loss_and_grad(spec, O.unflatten(spec, th), xb, yb)
            t += 1
            th, m, v = O.adam_step(th, O.flatten(g), m, v, t, lr=float(f32(lr)), b1=float(f32(0.9)), b2=float(f32(0.999)),
                                   eps=float(f32(1e-7)))      # (nif_adam carries float32 hyper-parameters)
            step += 1
        for (off, n), mk in zip(segs, masks):
            th[off:off + n] = th[off:off + n] * mk
    return th, masks


@pytest.mark.parametrize("name", ["ms_plain", "nif_swish", "ll_res", "ms_mlp_pres"])
def test_pruned_fit_equals_the_numpy_loop(name):
    from nif_amd import sparsity as S
    kind, cs, cp, spec, ws, x, y = _problem(name)
    eng = PruneEngine(spec, ws)
    sched = S.PolynomialDecay(0.2, 0.75, begin_step=1, end_step=9, frequency=2)
    p = _pruned(eng, kind, cs, cp, sched)
    p.fit(x, y, batch_size=16, epochs=3, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    segs = R.segments(spec, S.prunable_weights(p))
    th, masks = _numpy_pruned_training(spec, ws, x, y, segs, sched, 16, 3, 1e-2)
    assert np.array_equal(eng.theta, th)
    assert all(np.array_equal(a, b) for a, b in zip(eng.masks, masks))
    # the calls of a batch: [prune_update] prune_apply loss_grad (one Adam step follows); 15 batches, turns at 1, 3, 5, 7, 9
    kinds = [c[0] for c in eng.calls if c[0] in ("prune_update", "prune_apply", "loss_grad")]
    assert kinds.count("loss_grad") == 15 and kinds.count("prune_update") == 5 and kinds.count("prune_apply") == 15 + 3
    for i, c in enumerate(kinds):
        if c == "loss_grad":
            assert kinds[i - 1] == "prune_apply"
    for (off, n), mk in zip(segs, masks):
        assert np.count_nonzero(th[off:off + n] == 0) == n - int(mk.sum())


def test_inference_applies_the_masks_first():
    from nif_amd import sparsity as S
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = PruneEngine(spec, ws)
    p = _pruned(eng, kind, cs, cp, S.ConstantSparsity(0.5, 0))
    p.fit(x, y, batch_size=72, epochs=1, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    eng.theta += 1e-3                                   # unmasked weights (what an optimizer step leaves)
    n0 = sum(1 for c in eng.calls if c == ("prune_apply",))
    p.predict(x); p(x); p.evaluate(x, y)
    assert sum(1 for c in eng.calls if c == ("prune_apply",)) == n0 + 3
    o, k = eng.segs[0]
    assert np.count_nonzero(eng.theta[o:o + k] == 0) == k - R.keep(k, 0.5)


def test_graph_epochs_are_off_for_pruned_fits():
    from nif_amd import sparsity as S
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = PruneEngine(spec, ws)
    eng.graph_begin = lambda: (_ for _ in ()).throw(AssertionError("captured"))
    p = _pruned(eng, kind, cs, cp, S.ConstantSparsity(0.5, 0))
    p._graph_epochs = True
    p.fit(x, y, batch_size=8, epochs=3, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])


def test_strip_pruning_returns_a_plain_model_over_the_masked_weights():
    from nif_amd import sparsity as S
    from nif_amd.model import Model
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = PruneEngine(spec, ws)
    p = _pruned(eng, kind, cs, cp, S.ConstantSparsity(0.5, 0))
    p.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    eng.theta += 1e-3
    plain = S.strip_pruning(p)
    assert type(plain) is Model and eng.segs == []
    o, n = R.segments(spec, S.prunable_weights(p))[0]
    assert np.count_nonzero(eng.theta[o:o + n] == 0) == n - R.keep(n, 0.5)
    S.prune_low_magnitude(plain)                          # the weights may be pruned again


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_unpruned_keys(tmp_path):
    import nif_amd
    from nif_amd import sparsity as S
    kind, cs, cp, spec, ws, x, y = _problem()
    plain = _model(PruneEngine(spec, ws), kind, cs, cp)
    plain.compile(nif_amd.Adam(1e-2), "mse")
    plain.save_weights(str(tmp_path / "plain"))
    keys = sorted(np.load(str(tmp_path / "plain.npz")).files)
    assert keys == sorted(["names", "adam_m", "adam_v", "adam_step"] + ["w%03d" % i for i in range(len(ws))])

    eng = PruneEngine(spec, ws)
    p = _pruned(eng, kind, cs, cp, S.ConstantSparsity(0.6, 0, frequency=2))
    p.fit(x, y, batch_size=16, epochs=2, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    p.save_weights(str(tmp_path / "pruned"))
    d = np.load(str(tmp_path / "pruned.npz"))
    names = S.prunable_weights(p)
    assert sorted(d.files) == sorted(keys + ["prune_mask_%s" % nm for nm in names] + ["prune_thresholds", "pruning_step"])
    assert int(d["pruning_step"]) == 9 and d["prune_thresholds"].dtype == np.float32
    assert all(d["prune_mask_%s" % nm].dtype == np.float32 for nm in names)

    eng2 = PruneEngine(spec, O.init_weights(spec, np.random.default_rng(9)))
    q = _pruned(eng2, kind, cs, cp, S.ConstantSparsity(0.6, 0, frequency=2))
    q.load_weights(str(tmp_path / "pruned"))
    assert q.pruning_step == 9
    assert np.array_equal(eng2.theta, eng.theta.astype(f32).astype(np.float64))
    assert all(np.array_equal(a, b) for a, b in zip(eng2.masks, eng.masks))
    assert np.array_equal(np.array(eng2.thr, f32), np.array(eng.thr, f32))
    # an unpruned model reads the pruned file's weights and ignores the rest
    r = _model(PruneEngine(spec, ws), kind, cs, cp)
    r.compile(nif_amd.Adam(1e-2), "mse")
    r.load_weights(str(tmp_path / "pruned"))


# ---- data parallel (gloo, world 2) ----------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


N_LOCAL = (40, 25)      # batches 16, 16, 8 on rank 0 and 16, 9, - on rank 1: rank 1 joins the third step with no rows


def _worker(rank, world, port, outdir):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank)})
    import torch.distributed as td
    td.init_process_group("gloo")
    import nif_amd
    from nif_amd import distributed as dist
    from nif_amd import sparsity as S
    from tests.doubles import GlooComm
    dist.install(GlooComm())
    kind, cs, cp, spec, ws, x, y = _problem("ms_plain", n=sum(N_LOCAL))
    eng = PruneEngine(spec, ws)
    p = S.prune_low_magnitude(_model(eng, kind, cs, cp), pruning_schedule=S.PolynomialDecay(0.3, 0.8, 0, 4, frequency=1))
    p.compile(nif_amd.Adam(1e-2), "mse")
    lo = sum(N_LOCAL[:rank]); hi = lo + N_LOCAL[rank]
    p.fit(x[lo:hi], y[lo:hi], batch_size=16, epochs=2, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    upd = [c[1] for c in eng.calls if c[0] == "prune_update"]
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), theta=eng.theta, upd=np.array(upd), step=p.pruning_step,
             masks=np.concatenate(eng.masks))
    dist.shutdown()
    if td.is_initialized():
        td.destroy_process_group()


def test_two_rank_pruned_fit_makes_the_same_decisions(tmp_path):
    pytest.importorskip("torch")
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert int(r0["step"]) == int(r1["step"]) == 5            # 3 steps per epoch on both ranks, the empty one included
    assert r0["upd"].shape[0] == 5 and np.array_equal(r0["upd"], r1["upd"])
    assert np.array_equal(r0["masks"], r1["masks"]) and np.array_equal(r0["theta"], r1["theta"])
