"""CPU tests of Keras' use_ema: the constructor keywords of Adam and the Keras kinds, the overwrite rule as a function of (t, f), and
the host logic of Model.fit / save_weights / load_weights on an engine double that keeps the average in NumPy (the state set before
the first step and cleared afterwards, the one finalize_variable_values behind the last epoch).  The semantics are Keras 2.11's,
restated from its documentation; they are not pinned by a TensorFlow run."""
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests.cfgs import ALL_SMALL
from tests.doubles import OracleEngine

f32 = np.float32


# ---- constructors ------------------------------------------------------------------------------------------------------------------
def test_constructors_take_the_ema_keywords():
    from nif_amd import optimizers as P
    a = P.Adam(use_ema=True)
    assert a.use_ema is True and a.ema_momentum == 0.99 and a.ema_overwrite_frequency is None
    assert a.is_plain                                    # the average is context state: plain Adam keeps nif_adam_step_dev
    s = P.SGD(use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=3)
    assert (s.use_ema, s.ema_momentum, s.ema_overwrite_frequency) == (True, 0.9, 3)
    assert P.ema_of(s) == (0.9, 3) and P.ema_of(a) == (0.99, None) and P.ema_of(P.Adam()) is None
    for cls in (P.Adam, P.AdamW, P.SGD, P.RMSprop, P.Adagrad, P.Adamax):
        o = cls(use_ema=True, ema_momentum=0.5, ema_overwrite_frequency=2)
        assert (o.use_ema, o.ema_momentum, o.ema_overwrite_frequency) == (True, 0.5, 2)
        assert not cls().use_ema
        assert bytes(o.as_opt()) == bytes(cls().as_opt())      # nothing of it travels in the nif_opt


def test_bad_momentum_and_frequency_raise_only_with_use_ema():
    from nif_amd import optimizers as P
    for mom in (-0.1, 1.5, float("nan"), "0.9", None):
        with pytest.raises(ValueError, match="ema_momentum"):
            P.Adam(use_ema=True, ema_momentum=mom)
    for f in (0, -3, 2.5, "3", True):
        with pytest.raises(ValueError, match="ema_overwrite_frequency"):
            P.SGD(use_ema=True, ema_overwrite_frequency=f)
    for mom in (0, 0.0, 1, 1.0):
        assert P.Adam(use_ema=True, ema_momentum=mom).ema_momentum == float(mom)
    # with use_ema false the other two keywords are ignored: kept as given, not judged
    o = P.RMSprop(ema_momentum=7.0, ema_overwrite_frequency=-2)
    assert not o.use_ema and P.ema_of(o) is None
    P.Adam(use_ema=False, ema_momentum="x", ema_overwrite_frequency=0.5)


def test_config_round_trip():
    from nif_amd import optimizers as P
    for o in (P.Adam(use_ema=True), P.SGD(use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=3), P.AdamW(use_ema=True, amsgrad=True),
              P.Adagrad(), P.Adamax(P.schedules.CosineDecay(1e-3, 5), use_ema=True, ema_overwrite_frequency=1)):
        cfg = o.get_config()
        assert cfg["use_ema"] == o.use_ema and cfg["ema_momentum"] == o.ema_momentum
        assert cfg["ema_overwrite_frequency"] == o.ema_overwrite_frequency
        o2 = type(o).from_config(cfg)
        assert o2.get_config() == cfg
        assert (o2.use_ema, o2.ema_momentum, o2.ema_overwrite_frequency) == (o.use_ema, o.ema_momentum, o.ema_overwrite_frequency)


def test_lion_and_adabelief_refuse_the_keyword_as_before():
    from nif_amd import optimizers as P
    for cls in (P.Lion, P.AdaBeliefOptimizer):
        with pytest.raises(NotImplementedError, match=r"\(use_ema\): not built"):
            cls(use_ema=True)
        assert P.ema_of(cls()) is None


# ---- the overwrite rule ---------------------------------------------------------------------------------------------------------------
def test_overwrite_rule_is_a_pure_function_of_t_and_f():
    """Keras: "every ema_overwrite_frequency steps of iterations, we overwrite the model variable by its moving average"; t counts the
    completed steps, the step that completes t overwrites when t % f == 0"""
    from nif_amd.optimizers import ema_overwrite
    want = {None: [], 1: [1, 2, 3, 4, 5, 6, 7], 3: [3, 6]}
    for f, steps in want.items():
        assert [t for t in range(1, 8) if ema_overwrite(t, f)] == steps, f
        assert all(isinstance(ema_overwrite(t, f), bool) for t in range(1, 8))


# ---- Model.fit on an engine double --------------------------------------------------------------------------------------------------
class EmaEngine(OracleEngine):
    """OracleEngine + Engine.set_ema and slot 3 kept in NumPy: the average is seeded with theta at the first step it does not exist
    for, reset by set_opt_state, updated behind every adam_step_dev with the overwrite rule; every call of the new surface recorded"""

    def __init__(self, spec_oracle, weights):
        OracleEngine.__init__(self, spec_oracle, weights)
        self.shapes = spec_oracle.param_shapes()
        self.ema_now, self.avg = None, None
        self.ema_calls, self.ema_at_step, self.log = [], [], []

    def set_ema(self, momentum=None, overwrite_frequency=None):
        self.ema_now = None if momentum is None else (momentum, overwrite_frequency)
        self.ema_calls.append(self.ema_now)
        self.log.append("set_ema" if momentum is not None else "clear_ema")

    def set_opt_state(self, m, v, step):
        OracleEngine.set_opt_state(self, m, v, step)
        self.avg = None

    def adam_step_dev(self, adam):
        from nif_amd.optimizers import ema_overwrite
        self.ema_at_step.append(self.ema_now)
        self.log.append("step")
        if self.ema_now is not None and self.avg is None:
            self.avg = self.theta.copy()
        OracleEngine.adam_step_dev(self, adam)
        if self.ema_now is not None:
            mom, f = self.ema_now
            self.avg = mom * self.avg + (1.0 - mom) * self.theta
            if ema_overwrite(self.t, f):
                self.theta = self.avg.copy()

    def get_opt_slot(self, slot):
        assert slot == 3
        return np.zeros((self.n_params,), f32) if self.avg is None else self.avg.astype(f32)

    def set_opt_slot(self, slot, values):
        assert slot == 3
        self.avg = np.asarray(values, np.float64).copy()
        self.log.append("set_slot3")

    def set_flat(self, flat):
        self.theta = np.asarray(flat, np.float64).copy()
        self.log.append("set_flat")

    def get_weights(self):
        return [w.astype(f32) for w in O.unflatten(self.o, self.theta)]

    def set_weights(self, weights):
        self.theta = O.flatten([np.asarray(w, np.float64) for w in weights])


def _problem(n=40):
    kind, cs, cp = ALL_SMALL["ms_plain"]
    spec = O.Spec(kind, cs, cp)
    rng = np.random.default_rng(0)
    ws = O.init_weights(spec, rng)
    x = rng.uniform(-1, 1, size=(n, spec.pi + spec.si)).astype(f32)
    y = rng.uniform(-1, 1, size=(n, spec.so)).astype(f32)
    return kind, cs, cp, spec, ws, x, y


def _model(eng, kind, cs, cp):
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    return Model(types.SimpleNamespace(_spec=Spec(kind, cs, cp), _engine=eng), "full")


class _Raise(object):
    def __init__(self, at):
        self.at = at

    def on_epoch_end(self, epoch, logs=None):
        if epoch == self.at:
            raise KeyError("callback")


def test_fit_sets_the_state_finalises_once_and_clears_it():
    import nif_amd
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = EmaEngine(spec, ws)
    model = _model(eng, kind, cs, cp)
    th0 = eng.theta.copy()
    model.compile(nif_amd.Adam(1e-2, use_ema=True, ema_momentum=0.9), "mse")
    model.fit(x, y, epochs=2, batch_size=20, shuffle=False, verbose=0)
    assert eng.ema_calls == [(0.9, None), None] and eng.ema_now is None
    assert eng.ema_at_step == [(0.9, None)] * 4
    # set before the first step; the fresh optimizer's average starts as theta_0; ONE finalise behind the last step; cleared at the end
    assert eng.log == ["set_ema", "set_slot3", "step", "step", "step", "step", "set_flat", "clear_ema"]
    assert np.array_equal(eng.theta, eng.avg.astype(f32)) and not np.array_equal(eng.theta, th0)      # (slot 3 travels as float32)
    # the manual sequence: Adam on the double, the average behind every step, theta = average at the end
    ref = OracleEngine(spec, ws)
    avg = ref.theta.copy()
    adam = nif_amd.Adam(1e-2).as_struct()
    xa = ref.alloc(x.size); xa.upload(x)
    ya = ref.alloc(y.size); ya.upload(y)
    for _ in range(2):
        for b0 in (0, 20):
            ref.loss_grad_dev(xa.at(b0 * (spec.pi + spec.si)), ya.at(b0 * spec.so), None, 20, 20)
            ref.adam_step_dev(adam)
            avg = 0.9 * avg + (1.0 - 0.9) * ref.theta
    assert np.array_equal(eng.avg, avg)
    # a second fit of the same optimizer continues the average (no new seed), the frequency reaches the engine
    eng.log.clear()
    model.optimizer.ema_overwrite_frequency = 2
    model.fit(x, y, epochs=1, batch_size=20, shuffle=False, verbose=0)
    assert eng.log == ["set_ema", "step", "step", "set_flat", "clear_ema"] and eng.ema_calls[-2:] == [(0.9, 2), None]


def test_fit_does_not_finalise_without_an_epoch_or_after_an_exception():
    import nif_amd
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = EmaEngine(spec, ws)
    model = _model(eng, kind, cs, cp)
    model.compile(nif_amd.Adam(1e-2, use_ema=True), "mse")
    model.fit(x, y, epochs=2, initial_epoch=2, batch_size=20, shuffle=False, verbose=0)      # initial_epoch >= epochs: no epoch runs
    assert "set_flat" not in eng.log and "step" not in eng.log and eng.ema_calls == [(0.99, None), None]
    eng.log.clear()
    with pytest.raises(KeyError):
        model.fit(x, y, epochs=3, batch_size=20, shuffle=False, verbose=0, callbacks=[_Raise(1)])
    assert eng.log.count("step") == 4 and "set_flat" not in eng.log      # two epochs ran, the call ended by the exception
    assert eng.log[-1] == "clear_ema" and eng.ema_now is None
    assert not np.array_equal(eng.theta, eng.avg)


def test_fit_without_use_ema_runs_on_the_unmodified_double():
    """with use_ema false fit makes the engine calls it made before: the double of tests/doubles.py has none of the new methods"""
    import nif_amd
    kind, cs, cp, spec, ws, x, y = _problem()
    for opt in (nif_amd.Adam(1e-2), nif_amd.Adam(1e-2, use_ema=False, ema_momentum=0.5, ema_overwrite_frequency=2)):
        eng = OracleEngine(spec, ws)
        assert not hasattr(eng, "set_ema") and not hasattr(eng, "get_opt_slot") and not hasattr(eng, "set_flat")
        model = _model(eng, kind, cs, cp)
        model.compile(opt, "mse")
        model.fit(x, y, epochs=2, batch_size=20, shuffle=False, verbose=0)
        assert eng.t == 4
        opt.finalize_variable_values(model)              # a no-op: nothing of the engine is touched
        opt.finalize_variable_values([])


def test_finalize_variable_values_takes_the_variables_or_the_model():
    import nif_amd
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = EmaEngine(spec, ws)
    model = _model(eng, kind, cs, cp)
    opt = nif_amd.SGD(use_ema=True)
    eng.avg = np.arange(eng.n_params, dtype=np.float64)
    opt.finalize_variable_values(model.trainable_variables)
    assert np.array_equal(eng.theta, eng.avg)
    eng.avg = eng.avg + 1.0
    opt.finalize_variable_values(model)
    assert np.array_equal(eng.theta, eng.avg) and eng.log == ["set_flat", "set_flat"]
    with pytest.raises(TypeError):
        opt.finalize_variable_values([object()])


def test_opt_ema_round_trips_through_the_checkpoint_and_old_files_load(tmp_path):
    import nif_amd
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = EmaEngine(spec, ws)
    model = _model(eng, kind, cs, cp)
    model.compile(nif_amd.Adam(1e-2, use_ema=True, ema_momentum=0.9), "mse")
    # before the average exists the file has no opt_ema
    model.save_weights(str(tmp_path / "fresh"))
    assert "opt_ema" not in np.load(str(tmp_path / "fresh.npz"))

    class Save(object):
        def on_epoch_end(self, epoch, logs=None):
            model.save_weights(str(tmp_path / "mid"))      # (behind the epoch, ahead of the finalise)

    model.fit(x, y, epochs=1, batch_size=20, shuffle=False, verbose=0, callbacks=[Save()])
    d = np.load(str(tmp_path / "mid.npz"))
    assert "opt_ema" in d and "adam_m" in d and int(d["adam_step"]) == 2
    assert not np.array_equal(d["opt_ema"], O.flatten([d["w%03d" % i] for i in range(len(eng.shapes))]).astype(f32))
    eng2 = EmaEngine(spec, O.init_weights(spec, np.random.default_rng(9)))
    model2 = _model(eng2, kind, cs, cp)
    model2.compile(nif_amd.Adam(1e-2, use_ema=True, ema_momentum=0.9), "mse")
    model2.load_weights(str(tmp_path / "mid"))
    assert eng2.log == ["set_slot3"]                       # behind set_opt_state, which resets the average
    assert np.array_equal(eng2.avg.astype(f32), d["opt_ema"]) and eng2.t == 2
    assert np.array_equal(eng2.m, d["adam_m"])
    # the other layout (a nif_opt kind)
    eng3 = EmaEngine(spec, ws)
    model3 = _model(eng3, kind, cs, cp)
    model3.compile(nif_amd.SGD(1e-2, use_ema=True), "mse")
    eng3.avg = eng3.theta + 1.0
    model3.save_weights(str(tmp_path / "sgd"))
    d3 = np.load(str(tmp_path / "sgd.npz"))
    assert "opt_kind" in d3 and np.array_equal(d3["opt_ema"], eng3.avg.astype(f32))
    eng3.avg = None
    model3.load_weights(str(tmp_path / "sgd"))
    assert np.array_equal(eng3.avg.astype(f32), d3["opt_ema"])
    # a model compiled without use_ema writes the old layout and ignores the array of a file that has it
    eng4 = EmaEngine(spec, ws)
    model4 = _model(eng4, kind, cs, cp)
    model4.compile(nif_amd.Adam(1e-2), "mse")
    model4.load_weights(str(tmp_path / "mid"))
    assert eng4.avg is None and eng4.t == 2
    model4.save_weights(str(tmp_path / "old"))
    assert "opt_ema" not in np.load(str(tmp_path / "old.npz"))
    # an old-layout file loads into a use_ema model: weights and Adam slots, no average (the next step seeds it)
    eng5 = EmaEngine(spec, O.init_weights(spec, np.random.default_rng(9)))
    model5 = _model(eng5, kind, cs, cp)
    model5.compile(nif_amd.Adam(1e-2, use_ema=True), "mse")
    model5.load_weights(str(tmp_path / "old"))
    assert eng5.avg is None and eng5.t == 2 and np.array_equal(eng5.theta, eng4.theta)
    model5.fit(x, y, epochs=1, batch_size=20, shuffle=False, verbose=0)
    assert eng5.log == ["set_ema", "step", "step", "set_flat", "clear_ema"]      # (not fresh: the engine seeds at the first step)


def test_pruned_model_with_use_ema_is_refused():
    import nif_amd
    from nif_amd import sparsity as S
    from tests.test_pruning import PruneEngine
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = PruneEngine(spec, ws)
    p = S.prune_low_magnitude(_model(eng, kind, cs, cp))
    p.compile(nif_amd.Adam(1e-2, use_ema=True), "mse")
    n = len(eng.calls)
    with pytest.raises(NotImplementedError, match="use_ema"):
        p.fit(x, y, epochs=1, batch_size=20, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    assert len(eng.calls) == n                           # refused when fit starts: nothing reached the engine
    p.compile(nif_amd.Adam(1e-2), "mse")
    p.fit(x, y, epochs=1, batch_size=20, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
