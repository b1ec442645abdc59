"""CPU tests of Keras 2.11's SGD, RMSprop, Adagrad, Adamax, AdamW, amsgrad Adam and of the per-step learning-rate schedules
(nif_amd.optimizers, nif_amd.optimizers.schedules): constructors, names, refusals, the packing into the 72-byte nif_opt, the host
function that forms the step's learning rate (nif_opt_scalars: the code every eager step runs and every captured block compiles)
against the float64 schedules, and Model.fit / save_weights / load_weights on an engine double whose update is the NumPy restatement
of tests/keras_opt_ref.py.  The formulas are restated from Keras 2.11; no TensorFlow run pins them."""
import ctypes
import types

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import keras_opt_ref as K
from tests.cfgs import ALL_SMALL
from tests.doubles import OracleEngine

f32 = np.float32


def _x(v):
    """a float32-exact Python float: what the struct holds is what the float64 schedule object computes with"""
    return float(f32(v))


# ---- constructors, names, refusals --------------------------------------------------------------------------------------------------
def test_constructor_defaults_are_keras_2_11s():
    import nif_amd
    from nif_amd import optimizers as P
    for name in ("SGD", "RMSprop", "Adagrad", "Adamax", "AdamW", "Adam"):
        assert getattr(nif_amd, name) is getattr(P, name)
    s = P.SGD()
    assert (s.learning_rate, s.momentum, s.nesterov, s.name) == (0.01, 0.0, False, "SGD")
    r = P.RMSprop()
    assert (r.learning_rate, r.rho, r.momentum, r.epsilon, r.centered, r.name) == (0.001, 0.9, 0.0, 1e-7, False, "RMSprop")
    g = P.Adagrad()
    assert (g.learning_rate, g.initial_accumulator_value, g.epsilon, g.name) == (0.001, 0.1, 1e-7, "Adagrad")
    x = P.Adamax()
    assert (x.learning_rate, x.beta_1, x.beta_2, x.epsilon, x.name) == (0.001, 0.9, 0.999, 1e-7, "Adamax")
    w = P.AdamW()
    assert (w.learning_rate, w.weight_decay, w.beta_1, w.beta_2, w.epsilon, w.amsgrad, w.name) == (0.001, 0.004, 0.9, 0.999, 1e-7, False, "AdamW")
    a = P.Adam()
    assert (a.learning_rate, a.beta_1, a.beta_2, a.epsilon, a.amsgrad) == (0.001, 0.9, 0.999, 1e-7, False)
    assert P.Adam(amsgrad=False).is_plain and not P.Adam(amsgrad=True).is_plain and not w.is_plain
    assert P.SGD(lr=0.5).learning_rate == 0.5                       # Keras' legacy alias
    for o in (s, r, g, x, w, a):
        assert o.lr == o.learning_rate and (o.clipnorm, o.clipvalue, o.global_clipnorm) == (None, None, None)
        o.lr = 0.25
        assert o.learning_rate == 0.25 and o.as_opt().lr == 0.25


def test_get_config_round_trip():
    from nif_amd import optimizers as P
    S = P.schedules
    opts = [P.SGD(0.1, momentum=0.9, nesterov=True, clipnorm=1.0), P.RMSprop(1e-2, rho=0.8, momentum=0.5, epsilon=1e-6, centered=True),
            P.Adagrad(0.3, initial_accumulator_value=0.0, epsilon=1e-5, clipvalue=0.5), P.Adamax(2e-3, 0.8, 0.9, 1e-6),
            P.AdamW(1e-3, weight_decay=1e-2, amsgrad=True, global_clipnorm=2.0), P.Adam(3e-3, amsgrad=True),
            P.Adam(S.CosineDecay(1e-2, 100, alpha=0.1)), P.SGD(S.PolynomialDecay(0.1, 10, 0.01, power=2.0, cycle=True)),
            P.RMSprop(S.ExponentialDecay(1e-3, 50, 0.9, staircase=True)), P.Adamax(S.InverseTimeDecay(1e-3, 7, 0.5))]
    for o in opts:
        cfg = o.get_config()
        o2 = type(o).from_config(cfg)
        assert o2.get_config() == cfg
        assert bytes(o2.as_opt()) == bytes(o.as_opt())
    for sch in (S.ExponentialDecay(1e-3, 50, 0.9, staircase=True), S.InverseTimeDecay(1e-3, 7, 0.5), S.CosineDecay(1e-2, 100, 0.1),
                S.PolynomialDecay(0.1, 10, 0.01, 2.0, True)):
        assert type(sch).from_config(sch.get_config()).get_config() == sch.get_config()


def test_get_resolves_keras_names_and_keeps_the_refusals():
    from nif_amd import optimizers as P
    for name, cls in (("sgd", P.SGD), ("rmsprop", P.RMSprop), ("adagrad", P.Adagrad), ("adamax", P.Adamax), ("adamw", P.AdamW),
                      ("adam", P.Adam), ("RMSprop", P.RMSprop), ("SGD", P.SGD)):
        assert type(P.get(name)) is cls
    o = P.Adagrad()
    assert P.get(o) is o
    with pytest.raises(NotImplementedError):
        P.get("lion")
    with pytest.raises(NotImplementedError, match="Nadam"):
        P.get("nadam")
    with pytest.raises(NotImplementedError, match="Nadam"):
        P.Nadam()
    with pytest.raises(NotImplementedError, match="PiecewiseConstantDecay"):
        P.schedules.PiecewiseConstantDecay([10], [1e-3, 1e-4])
    with pytest.raises(NotImplementedError, match="CosineDecayRestarts"):
        P.schedules.CosineDecayRestarts(1e-3, 10)
    with pytest.raises(NotImplementedError):
        P.L4Adam()
    sched = P.schedules.CosineDecay(1e-3, 10)
    with pytest.raises(NotImplementedError, match="learning_rate"):
        P.Lion(learning_rate=sched)
    with pytest.raises(NotImplementedError, match="learning_rate"):
        P.AdaBeliefOptimizer(learning_rate=sched)
    with pytest.raises(NotImplementedError, match="clipnorm"):
        P.Lion(clipnorm=1.0)
    with pytest.raises(NotImplementedError):
        P.Adam(learning_rate=lambda step: 1e-3)                   # a Python callable cannot run inside the step
    with pytest.raises(ValueError, match="At most one"):
        P.SGD(clipnorm=1.0, clipvalue=1.0)
    with pytest.raises(ValueError):
        P.SGD(momentum=1.5)
    with pytest.raises(TypeError, match="rho"):
        P.SGD(rho=0.5)
    with pytest.raises(NotImplementedError, match="decay_steps"):
        P.schedules.CosineDecay(1e-3, 10.5)


def test_clip_keywords_and_centralisation_work_on_the_new_classes():
    from nif_amd import optimizers as P
    assert P.grad_transform_of(P.SGD()) is None
    assert P.grad_transform_of(P.RMSprop(clipnorm=2.0)) == {"clipnorm": 2.0, "clipvalue": 0.0, "global_clipnorm": 0.0}
    assert P.grad_transform_of(P.AdamW(global_clipnorm=3.0))["global_clipnorm"] == 3.0
    o = P.Adagrad(clipvalue=0.5)
    o.get_gradients = P.centralized_gradients_for_optimizer(o)
    assert P.grad_transform_of(o) == {"centralize": True, "gtcf": True, "clipnorm": 0.0, "clipvalue": 0.5}


# ---- packing ------------------------------------------------------------------------------------------------------------------------
def test_nif_opt_is_72_bytes_and_default_adam_is_the_parents_bytes():
    """the all-default Adam as a nif_opt: kind 0, flags 0, lr 1e-3, 0.9, 0.999, 1e-7 as float32 and 48 zero bytes -- the struct the
    parent commit's nif_adam_step_dev built from its nif_adam (opt_of_adam), recorded here"""
    from nif_amd import _lib
    from nif_amd.optimizers import Adam
    assert ctypes.sizeof(_lib.nif_opt) == 72
    want = bytes.fromhex("00000000" "00000000" "6f12833a" "6666663f" "77be7f3f" "95bfd633") + bytes(48)
    assert bytes(Adam().as_opt()) == want
    assert bytes(Adam().as_struct()) == want[8:24]
    assert bytes(Adam(amsgrad=False).as_opt()) == want
    for fld, off in (("sched", 44), ("total_steps", 48), ("decay_steps", 56), ("sched_a", 60), ("sched_b", 64), ("init_acc", 68)):
        assert getattr(_lib.nif_opt, fld).offset == off


def test_as_opt_field_packing():
    from nif_amd import _lib
    from nif_amd import optimizers as P
    S = P.schedules

    def fields(o):
        return {nm: getattr(o, nm) for nm, _ in _lib.nif_opt._fields_}

    def expect(o, **kw):
        got = fields(o)
        for k, v in kw.items():
            assert got.pop(k) == (f32(v) if isinstance(v, float) else v), k
        assert all(v == 0 for v in got.values()), got              # everything not named is zero

    expect(P.SGD(0.1).as_opt(), kind=3, lr=0.1)
    expect(P.SGD(0.1, momentum=0.9, nesterov=True).as_opt(), kind=3, lr=0.1, beta1=0.9, flags=_lib.OPT_NESTEROV)
    expect(P.RMSprop(centered=True, momentum=0.5).as_opt(), kind=4, lr=0.001, beta1=0.5, beta2=0.9, eps=1e-7, flags=_lib.OPT_CENTERED)
    expect(P.Adagrad().as_opt(), kind=5, lr=0.001, eps=1e-7, init_acc=0.1)
    expect(P.Adamax().as_opt(), kind=6, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-7)
    expect(P.Adam(amsgrad=True).as_opt(), kind=0, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-7, flags=_lib.OPT_AMSGRAD)
    expect(P.AdamW(amsgrad=True).as_opt(), kind=0, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-7, weight_decay=0.004,
           flags=_lib.OPT_AMSGRAD | _lib.OPT_DECOUPLED_WD)
    expect(P.SGD(S.ExponentialDecay(0.1, 50, 0.9, staircase=True)).as_opt(), kind=3, lr=0.1, decay_steps=50, sched_a=0.9,
           sched=_lib.SCHED_EXPONENTIAL | _lib.SCHED_STAIRCASE)
    expect(P.SGD(S.InverseTimeDecay(0.1, 50, 0.5)).as_opt(), kind=3, lr=0.1, decay_steps=50, sched_a=0.5, sched=_lib.SCHED_INVERSE_TIME)
    expect(P.Adagrad(S.CosineDecay(0.1, 7, alpha=0.25)).as_opt(), kind=5, lr=0.1, eps=1e-7, init_acc=0.1, decay_steps=7, sched_a=0.25,
           sched=_lib.SCHED_COSINE)
    expect(P.Adam(S.PolynomialDecay(0.1, 9, 0.01, power=2.0, cycle=True)).as_opt(), kind=0, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-7,
           decay_steps=9, sched_a=0.01, sched_b=2.0, sched=_lib.SCHED_POLYNOMIAL | _lib.SCHED_CYCLE)
    o = P.Adam(S.CosineDecay(0.1, 7))
    assert o.lr is o.learning_rate and isinstance(o.lr, S.CosineDecay)         # Keras: optimizer.lr returns the schedule
    with pytest.raises(ValueError):
        o.as_struct()


# ---- the host scalar function --------------------------------------------------------------------------------------------------------
def _scalars(o, t):
    from nif_amd import _lib
    out = (ctypes.c_double * 5)()
    _lib.check(_lib.load().nif_opt_scalars(ctypes.byref(o), int(t), out))
    return list(out)


DS = 10


def _schedules():
    from nif_amd.optimizers import schedules as S
    return {
        "exponential": S.ExponentialDecay(_x(1e-2), DS, _x(0.96)),
        "exponential_staircase": S.ExponentialDecay(_x(1e-2), DS, _x(0.96), staircase=True),
        "inverse_time": S.InverseTimeDecay(_x(1e-2), DS, _x(0.5)),
        "inverse_time_staircase": S.InverseTimeDecay(_x(1e-2), DS, _x(0.5), staircase=True),
        "cosine": S.CosineDecay(_x(1e-2), DS),
        "cosine_alpha": S.CosineDecay(_x(1e-2), DS, alpha=_x(0.1)),
        "polynomial": S.PolynomialDecay(_x(1e-2), DS, _x(1e-4), power=_x(1.0)),
        "polynomial_sqrt": S.PolynomialDecay(_x(1e-2), DS, _x(1e-4), power=_x(0.5)),
        "polynomial_cycle": S.PolynomialDecay(_x(1e-2), DS, _x(1e-4), power=_x(2.0), cycle=True),
    }


@pytest.mark.parametrize("name", sorted(_schedules()))
@pytest.mark.parametrize("cls", ["Adam", "SGD", "RMSprop", "Adagrad", "Adamax", "AdamW"])
def test_host_scalars_follow_the_float64_schedule(name, cls):
    """out[0] of nif_opt_scalars at t in {1, 2, decay_steps, decay_steps + 1, 3 decay_steps + 7} against the schedule object's float64
    value at Keras' step = t - 1 and against the independent restatement of keras_opt_ref: within one float32 rounding (1.2e-7
    relative); the constants are float32-exact, so that the struct holds what the object computes with.  Measured: <= 4.4e-16"""
    from nif_amd import optimizers as P
    sch = _schedules()[name]
    o = getattr(P, cls)(sch).as_opt()
    worst = 0.0
    for t in (1, 2, DS, DS + 1, 3 * DS + 7):
        got = _scalars(o, t)[0]
        for want in (float(sch(t - 1)), K.schedule_lr(o, t - 1)):
            worst = max(worst, 0.0 if got == want else abs(got - want) / abs(want))      # (cosine's end is exactly 0 on both sides)
    print("WORST", name, cls, worst)
    assert worst <= 1.2e-7
    assert _scalars(o, 1)[0] == _x(1e-2)                                      # step 0: the initial learning rate


def test_schedule_values_at_known_points():
    s = _schedules()
    lr, end = _x(1e-2), _x(1e-4)
    assert np.isclose(s["exponential"](5), lr * _x(0.96) ** 0.5, rtol=1e-14)
    assert s["exponential_staircase"](9) == lr and np.isclose(s["exponential_staircase"](19), lr * _x(0.96), rtol=1e-14)
    assert np.isclose(s["inverse_time"](20), lr / 2.0, rtol=1e-14) and s["inverse_time_staircase"](9) == lr
    assert np.isclose(s["cosine"](5), lr / 2, rtol=1e-12) and abs(s["cosine"](10)) < 1e-18 and s["cosine"](99) == s["cosine"](10)
    assert np.isclose(s["cosine_alpha"](1000), lr * _x(0.1), rtol=1e-12)
    assert np.isclose(s["polynomial"](5), (lr + end) / 2, rtol=1e-12) and s["polynomial"](37) == end
    assert s["polynomial_cycle"](0) == lr and s["polynomial_cycle"](10) == end            # the cycle's end, then a new cycle of 20
    assert np.isclose(s["polynomial_cycle"](15), (lr - end) * 0.25 ** 2 + end, rtol=1e-12)
    assert s["cosine"](np.arange(3)).dtype == np.float64


def test_invalid_structs_are_refused():
    from nif_amd import _lib
    from nif_amd import optimizers as P
    lib = _lib.load()
    out = (ctypes.c_double * 5)()

    def rc(o, **kw):
        for k, v in kw.items():
            setattr(o, k, v)
        return lib.nif_opt_scalars(ctypes.byref(o), 1, out)

    sched = P.schedules.CosineDecay(1e-3, 10)
    assert rc(P.SGD().as_opt()) == 0
    assert rc(P.Lion().as_opt(), sched=_lib.SCHED_COSINE, decay_steps=10) == 0           # a schedule is any kind's at the C level
    assert rc(P.Lion(decay=1e-3).as_opt(), sched=_lib.SCHED_COSINE, decay_steps=10) != 0  # the legacy decay and a schedule together
    assert rc(P.SGD().as_opt(), kind=7) != 0
    assert rc(P.SGD().as_opt(), flags=_lib.OPT_AMSGRAD) != 0
    assert rc(P.SGD().as_opt(), flags=32) != 0
    assert rc(P.Adam().as_opt(), flags=_lib.OPT_CENTERED) != 0
    assert rc(P.Adam().as_opt(), weight_decay=0.1) != 0                                  # needs the decoupled flag
    assert rc(P.Adam().as_opt(), init_acc=0.1) != 0
    assert rc(P.SGD().as_opt(), decay_steps=5) != 0                                      # schedule fields without a schedule
    assert rc(P.SGD(sched).as_opt(), decay_steps=0) != 0
    assert rc(P.SGD(sched).as_opt(), sched=_lib.SCHED_COSINE | _lib.SCHED_STAIRCASE) != 0
    assert rc(P.SGD(sched).as_opt(), sched=5) != 0
    assert rc(P.SGD().as_opt(), decay=1e-3) != 0


# ---- Model.fit on an engine double --------------------------------------------------------------------------------------------------
class KerasOptEngine(OracleEngine):
    """OracleEngine + nif_opt_step_dev for the Keras kinds: the update is keras_opt_ref's restatement (float32)"""

    def __init__(self, spec_oracle, weights):
        OracleEngine.__init__(self, spec_oracle, weights)
        self.s2 = np.zeros_like(self.theta)
        self.shapes = spec_oracle.param_shapes()
        self.opts = []

    def opt_step_dev(self, opt):
        self.t += 1
        self.opts.append(bytes(opt))
        th, s0, s1, s2 = K.update(opt, self.t, self.theta, self.grad_buf[:-1], self.m, self.v, self.s2)
        self.theta, self.m, self.v, self.s2 = (np.asarray(a, np.float64) for a in (th, s0, s1, s2))
        self.calls.append(("opt_step", int(opt.kind), int(opt.flags)))

    def adam_step_dev(self, adam):
        self.calls.append(("adam_step",))
        OracleEngine.adam_step_dev(self, adam)

    def get_opt_slot(self, slot):
        return np.asarray((self.m, self.v, self.s2)[slot], f32).copy()

    def set_opt_slot(self, slot, values):
        a = np.asarray(values, np.float64).copy()
        if slot == 0:
            self.m = a
        elif slot == 1:
            self.v = a
        else:
            self.s2 = a

    def get_weights(self):
        return [w.astype(f32) for w in O.unflatten(self.o, self.theta)]

    def set_weights(self, weights):
        self.theta = O.flatten([np.asarray(w, np.float64) for w in weights])


def _problem(n=72):
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


def test_fit_with_amsgrad_adam_hands_the_engine_the_amsgrad_flag():
    """Adam(amsgrad=True) reaches the engine as a nif_opt with NIF_OPT_AMSGRAD set on every step (the keyword used to be swallowed and
    the model trained with plain Adam through nif_adam_step_dev); plain Adam still takes nif_adam_step_dev"""
    from nif_amd import _lib
    from nif_amd.optimizers import Adam
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = KerasOptEngine(spec, ws)
    model = _model(eng, kind, cs, cp)
    eng.s2[:] = 7.0
    model.compile(Adam(1e-2, amsgrad=True), "mse")
    model.fit(x, y, batch_size=16, epochs=2, shuffle=False, verbose=0)
    steps = [c for c in eng.calls if c[0] in ("opt_step", "adam_step")]
    assert len(steps) == 10 and all(c == ("opt_step", _lib.OPT_ADAM, _lib.OPT_AMSGRAD) for c in steps)
    assert eng.t == 10 and np.all(eng.s2 < 7.0) and eng.s2.max() > 0       # vhat zeroed before the first step, then max(vhat, v)
    assert np.array_equal(eng.s2, np.maximum(eng.s2, eng.v))
    eng.calls.clear()
    model.compile(Adam(1e-2), "mse")
    model.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
    assert [c[0] for c in eng.calls if c[0].endswith("_step")] == ["adam_step"] * 5


def test_fit_with_a_schedule_and_each_new_kind_runs_the_restated_sequence():
    from nif_amd import optimizers as P
    kind, cs, cp, spec, ws, x, y = _problem()
    make = [lambda: P.SGD(P.schedules.ExponentialDecay(1e-3, 3, 0.5), momentum=0.9, nesterov=True), lambda: P.RMSprop(centered=True, momentum=0.5),
            lambda: P.Adagrad(0.05), lambda: P.Adamax(), lambda: P.AdamW(amsgrad=True)]
    for mk in make:
        eng = KerasOptEngine(spec, ws)
        model = _model(eng, kind, cs, cp)
        model.compile(mk(), "mse")
        model.fit(x, y, batch_size=16, epochs=2, shuffle=False, verbose=0)
        assert eng.t == 10 and set(eng.opts) == {bytes(mk().as_opt())}
        # the manual sequence
        o = mk().as_opt()
        th = O.flatten(ws)
        s0 = np.full_like(th, o.init_acc, dtype=f32); s1 = np.zeros_like(s0); s2 = np.zeros_like(s0)
        t = 0
        for _ in range(2):
            for b0 in range(0, 72, 16):
                _, g = O.loss_and_grad(spec, O.unflatten(spec, th), x[b0:b0 + 16].astype(np.float64), y[b0:b0 + 16].astype(np.float64))
                t += 1
                th, s0, s1, s2 = K.update(o, t, th, O.flatten(g), s0, s1, s2)
                th = th.astype(np.float64)
        assert np.array_equal(eng.theta, th)
        assert not np.array_equal(th, O.flatten(ws))


def test_learning_rate_scheduler_refuses_a_schedule_object():
    from nif_amd import optimizers as P
    from nif_amd.callbacks import LearningRateScheduler
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = KerasOptEngine(spec, ws)
    model = _model(eng, kind, cs, cp)
    model.compile(P.Adam(P.schedules.CosineDecay(1e-3, 10)), "mse")
    with pytest.raises(TypeError, match="schedule"):
        model.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0, callbacks=[LearningRateScheduler(lambda ep, lr: lr * 0.5)])
    model.compile(P.SGD(2.0 ** -9), "mse")
    model.fit(x, y, batch_size=16, epochs=2, shuffle=False, verbose=0, callbacks=[LearningRateScheduler(lambda ep, lr: lr * 0.5)])
    assert model.optimizer.learning_rate == 2.0 ** -11


def test_save_load_carries_the_new_slots_and_the_kind(tmp_path):
    from nif_amd import optimizers as P
    kind, cs, cp, spec, ws, x, y = _problem()
    cases = {"sgd": (lambda: P.SGD(1e-3, momentum=0.9), 1), "rmsprop_centered": (lambda: P.RMSprop(centered=True, momentum=0.5), 3),
             "adagrad": (lambda: P.Adagrad(0.05), 1), "adamax": (lambda: P.Adamax(), 2), "adam_ams": (lambda: P.Adam(amsgrad=True), 3),
             "adamw": (lambda: P.AdamW(), 2)}
    for name, (mk, nslot) in cases.items():
        eng = KerasOptEngine(spec, ws)
        model = _model(eng, kind, cs, cp)
        model.compile(mk(), "mse")
        model.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
        f = str(tmp_path / name)
        model.save_weights(f)
        d = np.load(f + ".npz")
        assert int(d["opt_step"]) == 5 and "adam_m" not in d and int(d["opt_kind"]) == mk().kind
        assert [k in d for k in ("opt_m", "opt_v", "opt_vhat")] == [True, nslot >= 2, nslot >= 3]
        eng2 = KerasOptEngine(spec, O.init_weights(spec, np.random.default_rng(5)))
        model2 = _model(eng2, kind, cs, cp)
        model2.compile(mk(), "mse")
        model2.load_weights(f)
        assert eng2.t == 5
        for s in range(nslot):
            assert np.array_equal(eng2.get_opt_slot(s), eng.get_opt_slot(s))
        model.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
        model2.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
        assert np.array_equal(eng2.theta, eng.theta)
        # a file of another kind: weights only, with a warning
        for other in (P.Adam(), P.Lion(), P.RMSprop() if name != "rmsprop_centered" else P.SGD()):
            eng3 = KerasOptEngine(spec, O.init_weights(spec, np.random.default_rng(6)))
            model3 = _model(eng3, kind, cs, cp)
            model3.compile(other, "mse")
            with pytest.warns(UserWarning, match="not restored"):
                model3.load_weights(f)
            assert eng3.t == 0
    # AdamW and Adam share kind and slots but not the update: the flag decides
    eng4 = KerasOptEngine(spec, ws)
    model4 = _model(eng4, kind, cs, cp)
    model4.compile(P.AdamW(amsgrad=True), "mse")
    with pytest.warns(UserWarning, match="not restored"):
        model4.load_weights(str(tmp_path / "adam_ams"))
    # a schedule does not change plain Adam's file
    eng5 = KerasOptEngine(spec, ws)
    model5 = _model(eng5, kind, cs, cp)
    model5.compile(P.Adam(P.schedules.CosineDecay(1e-3, 10)), "mse")
    model5.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
    model5.save_weights(str(tmp_path / "adam_sched"))
    assert "adam_m" in np.load(str(tmp_path / "adam_sched.npz"))
