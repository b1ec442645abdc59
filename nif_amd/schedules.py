"""tf.keras.optimizers.schedules.* as `learning_rate` of Adam, AdamW, SGD, RMSprop, Adagrad and Adamax (nif_amd.optimizers.schedules).
The formulas are restated from Keras 2.11 and are not pinned by a TensorFlow run (parity unpinned by TensorFlow).  A schedule is a
function of Keras' `step` = optimizer.iterations (0 at the first update).  `schedule(step)` evaluates it in float64 NumPy on the host;
training evaluates the same formula in fp64 inside the optimizer step (k_opt.hip, opt_scalars) from the nif_opt fields `pack` fills --
per captured step on the device, so an epoch replayed from a graph follows the schedule step by step.  The struct carries the
constants as float32 and decay_steps as int32."""
import numbers

import numpy as np

from . import _lib


def _real(cls, name, v):
    if isinstance(v, bool) or not isinstance(v, (numbers.Real, np.floating, np.integer)):
        raise TypeError("%s(%s=%r): a number" % (cls, name, v))
    return float(v)


def _steps(cls, v):
    if isinstance(v, bool) or not isinstance(v, (numbers.Real, np.floating, np.integer)) or float(v) != int(v):
        raise NotImplementedError("%s(decay_steps=%r): a whole number of steps (the optimizer struct holds an int32)" % (cls, v))
    if not 0 < int(v) < 2 ** 31:
        raise ValueError("%s(decay_steps=%r): within [1, 2^31)" % (cls, v))
    return int(v)


class LearningRateSchedule(object):
    """base of the built schedules; a subclass of the user's own cannot run inside the optimizer kernels"""

    def __call__(self, step):
        raise NotImplementedError("LearningRateSchedule: built are ExponentialDecay, InverseTimeDecay, CosineDecay and PolynomialDecay "
                                  "(a Python schedule cannot be evaluated inside a captured optimizer step)")

    def get_config(self):
        raise NotImplementedError

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def pack(self, o):
        """the schedule into a _lib.nif_opt: lr, sched, decay_steps, sched_a, sched_b"""
        raise NotImplementedError


class ExponentialDecay(LearningRateSchedule):
    """lr * decay_rate ^ (step / decay_steps); staircase: the exponent floored"""
    _KIND = _lib.SCHED_EXPONENTIAL

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        cls = type(self).__name__
        self.initial_learning_rate = _real(cls, "initial_learning_rate", initial_learning_rate)
        self.decay_steps = _steps(cls, decay_steps)
        self.decay_rate = _real(cls, "decay_rate", decay_rate)
        self.staircase = bool(staircase)
        self.name = name

    def _p(self, step):
        p = np.asarray(step, dtype=np.float64) / float(self.decay_steps)
        return np.floor(p) if self.staircase else p

    def __call__(self, step):
        return np.float64(self.initial_learning_rate * np.power(self.decay_rate, self._p(step)))

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps, "decay_rate": self.decay_rate,
                "staircase": self.staircase, "name": self.name}

    def pack(self, o):
        o.lr, o.decay_steps, o.sched_a, o.sched_b = self.initial_learning_rate, self.decay_steps, self.decay_rate, 0.0
        o.sched = self._KIND | (_lib.SCHED_STAIRCASE if self.staircase else 0)


class InverseTimeDecay(ExponentialDecay):
    """lr / (1 + decay_rate * step / decay_steps); staircase: the quotient floored"""
    _KIND = _lib.SCHED_INVERSE_TIME

    def __call__(self, step):
        return np.float64(self.initial_learning_rate / (1.0 + self.decay_rate * self._p(step)))


class CosineDecay(LearningRateSchedule):
    """lr * ((1 - alpha) * 0.5 * (1 + cos(pi * min(step, decay_steps) / decay_steps)) + alpha)"""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, name=None):
        self.initial_learning_rate = _real("CosineDecay", "initial_learning_rate", initial_learning_rate)
        self.decay_steps = _steps("CosineDecay", decay_steps)
        self.alpha = _real("CosineDecay", "alpha", alpha)
        self.name = name

    def __call__(self, step):
        q = np.minimum(np.asarray(step, dtype=np.float64), float(self.decay_steps)) / float(self.decay_steps)
        return np.float64(self.initial_learning_rate * ((1.0 - self.alpha) * 0.5 * (1.0 + np.cos(np.pi * q)) + self.alpha))

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps, "alpha": self.alpha,
                "name": self.name}

    def pack(self, o):
        o.lr, o.decay_steps, o.sched_a, o.sched_b = self.initial_learning_rate, self.decay_steps, self.alpha, 0.0
        o.sched = _lib.SCHED_COSINE


class PolynomialDecay(LearningRateSchedule):
    """(lr - end) * (1 - min(step, decay_steps) / decay_steps) ^ power + end; cycle: decay_steps * max(1, ceil(step / decay_steps))
    takes the place of decay_steps"""

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=0.0001, power=1.0, cycle=False, name=None):
        self.initial_learning_rate = _real("PolynomialDecay", "initial_learning_rate", initial_learning_rate)
        self.decay_steps = _steps("PolynomialDecay", decay_steps)
        self.end_learning_rate = _real("PolynomialDecay", "end_learning_rate", end_learning_rate)
        self.power = _real("PolynomialDecay", "power", power)
        self.cycle = bool(cycle)
        self.name = name

    def __call__(self, step):
        step = np.asarray(step, dtype=np.float64)
        ds = float(self.decay_steps)
        if self.cycle:
            ds = ds * np.maximum(1.0, np.ceil(step / ds))
        q = np.minimum(step, ds) / ds
        return np.float64((self.initial_learning_rate - self.end_learning_rate) * np.power(1.0 - q, self.power) + self.end_learning_rate)

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "end_learning_rate": self.end_learning_rate, "power": self.power, "cycle": self.cycle, "name": self.name}

    def pack(self, o):
        o.lr, o.decay_steps, o.sched_a, o.sched_b = self.initial_learning_rate, self.decay_steps, self.end_learning_rate, self.power
        o.sched = _lib.SCHED_POLYNOMIAL | (_lib.SCHED_CYCLE if self.cycle else 0)


def _not_built(name, why):
    class _NotBuilt(LearningRateSchedule):
        def __init__(self, *args, **kwargs):
            raise NotImplementedError("%s: not built (%s); built are ExponentialDecay, InverseTimeDecay, CosineDecay and PolynomialDecay"
                                      % (name, why))
    _NotBuilt.__name__ = _NotBuilt.__qualname__ = name
    return _NotBuilt


PiecewiseConstantDecay = _not_built("PiecewiseConstantDecay", "its boundaries and values do not fit the optimizer struct")
CosineDecayRestarts = _not_built("CosineDecayRestarts", "its constants do not fit the optimizer struct")
