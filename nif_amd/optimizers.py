"""Optimizers accepted by Model.compile.  The hot path uses stock Keras-2.11 Adam (README.md:33;
SURVEY a-11); the reference's Lion and AdaBeliefOptimizer (nif/optimizers/__init__.py) and Keras 2.11's SGD, RMSprop, Adagrad,
Adamax, AdamW and amsgrad Adam are the other kinds; Adam and the Keras kinds take a nif_amd.optimizers.schedules.* object as
learning_rate.  All update on the k_opt.hip kernels (k_opt, k_reduce_opt, k_opt_dev).  The Keras kinds' formulas are restated from
Keras 2.11 and are not pinned by a TensorFlow run (parity unpinned by TensorFlow).  use_ema / ema_momentum / ema_overwrite_frequency
of Adam and the Keras kinds: the weights' moving average, kept by the same kernels behind every update (slot 3 of the engine;
semantics restated from Keras 2.11's documentation, unpinned by TensorFlow)."""
import numbers

import numpy as np

from . import _lib
from . import schedules


_CLIP_KEYS = ("clipnorm", "clipvalue", "global_clipnorm")


def _clip_constant(name, v):
    """None (off) or a non-negative number, as Keras' optimizer base checks its clip keywords"""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (numbers.Real, np.floating, np.integer)):
        raise TypeError("%s=%r: a number or None" % (name, v))
    if float(v) < 0.0:
        raise ValueError("%s cannot be less than 0. Received: %s=%r." % (name, name, v))
    return float(v)


class _KerasOptimizer(object):
    """what Adam and the Keras-2.11 kinds share: learning_rate as a number or a schedules.* object, Keras' clip keywords (gradient
    clipping per tensor by norm, by value, by the global norm, applied on the device in front of the update, k_gradtf.hip; at most
    one of them, as in Keras), optimizer.lr, get_config / from_config and the nif_opt a step receives"""
    kind = _lib.OPT_ADAM
    amsgrad = False
    _DEFAULT_NAME = None

    def _base(self, learning_rate, clipnorm, clipvalue, global_clipnorm, kwargs, name=None):
        cls = type(self).__name__
        kwargs = dict(kwargs)
        if "lr" in kwargs:
            learning_rate = kwargs.pop("lr")
        kwargs.pop("jit_compile", None)            # (nothing to compile here)
        # Keras' weight averaging (use_ema): validated as Keras' optimizer base does, and only when it is on
        self.use_ema = bool(kwargs.pop("use_ema", False))
        self.ema_momentum = kwargs.pop("ema_momentum", 0.99)
        self.ema_overwrite_frequency = kwargs.pop("ema_overwrite_frequency", None)
        if self.use_ema:
            mom, f = self.ema_momentum, self.ema_overwrite_frequency
            if isinstance(mom, bool) or not isinstance(mom, (numbers.Real, np.floating, np.integer)) or not 0.0 <= float(mom) <= 1.0:
                raise ValueError("`ema_momentum` must be in the range [0, 1]. Received: ema_momentum=%r" % (mom,))
            if f is not None and (isinstance(f, bool) or not isinstance(f, (int, np.integer)) or f < 1):
                raise ValueError("`ema_overwrite_frequency` must be an integer >= 1 or None. Received: ema_overwrite_frequency=%r" % (f,))
            self.ema_momentum = float(mom)
            self.ema_overwrite_frequency = None if f is None else int(f)
        if kwargs.pop("decay", 0):
            raise NotImplementedError("%s(decay=...): Keras 2.11's optimizers take a schedule instead (schedules.InverseTimeDecay)" % cls)
        self._unknown_kwargs(kwargs)
        self.learning_rate = learning_rate
        self.name = self._DEFAULT_NAME if name is None else name
        self.clipnorm = _clip_constant("clipnorm", clipnorm)
        self.clipvalue = _clip_constant("clipvalue", clipvalue)
        self.global_clipnorm = _clip_constant("global_clipnorm", global_clipnorm)
        if sum(v is not None for v in (self.clipnorm, self.clipvalue, self.global_clipnorm)) > 1:
            raise ValueError("At most one of `clipnorm`, `clipvalue` and `global_clipnorm` can be set. Received: clipnorm=%r, "
                             "clipvalue=%r, global_clipnorm=%r." % (clipnorm, clipvalue, global_clipnorm))

    def _unknown_kwargs(self, kwargs):
        if kwargs:
            raise TypeError("%s: unexpected keyword argument(s) %s" % (type(self).__name__, ", ".join(sorted(kwargs))))

    # learning_rate: a float, or a schedule object kept as it is (Keras: optimizer.lr then returns the schedule)
    @property
    def learning_rate(self):
        return self._learning_rate

    @learning_rate.setter
    def learning_rate(self, v):
        if isinstance(v, schedules.LearningRateSchedule):
            if type(v).pack is schedules.LearningRateSchedule.pack:
                raise NotImplementedError("%s(learning_rate=%s): built schedules are ExponentialDecay, InverseTimeDecay, CosineDecay "
                                          "and PolynomialDecay" % (type(self).__name__, type(v).__name__))
            self._learning_rate = v
        elif callable(v):
            raise NotImplementedError("%s(learning_rate=%r): a nif_amd.optimizers.schedules object or a number (a Python callable "
                                      "cannot be evaluated inside the optimizer step)" % (type(self).__name__, v))
        else:
            self._learning_rate = float(v)

    # Keras exposes optimizer.lr / optimizer.learning_rate; LearningRateScheduler sets it
    @property
    def lr(self):
        return self._learning_rate

    @lr.setter
    def lr(self, v):
        self.learning_rate = v

    @property
    def has_schedule(self):
        return isinstance(self._learning_rate, schedules.LearningRateSchedule)

    def _hyper(self):
        """the constructor arguments besides learning_rate, the clip keywords and name"""
        return {}

    def get_config(self):
        lr = self._learning_rate
        if self.has_schedule:
            lr = {"class_name": type(lr).__name__, "config": lr.get_config()}
        cfg = {"name": self.name, "learning_rate": lr}
        cfg.update(self._hyper())
        cfg.update({"clipnorm": self.clipnorm, "clipvalue": self.clipvalue, "global_clipnorm": self.global_clipnorm})
        cfg.update({"use_ema": self.use_ema, "ema_momentum": self.ema_momentum, "ema_overwrite_frequency": self.ema_overwrite_frequency})
        return cfg

    @classmethod
    def from_config(cls, config):
        config = dict(config)
        lr = config.get("learning_rate")
        if isinstance(lr, dict):
            config["learning_rate"] = getattr(schedules, lr["class_name"]).from_config(lr["config"])
        return cls(**config)

    def _fill(self, o):
        """the kind's own fields of the nif_opt"""

    def finalize_variable_values(self, var_list):
        """Keras' optimizer.finalize_variable_values(model.trainable_variables): the weights become their moving average (slot 3 of
        the engine).  var_list: the model's trainable_variables (the Variable objects know their model) or the model itself.  Nothing
        happens when use_ema is false; Model.fit calls this after its last epoch."""
        if not self.use_ema:
            return
        model = var_list
        if isinstance(var_list, (list, tuple)):
            if not var_list:
                return
            model = getattr(var_list[0], "_model", None)
        e = getattr(model, "_engine", None)
        if e is None:
            raise TypeError("finalize_variable_values(var_list): model.trainable_variables or the model")
        e.set_flat(e.get_opt_slot(3))

    def as_opt(self):
        o = _lib.nif_opt()
        o.kind = self.kind
        if self.has_schedule:
            self._learning_rate.pack(o)
        else:
            o.lr = self._learning_rate
        self._fill(o)
        return o


class Adam(_KerasOptimizer):
    """Keras-2.11 Adam.  clipnorm / clipvalue / global_clipnorm are Keras' gradient clipping (per tensor by norm, by value, by the
    global norm), applied on the device in front of the update (k_gradtf.hip); at most one of them, as in Keras.  amsgrad=True keeps
    vhat = max(vhat, v) in a third slot and divides by sqrt(vhat) + epsilon.  Without amsgrad and with a constant learning rate the
    step is nif_adam_step_dev's (as_struct); otherwise it travels as a nif_opt (as_opt)."""
    _DEFAULT_NAME = "Adam"

    def __init__(self, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, clipnorm=None, clipvalue=None,
                 global_clipnorm=None, name=None, **kwargs):
        self._base(learning_rate, clipnorm, clipvalue, global_clipnorm, kwargs, name)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.amsgrad = bool(amsgrad)

    def _unknown_kwargs(self, kwargs):
        """(Adam has always let the other keyword arguments of Keras' optimizer base pass)"""

    @property
    def is_plain(self):
        """the step nif_adam_step_dev / nif_graph_launch run: no amsgrad, no schedule, no decoupled weight decay"""
        return type(self)._fill is Adam._fill and not self.amsgrad and not self.has_schedule

    def _hyper(self):
        return {"beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon, "amsgrad": self.amsgrad}

    def as_struct(self):
        if not self.is_plain:
            raise ValueError("%s.as_struct(): amsgrad, a schedule and decoupled weight decay travel as a nif_opt (as_opt)" % type(self).__name__)
        return _lib.nif_adam(self._learning_rate, self.beta_1, self.beta_2, self.epsilon)

    def _fill(self, o):
        o.beta1, o.beta2, o.eps = self.beta_1, self.beta_2, self.epsilon
        o.flags = _lib.OPT_AMSGRAD if self.amsgrad else 0


class AdamW(Adam):
    """Keras-2.11 AdamW: theta -= lr * weight_decay * theta with the step's learning rate, then Adam's update (with or without amsgrad)"""
    _DEFAULT_NAME = "AdamW"

    def __init__(self, learning_rate=0.001, weight_decay=0.004, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, clipnorm=None,
                 clipvalue=None, global_clipnorm=None, name=None, **kwargs):
        Adam.__init__(self, learning_rate, beta_1, beta_2, epsilon, amsgrad, clipnorm, clipvalue, global_clipnorm, name, **kwargs)
        if weight_decay is None:
            raise ValueError("Missing value of `weight_decay` which is required and must be a float value.")
        self.weight_decay = _number("AdamW", "weight_decay", weight_decay)

    _unknown_kwargs = _KerasOptimizer._unknown_kwargs

    def _hyper(self):
        return dict(Adam._hyper(self), weight_decay=self.weight_decay)

    def _fill(self, o):
        Adam._fill(self, o)
        o.flags |= _lib.OPT_DECOUPLED_WD
        o.weight_decay = self.weight_decay


class SGD(_KerasOptimizer):
    """Keras-2.11 SGD: theta -= lr g; with momentum m = momentum m - lr g and theta += m, nesterov: theta += momentum m - lr g"""
    kind = _lib.OPT_SGD
    _DEFAULT_NAME = "SGD"

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, amsgrad=False, clipnorm=None, clipvalue=None,
                 global_clipnorm=None, name=None, **kwargs):
        self._base(learning_rate, clipnorm, clipvalue, global_clipnorm, kwargs, name)
        self.momentum = _number("SGD", "momentum", momentum)
        if not 0.0 <= self.momentum <= 1.0:
            raise ValueError("`momentum` must be between [0, 1].")
        self.nesterov = bool(nesterov)
        if amsgrad:
            raise NotImplementedError("SGD(amsgrad=True): Keras' SGD has no such update")

    def _hyper(self):
        return {"momentum": self.momentum, "nesterov": self.nesterov}

    def _fill(self, o):
        o.beta1 = self.momentum
        o.flags = _lib.OPT_NESTEROV if self.nesterov else 0


class RMSprop(_KerasOptimizer):
    """Keras-2.11 RMSprop: v = rho v + (1-rho) g^2; centered: a = rho a + (1-rho) g and the denominator v - a^2 + epsilon, else
    v + epsilon; inc = lr g / sqrt(denominator); with momentum mom = momentum mom + inc and theta -= mom, else theta -= inc"""
    kind = _lib.OPT_RMSPROP
    _DEFAULT_NAME = "RMSprop"

    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, clipnorm=None, clipvalue=None,
                 global_clipnorm=None, name=None, **kwargs):
        self._base(learning_rate, clipnorm, clipvalue, global_clipnorm, kwargs, name)
        self.rho, self.epsilon = _number("RMSprop", "rho", rho), float(epsilon)
        self.momentum = _number("RMSprop", "momentum", momentum)
        if not 0.0 <= self.momentum <= 1.0:
            raise ValueError("`momentum` must be between [0, 1].")
        self.centered = bool(centered)

    def _hyper(self):
        return {"rho": self.rho, "momentum": self.momentum, "epsilon": self.epsilon, "centered": self.centered}

    def _fill(self, o):
        o.beta1, o.beta2, o.eps = self.momentum, self.rho, self.epsilon
        o.flags = _lib.OPT_CENTERED if self.centered else 0


class Adagrad(_KerasOptimizer):
    """Keras-2.11 Adagrad: acc += g^2 from acc = initial_accumulator_value; theta -= lr g / sqrt(acc + epsilon)"""
    kind = _lib.OPT_ADAGRAD
    _DEFAULT_NAME = "Adagrad"

    def __init__(self, learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7, clipnorm=None, clipvalue=None,
                 global_clipnorm=None, name=None, **kwargs):
        self._base(learning_rate, clipnorm, clipvalue, global_clipnorm, kwargs, name)
        self.initial_accumulator_value = _number("Adagrad", "initial_accumulator_value", initial_accumulator_value)
        if self.initial_accumulator_value < 0.0:
            raise ValueError("initial_accumulator_value must be non-negative: %r" % (initial_accumulator_value,))
        self.epsilon = float(epsilon)

    def _hyper(self):
        return {"initial_accumulator_value": self.initial_accumulator_value, "epsilon": self.epsilon}

    def _fill(self, o):
        o.eps, o.init_acc = self.epsilon, self.initial_accumulator_value


class Adamax(_KerasOptimizer):
    """Keras-2.11 Adamax: m += (g - m)(1 - beta_1); u = max(beta_2 u, |g|); theta -= (lr / (1 - beta_1^t)) m / (u + epsilon)"""
    kind = _lib.OPT_ADAMAX
    _DEFAULT_NAME = "Adamax"

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, clipvalue=None,
                 global_clipnorm=None, name=None, **kwargs):
        self._base(learning_rate, clipnorm, clipvalue, global_clipnorm, kwargs, name)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)

    def _hyper(self):
        return {"beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon}

    def _fill(self, o):
        o.beta1, o.beta2, o.eps = self.beta_1, self.beta_2, self.epsilon


class Nadam(object):
    """tf.keras.optimizers.Nadam: not built -- its momentum schedule keeps a running product as state that the optimizer step has no
    place for"""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("Nadam: not built (its running product of the momentum schedule is state the optimizer step does "
                                  "not carry); built are Adam, AdamW, SGD, RMSprop, Adagrad, Adamax, Lion and AdaBeliefOptimizer")


def ema_overwrite(t, frequency):
    """whether the step that completes iteration t (1-based) overwrites the weights by their average, for ema_overwrite_frequency
    `frequency` (None: never): every `frequency` steps, the rule of the kernels (nif_internal.h ema_overwrite)"""
    return frequency is not None and int(frequency) >= 1 and int(t) % int(frequency) == 0


def ema_of(opt):
    """None, or Engine.set_ema's (momentum, overwrite_frequency) of an optimizer compiled with use_ema"""
    if not getattr(opt, "use_ema", False):
        return None
    return float(opt.ema_momentum), opt.ema_overwrite_frequency


def slot_layout(opt):
    """(kind, slot-shaping flags, has a second slot, has a third slot) of a compiled optimizer: what a checkpoint and a captured graph
    are tied to.  Slots by index: Adam / AdaBelief m, v, vhat; Lion, SGD m; RMSprop v, mom, a; Adagrad acc; Adamax m, u"""
    if isinstance(opt, _KerasOptimizer):
        flags = opt.as_opt().flags & (_lib.OPT_AMSGRAD | _lib.OPT_CENTERED | _lib.OPT_DECOUPLED_WD)
    else:
        flags = _lib.OPT_AMSGRAD if opt.amsgrad else 0
    second = opt.kind not in (_lib.OPT_LION, _lib.OPT_SGD, _lib.OPT_ADAGRAD)
    return opt.kind, flags, second, bool(flags & (_lib.OPT_AMSGRAD | _lib.OPT_CENTERED))


def _number(cls, what, v):
    """a plain number (learning-rate / weight-decay schedule objects are not built)"""
    if isinstance(v, bool) or not isinstance(v, (numbers.Real, np.floating, np.integer)):
        raise NotImplementedError("%s(%s=%r): only numbers are built (no schedule objects)" % (cls, what, v))
    return float(v)


def _legacy_kwargs(cls, kwargs, learning_rate):
    """the keyword arguments of Keras' legacy optimizer base both reference classes accept: `lr` (wins over learning_rate, as in
    the reference's kwargs.get("lr", learning_rate)) and `decay`; clipping and anything else is not built"""
    kwargs = dict(kwargs)
    learning_rate = kwargs.pop("lr", learning_rate)
    decay = _number(cls, "decay", kwargs.pop("decay", 0.0))
    if decay < 0.0:
        raise ValueError("decay cannot be less than 0. Received: decay=%r." % (decay,))
    if kwargs:
        clip = " -- clipping reaches %s through centralized_gradients_for_optimizer: set opt.clipnorm / opt.clipvalue as " \
               "attributes and opt.get_gradients = centralized_gradients_for_optimizer(opt)" % cls if set(kwargs) & set(_CLIP_KEYS) else ""
        raise NotImplementedError("%s(%s): not built (the clip keywords and the other keyword arguments of Keras' optimizer base "
                                  "are not constructor arguments here)%s" % (cls, ", ".join(sorted(kwargs)), clip))
    return _number(cls, "learning_rate", learning_rate), decay


class _LrProperty(object):
    # Keras exposes optimizer.lr / optimizer.learning_rate; LearningRateScheduler sets it
    @property
    def lr(self):
        return self.learning_rate

    @lr.setter
    def lr(self, v):
        self.learning_rate = float(v)

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class Lion(_LrProperty):
    """nif.optimizers.Lion (reference nif/optimizers/external_optimizers.py:631-735), updated by the k_opt.hip kernels:
    theta -= lr_d (sign(b1 m + (1-b1) g) + wd theta), then m = b2 m + (1-b2) g; lr_d = lr / (1 + decay (t - 1))."""
    kind = _lib.OPT_LION
    amsgrad = False

    def __init__(self, learning_rate=1e-4, beta_1=0.9, beta_2=0.99, wd=0, name="lion", print_change_log=True, **kwargs):
        self.learning_rate, self.decay = _legacy_kwargs("Lion", kwargs, learning_rate)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.wd = _number("Lion", "wd", wd)
        self.name = name

    def get_config(self):
        return {"name": self.name, "learning_rate": self.learning_rate, "decay": self.decay, "beta_1": self.beta_1,
                "beta_2": self.beta_2, "wd": self.wd}

    def as_opt(self):
        o = _lib.nif_opt()
        o.kind = self.kind
        o.lr, o.beta1, o.beta2, o.weight_decay, o.decay = self.learning_rate, self.beta_1, self.beta_2, self.wd, self.decay
        return o


class AdaBeliefOptimizer(_LrProperty):
    """nif.optimizers.AdaBeliefOptimizer (reference nif/optimizers/external_optimizers.py:322-628), updated by the k_opt.hip kernels:
    Adam on the belief (g - m)^2, optional rectification (RAdam) behind sma_threshold, AMSGrad, weight_decay * theta added to the
    step, and a warm-up / linear decay of the learning rate over total_steps.  epsilon 0 becomes Keras' 1e-7."""
    kind = _lib.OPT_ADABELIEF

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-14, weight_decay=0.0, rectify=True, amsgrad=False,
                 sma_threshold=5.0, total_steps=0, warmup_proportion=0.1, min_lr=0.0, name="AdaBeliefOptimizer",
                 print_change_log=True, **kwargs):
        self.learning_rate, self.decay = _legacy_kwargs("AdaBeliefOptimizer", kwargs, learning_rate)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = float(epsilon or 1e-7)
        self.weight_decay = _number("AdaBeliefOptimizer", "weight_decay", weight_decay)
        self.rectify, self.amsgrad = bool(rectify), bool(amsgrad)
        self.sma_threshold = float(sma_threshold)
        self.total_steps = int(total_steps)
        self.warmup_proportion, self.min_lr = float(warmup_proportion), float(min_lr)
        self.name = name

    def get_config(self):
        return {"name": self.name, "learning_rate": self.learning_rate, "beta_1": self.beta_1, "beta_2": self.beta_2,
                "decay": self.decay, "weight_decay": self.weight_decay, "sma_threshold": self.sma_threshold,
                "epsilon": self.epsilon, "amsgrad": self.amsgrad, "rectify": self.rectify, "total_steps": self.total_steps,
                "warmup_proportion": self.warmup_proportion, "min_lr": self.min_lr}

    def as_opt(self):
        o = _lib.nif_opt()
        o.kind = self.kind
        o.flags = (_lib.OPT_RECTIFY if self.rectify else 0) | (_lib.OPT_AMSGRAD if self.amsgrad else 0)
        o.lr, o.beta1, o.beta2, o.eps = self.learning_rate, self.beta_1, self.beta_2, self.epsilon
        o.weight_decay, o.decay, o.sma_threshold = self.weight_decay, self.decay, self.sma_threshold
        o.warmup_proportion, o.min_lr, o.total_steps = self.warmup_proportion, self.min_lr, self.total_steps
        return o


class L4Adam(object):
    """nif.optimizers.L4Adam: not built -- the reference's own class cannot run (its apply step starts from new_var = None,
    external_optimizers.py:148)."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("L4Adam: the reference's implementation does not run (external_optimizers.py:148 new_var=None); "
                                  "use Adam, Lion or AdaBeliefOptimizer")


class _CentralizedGradients(object):
    """what centralized_gradients_for_optimizer returns: a marker Model.compile recognises on optimizer.get_gradients"""

    def __init__(self, optimizer):
        self.optimizer = optimizer

    def __call__(self, loss=None, params=None):
        raise NotImplementedError("centralized_gradients_for_optimizer(opt)(loss, params): there is no symbolic loss to differentiate "
                                  "here -- assign the result to opt.get_gradients and compile the model with opt; the gradient is "
                                  "centralised and clipped on the device in front of every update")


def centralized_gradients_for_optimizer(optimizer):
    """nif.optimizers.centralized_gradients_for_optimizer (reference nif/optimizers/gtcf.py:7-67; gradient centralisation, Yong et al.
    2020).  Documented use, as in the reference:

        opt = nif_amd.optimizers.Lion(1e-4)            # or Adam, AdaBeliefOptimizer
        opt.clipnorm = 1.0                              # optional attributes, read at the start of every fit()
        opt.get_gradients = centralized_gradients_for_optimizer(opt)
        model.compile(optimizer=opt, loss="mse")

    Every step's gradient then goes through what the reference function's body computes: each rank-2 gradient [in, out] loses its
    mean over the `in` axis per output column (the body's `keep_dims` is TF1's spelling of `keepdims`); if `opt.clipnorm` exists
    and is > 0 the whole gradient is scaled to that global norm where its norm is larger; if `opt.clipvalue` exists and is > 0 it
    is clamped to [-clipvalue, clipvalue] behind that.  A kernel with ONE input row (latent_dim = 1's hypernetwork matrix, a first
    layer with one input) is centralised to exactly zero and stops training, in the reference's formula as here.
    Under the reference's pinned TensorFlow 2.11 the hook is inert: Keras' fit() never calls optimizer.get_gradients, so the
    reference trains unchanged whether or not the function was used; what is built here is what its body computes.  The returned
    object cannot be called (there is no symbolic loss): it is a marker."""
    if not isinstance(optimizer, (_KerasOptimizer, Lion, AdaBeliefOptimizer)):
        raise TypeError("centralized_gradients_for_optimizer(optimizer): an Adam, Lion or AdaBeliefOptimizer of nif_amd.optimizers "
                        "(or one of its Keras kinds: AdamW, SGD, RMSprop, Adagrad, Adamax)")
    return _CentralizedGradients(optimizer)


def grad_transform_of(opt):
    """the gradient transform an optimizer asks for, as Engine.set_grad_transform's dict, or None: the gtcf route when
    opt.get_gradients carries centralized_gradients_for_optimizer's marker (clipnorm / clipvalue read as gtcf.py:42,47 does:
    hasattr(...) and > 0), else Keras' route from Adam's clip keywords"""
    def positive(name):
        v = getattr(opt, name, None)
        return float(v) if v is not None and float(v) > 0.0 else 0.0
    if isinstance(getattr(opt, "get_gradients", None), _CentralizedGradients):
        if getattr(opt, "global_clipnorm", None):
            raise ValueError("centralized_gradients_for_optimizer reads clipnorm (its global norm) and clipvalue; global_clipnorm=%r "
                             "is set as well" % (opt.global_clipnorm,))
        return {"centralize": True, "gtcf": True, "clipnorm": positive("clipnorm"), "clipvalue": positive("clipvalue")}
    if not isinstance(opt, _KerasOptimizer):
        return None       # (Lion / AdaBeliefOptimizer take no clip keywords: attributes count on the gtcf route only)
    spec = {k: positive(k) for k in _CLIP_KEYS}
    if sum(1 for v in spec.values() if v) > 1:
        raise ValueError("At most one of `clipnorm`, `clipvalue` and `global_clipnorm` can be set.")
    return spec if any(spec.values()) else None


_BY_NAME = {"adam": Adam, "adamw": AdamW, "sgd": SGD, "rmsprop": RMSprop, "adagrad": Adagrad, "adamax": Adamax}


def get(opt):
    if isinstance(opt, (_KerasOptimizer, Lion, AdaBeliefOptimizer)):
        return opt
    if isinstance(opt, str):
        if opt.lower() in _BY_NAME:
            return _BY_NAME[opt.lower()]()
        if opt.lower() == "nadam":
            return Nadam()
        raise NotImplementedError("optimizer %r: Keras' names built here are %s (Lion and AdaBeliefOptimizer are passed as objects)"
                                  % (opt, ", ".join(sorted(_BY_NAME))))
    # duck-typed: anything with learning_rate/beta_1/beta_2/epsilon (e.g. a config object)
    if all(hasattr(opt, a) for a in ("learning_rate", "beta_1", "beta_2", "epsilon")):
        return Adam(float(opt.learning_rate), float(opt.beta_1), float(opt.beta_2), float(opt.epsilon))
    raise NotImplementedError("optimizer %r: an Adam, AdamW, SGD, RMSprop, Adagrad, Adamax, Lion or AdaBeliefOptimizer of "
                              "nif_amd.optimizers, or one of Keras' names for them" % (opt,))


import numpy as np


class LBFGSMinimizer(object):
    """Host side of one `tfp.optimizer.lbfgs_minimize` call on a closure fun(x) -> (loss, gradient) (float64 NumPy):
    two-loop recursion over up to 20 correction pairs and a Hager-Zhang line search with approximate Wolfe
    conditions.  No device code: the closure is where the HIP kernels run."""
    NUM_CORRECTION_PAIRS = 20          # lbfgs.py:111
    MAX_LINE_SEARCH_ITERATIONS = 100   # lbfgs.py:117
    TOLERANCE = 1e-15                  # lbfgs.py:112-114 (gradient sup-norm, x and relative f tolerances)

    def __init__(self, fun):
        self.fun = fun

    # ---- Hager-Zhang line search along d from x: phi(a) = f(x + a d) -------------------------------------------
    def _line_search(self, x, d, f0, g0):
        delta, sigma, eps, theta, gamma, rho = 0.1, 0.9, 1e-6, 0.5, 0.66, 5.0
        dphi0 = float(g0.dot(d))
        flimit = f0 + eps * abs(f0)
        budget = [self.MAX_LINE_SEARCH_ITERATIONS]

        def phi(a):
            budget[0] -= 1
            fv, gv = self.fun(x + a * d)
            return {"a": a, "f": fv, "df": float(gv.dot(d)), "g": gv}

        def ok(p):   # Wolfe, or the approximate Wolfe conditions near the minimum
            if not np.isfinite(p["f"]):
                return False
            wolfe = p["f"] <= f0 + delta * p["a"] * dphi0 and p["df"] >= sigma * dphi0
            approx = p["f"] <= flimit and (2 * delta - 1) * dphi0 >= p["df"] >= sigma * dphi0
            return wolfe or approx

        p0 = {"a": 0.0, "f": f0, "df": dphi0, "g": g0}
        c = phi(1.0)
        while not np.isfinite(c["f"]) and budget[0] > 0:       # step into a non-finite region: shrink
            c = phi(c["a"] * 0.1)
        if ok(c):
            return c
        # bracket [lo, hi]: dphi(lo) < 0, phi(lo) <= flimit, dphi(hi) >= 0
        lo, hi = p0, None
        while budget[0] > 0:
            if c["df"] >= 0:
                hi = c
                break
            if c["f"] > flimit:            # went uphill with a negative slope: the minimum is in (lo, c): bisect
                a_, b_ = lo, c
                while budget[0] > 0:
                    m = phi((1 - theta) * a_["a"] + theta * b_["a"])
                    if ok(m):
                        return m
                    if m["df"] >= 0:
                        lo, hi = a_, m
                        break
                    if m["f"] <= flimit:
                        a_ = m
                    else:
                        b_ = m
                break
            lo = c
            c = phi(rho * c["a"])
            if ok(c):
                return c
        if hi is None:
            return c if np.isfinite(c["f"]) and c["f"] < f0 else None

        def update(a_, b_, m):       # HZ "update": keep a bracket with the sign conditions
            if not (a_["a"] < m["a"] < b_["a"]):
                return a_, b_
            if m["df"] >= 0:
                return a_, m
            if m["f"] <= flimit:
                return m, b_
            aa, bb = a_, m
            while budget[0] > 0:
                t = phi((1 - theta) * aa["a"] + theta * bb["a"])
                if t["df"] >= 0:
                    return aa, t
                if t["f"] <= flimit:
                    aa = t
                else:
                    bb = t
            return aa, bb

        def secant(a_, b_):
            den = b_["df"] - a_["df"]
            return (a_["a"] * b_["df"] - b_["a"] * a_["df"]) / den if den != 0 else 0.5 * (a_["a"] + b_["a"])

        while budget[0] > 0:
            width = hi["a"] - lo["a"]
            cs = secant(lo, hi)
            m = phi(cs) if lo["a"] < cs < hi["a"] else None
            if m is not None and ok(m):
                return m
            A, Bk = update(lo, hi, m) if m is not None else (lo, hi)
            if m is not None and budget[0] > 0:      # secant^2: a second secant step from the side that moved
                c2 = None
                if m is Bk:
                    c2 = secant(hi, Bk)
                elif m is A:
                    c2 = secant(lo, A)
                if c2 is not None and A["a"] < c2 < Bk["a"]:
                    m2 = phi(c2)
                    if ok(m2):
                        return m2
                    A, Bk = update(A, Bk, m2)
            if Bk["a"] - A["a"] > gamma * width and budget[0] > 0:
                m3 = phi(0.5 * (A["a"] + Bk["a"]))
                if ok(m3):
                    return m3
                A, Bk = update(A, Bk, m3)
            lo, hi = A, Bk
            if hi["a"] - lo["a"] <= 1e-16 * max(1.0, hi["a"]):
                break
        best = lo if lo["a"] > 0 and lo["f"] < f0 else None
        return best

    def run(self, x, max_iter):
        """one tfp.optimizer.lbfgs_minimize call: fresh memory, up to max_iter iterations"""
        x, f, _, _ = self.run_resumable(x, max_iter, None)
        return x, f

    def run_resumable(self, x, max_iter, state):
        """up to max_iter more iterations of a run whose correction pairs / last evaluation are carried in `state`
        (lbfgs_minimize(previous_optimizer_results=...)) -> (x, f, state, iterations done)"""
        if state is None:
            f, g = self.fun(x)
            S, Y = [], []
        else:
            f, g, S, Y = state
        done = 0
        for _ in range(max_iter):
            if np.abs(g).max() <= self.TOLERANCE:
                break
            q = g.copy()
            alphas = []
            for s_, y_ in zip(reversed(S), reversed(Y)):
                a = s_.dot(q) / y_.dot(s_)
                alphas.append(a)
                q -= a * y_
            if S:
                q *= S[-1].dot(Y[-1]) / Y[-1].dot(Y[-1])
            for (s_, y_), a in zip(zip(S, Y), reversed(alphas)):
                b = y_.dot(q) / y_.dot(s_)
                q += (a - b) * s_
            d = -q
            if g.dot(d) >= 0:        # not a descent direction (lost curvature): steepest descent, memory dropped
                S, Y, d = [], [], -g
            p = self._line_search(x, d, f, g)
            if p is None:
                break
            s_, y_ = p["a"] * d, p["g"] - g
            fprev = f
            x, f, g = x + s_, p["f"], p["g"]
            done += 1
            if s_.dot(y_) > 0:
                S.append(s_); Y.append(y_)
                if len(S) > self.NUM_CORRECTION_PAIRS:
                    S.pop(0); Y.pop(0)
            if np.abs(s_).max() <= self.TOLERANCE or abs(fprev - f) <= self.TOLERANCE * abs(fprev):
                break
        return x, f, (f, g, S, Y), done


class TFPLBFGS(object):
    """Second-stage fine-tuner of the reference (nif/optimizers/lbfgs.py:98-126, README.md:51-69):
    `TFPLBFGS(model, loss_fun, inps, outs, display_epoch).minimize(rounds, max_iter)` runs full-batch L-BFGS on the
    flat parameter vector.  As in the reference, every round is a FRESH `lbfgs_minimize` started from the model's
    current variables (correction pairs are dropped between rounds, lbfgs.py:106-118) with 20 correction pairs, up to
    `max_iter` iterations and up to 100 line-search evaluations each, and `history` lists the loss of EVERY closure
    evaluation (lbfgs.py:80-88, :123-126).  The loss+gradient closure (lbfgs.py:66-74) is the HIP training-step kernels
    on a dataset made resident in HBM once (`nif_loss_grad_dev` + `nif_grad_read`: per evaluation only the P parameters
    go up and P+1 floats come back).  The two-loop recursion and the Hager-Zhang line search (what
    tfp.optimizer.lbfgs_minimize uses; restated from the published algorithm, CG_DESCENT, Hager & Zhang 2005/2006:
    approximate Wolfe conditions, bracketing by expansion, secant^2 + bisection updates) run on the host in float64.

    dtype="float64" (the reference's newer fine-tuner switches Keras to float64, lbfgs_V2.py:79) is a precision of the FINE-TUNER,
    not Keras' float64 policy: the model stays a float32 model; the closure evaluates loss and gradient in double on the device
    (nif_f64_*, k_f64.hip) at a float64 master vector that starts as the exact upcast of the model's parameters, receives every
    trial point unrounded, survives between rounds (`position`), and is rounded into the model's float32 parameters after every
    round.  Inputs, targets and sample weights travel as float64.  Built for class NIF and NIFMultiScale under policy float32."""

    _F64_BUILT = "dtype='float64' is built for class NIF and NIFMultiScale under mixed_policy='float32'"

    def __init__(self, model, loss_fun, inps, outs, display_epoch=1, sample_weight=None, dtype="float32"):
        import numpy as np
        self._np = np
        if dtype not in ("float32", "float64"):
            raise ValueError("TFPLBFGS / MSEClosure: dtype is 'float32' or 'float64', got %r" % (dtype,))
        self.dtype = dtype
        if getattr(model, "_is_pruned", False):
            raise NotImplementedError("TFPLBFGS / LBFGSOptimizer on a pruned model (nif_amd.sparsity): strip_pruning(model) first")
        if getattr(model, "_order", 1) == 2:
            raise NotImplementedError("TFPLBFGS / LBFGSOptimizer on the three-output Sobolev model (HessianLayer) is not built: its "
                                      "loss has a second-derivative term the L-BFGS closure does not fit; train it with fit()")
        name = loss_fun if isinstance(loss_fun, str) else getattr(loss_fun, "name", None) or getattr(loss_fun, "__name__", None)
        if not isinstance(loss_fun, str) and loss_fun is not None:      # loss OBJECTS: only their defaults are built (as Model.compile)
            if float(getattr(loss_fun, "delta", 1.0)) != 1.0:
                raise NotImplementedError("TFPLBFGS: huber with delta != 1")
            red = getattr(loss_fun, "reduction", None)
            if red is not None and str(red).lower().rsplit(".", 1)[-1] not in ("auto", "sum_over_batch_size"):
                raise NotImplementedError("TFPLBFGS: loss reduction %r (built: the default SUM_OVER_BATCH_SIZE)" % (red,))
        from . import _lib
        if name is not None and name not in _lib.LOSS_IDS:
            raise NotImplementedError("TFPLBFGS: built losses are 'mse', 'mae', 'huber', 'log_cosh', got %r" % (loss_fun,))
        self._loss = "mse" if name is None else ("mse", "mae", "huber", "log_cosh")[_lib.LOSS_IDS[name]]
        self.model = model
        e = model._engine
        if dtype == "float64":
            self._init_f64(e, inps, outs, sample_weight, display_epoch)
            return
        x = e._inputs(inps)
        self._B = x.shape[0]
        y = e._targets(outs, self._B)
        sw = e._weights(sample_weight, self._B)
        self._d_x, self._d_y = e.alloc(x.size), e.alloc(y.size)
        self._d_x.upload(x); self._d_y.upload(y)
        self._d_sw = None
        if sw is not None:
            self._d_sw = e.alloc(sw.size); self._d_sw.upload(sw)
        e.reserve(self._B, 0)
        self.display_epoch = max(int(display_epoch), 1)
        self._losses = []

    def _init_f64(self, e, inps, outs, sample_weight, display_epoch):
        np = self._np
        model = self.model
        if hasattr(model, "_order"):
            raise NotImplementedError("TFPLBFGS / MSEClosure(dtype='float64') on a Sobolev model is not built (%s)" % self._F64_BUILT)
        if e.spec.kind == "NIFMultiScaleLastLayerParameterized":
            raise NotImplementedError("TFPLBFGS / MSEClosure(dtype='float64') on NIFMultiScaleLastLayerParameterized is not built (%s)"
                                      % self._F64_BUILT)
        if e.spec.mixed_policy != "float32":
            raise NotImplementedError("TFPLBFGS / MSEClosure(dtype='float64') on a model built under mixed_policy=%r is not built (%s)"
                                      % (e.spec.mixed_policy, self._F64_BUILT))
        ncol, so = e.spec.pi_dim + e.spec.si_dim, e.spec.so_dim
        x = np.asarray(inps, dtype=np.float64)            # float64 arrays of the caller are NOT rounded to float32
        if x.ndim != 2 or x.shape[1] < ncol:
            raise ValueError("inputs: expected shape (batch, %d), got %s" % (ncol, x.shape))
        x = np.ascontiguousarray(x[:, :ncol])
        self._B = x.shape[0]
        y = np.asarray(outs, dtype=np.float64)
        if y.ndim == 1:
            y = y[:, None]
        if y.shape != (self._B, so):
            raise ValueError("targets: expected shape (%d, %d), got %s" % (self._B, so, y.shape))
        y = np.ascontiguousarray(y)
        self._d_x, self._d_y = e.alloc_f64(x.size), e.alloc_f64(y.size)
        self._d_x.upload(x); self._d_y.upload(y)
        self._d_sw = None
        if sample_weight is not None:
            sw = np.ascontiguousarray(sample_weight, dtype=np.float64).reshape(-1)
            if sw.shape != (self._B,):
                raise ValueError("sample_weight: expected shape (%d,), got %s" % (self._B, sw.shape))
            self._d_sw = e.alloc_f64(sw.size); self._d_sw.upload(sw)
        self._master = e.get_flat().astype(np.float64)    # the exact upcast of the model's float32 parameters
        e.f64_set_flat(self._master)
        self.display_epoch = max(int(display_epoch), 1)
        self._losses = []

    @property
    def position(self):
        """the fine-tuner's parameter vector: dtype='float64' the float64 master vector (kept between rounds and minimize() calls),
        else the model's float32 parameters"""
        if self.dtype == "float64":
            return self._master.copy()
        return self.model._engine.get_flat()

    def _commit(self, x):
        """lbfgs.py:120 / lbfgs_V2.py:112 assign the result: dtype='float64' keeps x as the master vector and gives the model its
        rounding, so that predict, save_weights and a later fit see the fine-tuned model"""
        np = self._np
        e = self.model._engine
        if self.dtype == "float64":
            self._master = np.array(x, dtype=np.float64)
            e.f64_set_flat(self._master)
        e.set_flat(x.astype(np.float32))

    def _start(self):
        np = self._np
        return self._master.copy() if self.dtype == "float64" else self.model._engine.get_flat().astype(np.float64)

    def _f64(self, theta):
        """the closure in double: theta goes up unrounded, loss and gradient come back as float64"""
        np = self._np
        e = self.model._engine
        e.f64_set_flat(np.ascontiguousarray(theta, dtype=np.float64))
        if hasattr(e, "set_loss"):
            e.set_loss(self._loss)            # (the double path has no regulariser term to switch off: the loss kind alone)
        try:
            e.f64_loss_grad_dev(self._d_x.at(0), self._d_y.at(0), self._d_sw.at(0) if self._d_sw is not None else None, self._B, self._B)
            loss, g = e.f64_grad_read()
        finally:
            if hasattr(e, "set_loss"):
                e.set_loss("mse")
        self._losses.append(loss)
        if len(self._losses) % self.display_epoch == 0:
            print("Epoch: %d loss: %.8e" % (len(self._losses), loss))
        return float(loss), g

    @property
    def history(self):
        """lbfgs.py:123-126"""
        return {"iteration": self._np.arange(1, len(self._losses) + 1), "loss": list(self._losses)}

    def _f(self, theta):
        """lbfgs.py:56-88: assign the parameters, loss and flat gradient; every call is counted and recorded"""
        if getattr(self, "dtype", "float32") == "float64":
            return self._f64(theta)
        np = self._np
        e = self.model._engine
        e.set_flat(theta.astype(np.float32))
        # the reference's closure is `loss(model(x), y)` -- the loss FUNCTION alone, model.losses is never added (lbfgs.py:66-68,
        # lbfgs_V2.py:63-66): no weight / activity / latent-Jacobian regulariser in the L-BFGS objective, whatever the last
        # fit() of a model sharing this engine left configured
        with self.model._plain_loss(e, **({} if getattr(self, "_loss", "mse") == "mse" else {"loss": self._loss})):
            e.loss_grad_dev(self._d_x.at(0), self._d_y.at(0), self._d_sw.at(0) if self._d_sw is not None else None, self._B, self._B)
            loss, g = e.grad_read()
        self._losses.append(loss)
        if len(self._losses) % self.display_epoch == 0:
            print("Epoch: %d loss: %.8e" % (len(self._losses), loss))
        return float(loss), g.astype(np.float64)

    def minimize(self, rounds=50, max_iter=50):
        """lbfgs.py:103-121: `rounds` independent lbfgs_minimize calls, each from the model's current variables"""
        for _ in range(rounds):
            x, _f = LBFGSMinimizer(self._f).run(self._start(), max_iter)
            self._commit(x)                       # lbfgs.py:120 assign_new_model_parameters(results.position)
        return self.history


class MSEClosure(object):
    """What `LBFGSOptimizer` takes where the reference takes a Python function evaluated under a GradientTape
    (lbfgs_V2.py:77-85: `loss_closure` = "the model's loss on the training table"): the model, its full-batch table and
    optional sample weights -- resident in HBM once; calling it returns the current loss like the reference's closure does."""

    def __init__(self, model, x, y, sample_weight=None, dtype="float32"):
        self._t = TFPLBFGS(model, "mse", x, y, display_epoch=1 << 62, sample_weight=sample_weight, dtype=dtype)
        self.model = model
        self.dtype = dtype

    def __call__(self):
        return self._t._f(self._t._start())[0]


class LBFGSOptimizer(object):
    """nif/optimizers/lbfgs_V2.py:77-112: `opt = LBFGSOptimizer(loss_closure, trainable_variables, steps)`; every
    `opt.minimize()` continues the SAME L-BFGS run for `steps` more iterations (previous_optimizer_results: the correction
    pairs survive between calls, unlike TFPLBFGS); `.epoch` = iterations so far, `.loss` = the objective there.
    `loss_closure` is an `MSEClosure`; `trainable_variables` is accepted for signature parity (it is always the model's
    full variable list, which is what the reference passes)."""

    def __init__(self, loss_closure, trainable_variables=None, steps=1):
        if not isinstance(loss_closure, MSEClosure):
            raise TypeError("LBFGSOptimizer(loss_closure=nif_amd.optimizers.MSEClosure(model, x, y), ...): a Python loss function "
                            "cannot be differentiated here -- the closure names the model and its table, the HIP kernels do the rest")
        if getattr(loss_closure.model, "_is_pruned", False):
            raise NotImplementedError("TFPLBFGS / LBFGSOptimizer on a pruned model (nif_amd.sparsity): strip_pruning(model) first")
        self._c = loss_closure
        self.steps = int(steps)
        self._it = 0
        self._loss = None
        self._state = None

    @property
    def epoch(self):
        return self._it

    @property
    def loss(self):
        return self._loss

    def minimize(self):
        t = self._c._t
        mz = LBFGSMinimizer(t._f)
        x, f, self._state, done = mz.run_resumable(t._start(), self.steps, self._state)
        self._it += done
        self._loss = float(f)
        t._commit(x)                               # lbfgs_V2.py:112 assign(results.position)

    @property
    def position(self):
        """the closure's parameter vector: a MSEClosure(dtype='float64') keeps its float64 master vector between minimize() calls"""
        return self._c._t.position
