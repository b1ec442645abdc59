"""Low-magnitude pruning of NIF models: the `tfmot.sparsity.keras` surface (TensorFlow Model Optimization 0.7.3, the reference's
pinned version) for the models NIF / NIFMultiScale / NIFMultiScaleLastLayerParameterized build.

    pruned = nif_amd.sparsity.prune_low_magnitude(model, pruning_schedule=PolynomialDecay(0.0, 0.8, 0, 1000))
    pruned.compile(optimizer, loss)
    pruned.fit(x, y, callbacks=[nif_amd.sparsity.UpdatePruningStep()])
    plain = nif_amd.sparsity.strip_pruning(pruned)

Which tensors are pruned is what the reference's layers return from `get_prunable_weights`, plus `kernel` of a plain Keras Dense
(TF-MOT's registry):
  * SIREN (first / hidden / bottleneck)  nif/layers/siren.py:298-304   [w]
  * SIREN_ResNet                         nif/layers/siren.py:412-420   [w, w2]
  * HyperLinearForSIREN                  nif/layers/siren.py:536-538   [w]   (the bias is not pruned)
  * MLP_ResNet                           nif/layers/mlp.py:92-99       L1.weights + L2.weights = [w, b, w2, b2]
  * MLP_SimpleShortCut                   nif/layers/mlp.py:183-190     L1.weights = [w, b]
and the ParameterNet / ShapeNet each class builds from them (nif/model.py:176-231 NIF: Dense, MLP_SimpleShortCut, Dense, Dense;
:591-663 NIFMultiScale with a sine ParameterNet: SIREN, SIREN / SIREN_ResNet, SIREN, HyperLinearForSIREN; :665-734 other activations:
Dense, MLP_SimpleShortCut / MLP_ResNet, Dense, HyperLinearForSIREN; :1147-1218 the last-layer class's ShapeNet: SIREN, SIREN /
SIREN_ResNet, SIREN bottleneck -- last_layer_bias is a bare variable and is not pruned).  `prunable_weights(model)` lists the names.

The masks are chosen on the device (k_prune.hip): a radix select finds each tensor's exact k-th largest magnitude with integer counts,
so the weights never leave the GPU and the ranks of a data-parallel run choose the same masks from the same weights.

TF-MOT itself is not a dependency; the rules below restate its pruning_schedule.py, pruning_impl.py, pruning_wrapper.py and
pruning_callbacks.py:
  * schedule at step s: should_prune = s >= begin and (end < 0 or s <= end) and (s - begin) % frequency == 0;
    PolynomialDecay p = clip((s - begin) / (end - begin), 0, 1), sparsity = (initial - final) (1 - p)^power + final, in float32
    (the difference initial - final is a Python float, as TF-MOT forms it, rounded once to float32); ConstantSparsity: target.
    float32 `pow` is NumPy's here, TensorFlow's there: the two are not confirmed to agree to the last bit for every argument.
  * on a pruning turn each tensor keeps k = max(round_half_even(float32(size) * (1 - float32(sparsity))), 1) entries:
    threshold = the k-th largest |w|, mask = |w| >= threshold (ties keep more than k);
  * order within a training batch: the step number is set by UpdatePruningStep, the masks are updated from the current weights if
    the schedule says so, w *= mask, then the batch's forward / gradient / all-reduce / optimizer update (dense: pruned entries and
    their optimizer slots move, and are zeroed again before the next forward);
  * predict / evaluate / __call__ (fit's validation included) apply the masks first, as the wrapper's weight_mask_op runs on every
    call; UpdatePruningStep.on_epoch_end applies them at its own place in the callback list."""
import numpy as np

from .model import Model, SobolevModel
from .callbacks import Callback

__all__ = ["PolynomialDecay", "ConstantSparsity", "prune_low_magnitude", "UpdatePruningStep", "strip_pruning", "prunable_weights"]

_CALLBACK_ERROR = ("Prune() wrapper requires the UpdatePruningStep callback to be provided during training. Please add it as a "
                   "callback to your model.fit call.")


def _check_sparsity(v, name):
    if not 0.0 <= v < 1.0:
        raise ValueError("%s must be in range [0,1), got %r" % (name, v))


def _check_steps(begin_step, end_step, frequency, allow_negative_1):
    if begin_step < 0:
        raise ValueError("begin_step should be >= 0")
    if not allow_negative_1 and end_step == -1:
        raise ValueError("end_step cannot be -1.")
    if end_step != -1:
        if end_step < 0:
            raise ValueError("end_step can be -1 or >= 0")
        if end_step < begin_step:
            raise ValueError("begin_step should be <= end_step if end_step != -1")
    if frequency <= 0:
        raise ValueError("frequency should be > 0")


class PruningSchedule(object):
    """`schedule(step)` -> (should_prune, float32 sparsity), as tfmot.sparsity.keras.PruningSchedule.__call__"""

    def should_prune(self, step):
        s, b, e = int(step), self.begin_step, self.end_step
        return s >= b and (e < 0 or s <= e) and (s - b) % self.frequency == 0

    def __call__(self, step):
        return self.should_prune(step), self.sparsity(step)


class PolynomialDecay(PruningSchedule):
    def __init__(self, initial_sparsity, final_sparsity, begin_step, end_step, power=3, frequency=100):
        self.initial_sparsity, self.final_sparsity = initial_sparsity, final_sparsity
        self.begin_step, self.end_step, self.power, self.frequency = int(begin_step), int(end_step), power, int(frequency)
        _check_steps(self.begin_step, self.end_step, self.frequency, allow_negative_1=False)
        _check_sparsity(initial_sparsity, "initial_sparsity")
        _check_sparsity(final_sparsity, "final_sparsity")

    def sparsity(self, step):
        f32 = np.float32
        span = self.end_step - self.begin_step
        if span == 0:      # (TF-MOT divides 0 by 0 at begin_step; here the decay is complete from begin_step on)
            p = f32(1.0) if int(step) >= self.begin_step else f32(0.0)
        else:
            p = np.minimum(f32(1.0), np.maximum(f32(0.0), f32(int(step) - self.begin_step) / f32(span)))
        return f32(f32(self.initial_sparsity - self.final_sparsity) * np.power(f32(1.0) - p, f32(self.power)) + f32(self.final_sparsity))

    def get_config(self):
        return {"class_name": "PolynomialDecay", "config": {"initial_sparsity": self.initial_sparsity,
                "final_sparsity": self.final_sparsity, "power": self.power, "begin_step": self.begin_step,
                "end_step": self.end_step, "frequency": self.frequency}}


class ConstantSparsity(PruningSchedule):
    def __init__(self, target_sparsity, begin_step, end_step=-1, frequency=100):
        self.target_sparsity = target_sparsity
        self.begin_step, self.end_step, self.frequency = int(begin_step), int(end_step), int(frequency)
        _check_steps(self.begin_step, self.end_step, self.frequency, allow_negative_1=True)
        _check_sparsity(target_sparsity, "target_sparsity")

    def sparsity(self, step):
        return np.float32(self.target_sparsity)

    def get_config(self):
        return {"class_name": "ConstantSparsity", "config": {"target_sparsity": self.target_sparsity,
                "begin_step": self.begin_step, "end_step": self.end_step, "frequency": self.frequency}}


def keep_count(size, sparsity):
    """entries a tensor of `size` keeps at `sparsity` (pruning_impl.py: round half to even of a float32 product, at least one)"""
    one = np.float32(1.0)
    return max(int(np.rint(np.float32(size) * (one - np.float32(sparsity)))), 1)


def _prunable_names(spec):
    """the reference layers' get_prunable_weights in Spec.param_shapes names (module docstring for the citations)"""
    names = ["pnet_first_w"]
    for i in range(spec.l_st):
        if spec.p_siren:                                    # SIREN / SIREN_ResNet: [w] / [w, w2]
            names += ["pnet_h%d_w" % i] + (["pnet_h%d_w2" % i] if spec.p_resblock else [])
        else:                                               # MLP_SimpleShortCut: [w, b]; MLP_ResNet: [w, b, w2, b2]
            names += ["pnet_h%d_w" % i, "pnet_h%d_b" % i] + (["pnet_h%d_w2" % i, "pnet_h%d_b2" % i] if spec.p_resblock else [])
    names += ["pnet_bottleneck_w", "pnet_last_w"]           # Dense kernel / SIREN w; Dense kernel / HyperLinearForSIREN w
    if spec.kind == "NIFMultiScaleLastLayerParameterized":
        names += ["snet_first_w"]
        for i in range(spec.l_sx):
            names += ["snet_h%d_w" % i] + (["snet_h%d_w2" % i] if spec.s_resblock else [])
        names += ["snet_bottleneck_w"]
    return names


def _segments(spec):
    """(name, float offset, size) of every pruned tensor, in the flat parameter order"""
    keep = set(_prunable_names(spec))
    out, off = [], 0
    for nm, s in spec.param_shapes():
        n = int(np.prod(s))
        if nm in keep:
            out.append((nm, off, n))
        off += n
    return out


def prunable_weights(model):
    """names (Spec.param_shapes / trainable_variables names) of the tensors prune_low_magnitude prunes for this model"""
    return _prunable_names(model._owner._spec)


class PrunedModel(Model):
    """What prune_low_magnitude returns: a Model over the same variables whose training and inference run TF-MOT's pruning wrapper
    steps (module docstring).  `pruning_step` is the wrappers' shared step variable (-1 until the first fit with UpdatePruningStep)."""
    _is_pruned = True

    def __init__(self, base, schedule):
        Model.__init__(self, base._owner, "full", n_inputs=base._n_inputs)
        self._po_l1 = base._po_l1
        self.pruning_schedule = schedule
        self.pruning_step = -1
        self._segs = _segments(self._owner._spec)
        self._configured = None       # the engine the segments were registered with

    @property
    def _engine(self):
        e = self._owner._engine
        if self._configured is not e:
            e.prune_config([o for _, o, _ in self._segs], [n for _, _, n in self._segs])
            self._configured = e
        return e

    def _keep_counts(self, sparsity):
        return [keep_count(n, sparsity) for _, _, n in self._segs]

    def _apply_masks(self):
        self._engine.prune_apply()

    # ---- training: Model.fit's per-batch hook --------------------------------------------------------------------------------
    def _batch_hook(self, e, callbacks):
        cbs = [cb for cb in callbacks if isinstance(cb, UpdatePruningStep)]
        if not cbs and self.pruning_step < 0:
            raise ValueError(_CALLBACK_ERROR)
        e = self._engine

        def run():
            for cb in cbs:
                cb.on_train_batch_begin(None)
            sched = self.pruning_schedule
            if sched.should_prune(self.pruning_step):
                e.prune_update(self._keep_counts(sched.sparsity(self.pruning_step)))
            e.prune_apply()
        return run

    # ---- inference: the masks first --------------------------------------------------------------------------------------------
    def _run(self, x):
        self._apply_masks()
        return Model._run(self, x)

    def evaluate(self, x, y, sample_weight=None, verbose=0, **kwargs):
        self._apply_masks()
        return Model.evaluate(self, x, y, sample_weight=sample_weight, verbose=verbose, **kwargs)

    # ---- checkpoints: + masks (float32 0 / 1, one array per pruned tensor), thresholds, pruning_step -------------------------
    def _extra_arrays(self):
        masks, thr = self._engine.get_prune_state()
        out = {"prune_mask_%s" % nm: mk for (nm, _, _), mk in zip(self._segs, masks)}
        out["prune_thresholds"] = np.asarray(thr, dtype=np.float32)
        out["pruning_step"] = np.int64(self.pruning_step)
        return out

    def _load_extra(self, d):
        if "pruning_step" not in d:
            return
        self._engine.set_prune_state([d["prune_mask_%s" % nm] for nm, _, _ in self._segs], d["prune_thresholds"])
        self.pruning_step = int(d["pruning_step"])


def prune_low_magnitude(to_prune, pruning_schedule=None, block_size=(1, 1), block_pooling_type="AVG", pruning_policy=None,
                        sparsity_m_by_n=None, **kwargs):
    """tfmot.sparsity.keras.prune_low_magnitude for the model NIF(...).build() / .model() returns: a new, uncompiled model over the
    same engine and weights (compile it before fit, as with TF-MOT).  Default schedule: ConstantSparsity(0.5, 0)."""
    if tuple(block_size) != (1, 1):
        raise NotImplementedError("prune_low_magnitude(block_size=%r): only unstructured (1, 1) pruning is built" % (block_size,))
    if block_pooling_type != "AVG":
        raise NotImplementedError("prune_low_magnitude(block_pooling_type=%r): only unstructured pruning is built" % (block_pooling_type,))
    if pruning_policy is not None:
        raise NotImplementedError("prune_low_magnitude(pruning_policy=...): not built")
    if sparsity_m_by_n is not None:
        raise NotImplementedError("prune_low_magnitude(sparsity_m_by_n=...): not built")
    if kwargs:
        raise NotImplementedError("prune_low_magnitude(%s): not built" % ", ".join(sorted(kwargs)))
    if isinstance(to_prune, PrunedModel):
        raise ValueError("prune_low_magnitude: the model is already pruned")
    if isinstance(to_prune, SobolevModel):
        raise NotImplementedError("prune_low_magnitude: the Sobolev models (SobolevModel over a JacobianLayer, two outputs, or a "
                                  "HessianLayer, three outputs) are not built")
    if not isinstance(to_prune, Model) or to_prune._role != "full":
        raise NotImplementedError("prune_low_magnitude: the model NIF(...).build() / .model() returns (not the sub-models)")
    if to_prune._jac_reg:
        raise NotImplementedError("prune_low_magnitude: a model with cfg_parameter_net['jac_reg'] is not built")
    schedule = ConstantSparsity(0.5, 0) if pruning_schedule is None else pruning_schedule
    if not isinstance(schedule, PruningSchedule):
        raise NotImplementedError("pruning_schedule: PolynomialDecay or ConstantSparsity")
    owner = to_prune._owner
    if getattr(owner, "_pruned_model", None) is not None:
        raise ValueError("these weights are already pruned by another prune_low_magnitude model: strip_pruning it first")
    pm = PrunedModel(to_prune, schedule)
    owner._pruned_model = pm
    return pm


def strip_pruning(model):
    """tfmot.sparsity.keras.strip_pruning: a plain Model over the current weights, the masks applied, pruning off"""
    if not isinstance(model, PrunedModel):
        return model
    owner = model._owner
    if getattr(owner, "_pruned_model", None) is model:
        if model._configured is not None:
            e = model._engine
            e.prune_apply()
            e.prune_config([], [])
        owner._pruned_model = None
    plain = Model(owner, "full", n_inputs=model._n_inputs)
    plain._po_l1 = model._po_l1
    return plain


class UpdatePruningStep(Callback):
    """tfmot.sparsity.keras.UpdatePruningStep: starts the step at 0 on a new model, sets it before every batch (Model.fit calls
    on_train_batch_begin through the pruned model's batch hook, batches without rows on this rank included), and applies the masks
    at the end of every epoch"""

    def __init__(self):
        Callback.__init__(self)
        self.step = 0

    def _pruned(self):
        return self.model if isinstance(self.model, PrunedModel) else None

    def on_train_begin(self, logs=None):
        m = self._pruned()
        if m is None:
            return
        if m.pruning_step == -1:
            m.pruning_step = 0
        self.step = m.pruning_step

    def on_train_batch_begin(self, batch, logs=None):
        m = self._pruned()
        if m is None:
            return
        m.pruning_step = self.step
        self.step = self.step + 1

    def on_epoch_end(self, epoch, logs=None):
        m = self._pruned()
        if m is not None:
            m._apply_masks()
