"""Drop-in Python surface of reference nif/model.py for the point-wise training path:
NIF / NIFMultiScale / NIFMultiScaleLastLayerParameterized with build/model/compile/fit/predict and
the sub-model extractors.  Same constructor arguments, attribute names and error behaviour as the
reference (file:line cited per method); every number comes from libnif_hip.so (HIP, gfx950)."""
import collections
import contextlib
import json
import os
import time
import warnings

import numpy as np

from . import _lib
from . import distributed as dist
from .data import ShardBatches
from .engine import Engine
from .optimizers import Adam, ema_of, get as get_optimizer, grad_transform_of, slot_layout
from .spec import Spec

_global_rng = [np.random.default_rng()]

SensorResult = collections.namedtuple("SensorResult", ["point", "component", "x", "diag", "rank"])


def set_seed(seed):
    """Seed for the initial weights of models constructed afterwards (tf.random.set_seed analogue)."""
    _global_rng[0] = np.random.default_rng(seed)


class History(object):
    def __init__(self):
        self.history = {}
        self.epoch = []


class Variable(object):
    """What `model.trainable_variables` lists: name, shape, numpy()."""

    def __init__(self, model, index, name, shape):
        self._model, self._index, self.name, self.shape = model, index, name, tuple(shape)

    def numpy(self):
        return self._model.get_weights()[self._index]


class Model(object):
    """The subset of tf.keras.Model the reference's README uses (README.md:23-37, :71-117, :179-195)."""

    def __init__(self, owner, role, n_inputs=1, jac_reg=0.0):
        self._owner = owner
        self._role = role  # 'full' | 'p_to_lr' | 'p_to_w' | 'lr_to_w' | 'x_to_u_given_w' | 'x_to_phi'
        # l1 of the latent Jacobian regulariser: only the model build() returns carries it (the reference wraps JacRegLatentLayer
        # in build() alone, model.py:353-375; .model() and the sub-models train / evaluate without it).  Pushed to the shared
        # engine whenever THIS model computes a loss.
        self._jac_reg = float(jac_reg or 0.0)
        self._po_l1 = 0.0      # layers.ParameterOutputL1ActReg: l1 * sum |pnet_output| (un-normalised, regularization.py:28-30)
        self.optimizer = None
        self.loss = None
        self.stop_training = False
        self.history = None
        self._n_inputs = n_inputs


    def _push_losses(self, e, bg):
        """the loss terms THIS model adds on top of its owner's configuration, for a step / evaluation over bg rows"""
        e.set_jac_regularizer(self._jac_reg)
        if hasattr(e, "set_loss"):
            e.set_loss(self.loss or "mse")          # compile(loss=...): per model, the engine is shared
        if self._po_l1:
            a1, a2 = getattr(self._owner, "_act_reg", (0.0, 0.0))
            if a2:
                raise NotImplementedError("ParameterOutputL1ActReg on a model configured with act_l2_reg")
            e.set_activity_regularizer(a1 + self._po_l1 * float(bg), 0.0)     # the engine's term is c / B * sum |out|

    def _pop_losses(self, e):
        """back to the owner's configuration: models that share the engine (.model(), the sub-models, SobolevModel, the L-BFGS
        closures) must not inherit this model's terms"""
        e.set_jac_regularizer(0.0)
        if hasattr(e, "set_loss"):
            e.set_loss("mse")
        if self._po_l1:
            e.set_activity_regularizer(*getattr(self._owner, "_act_reg", (0.0, 0.0)))

    @contextlib.contextmanager
    def _plain_loss(self, e, loss="mse"):
        """the bare `loss(model(x), y)` of the reference's L-BFGS closures (lbfgs.py:66-68, lbfgs_V2.py:63-66 evaluate the loss
        FUNCTION on the model's output: `model.losses` -- kernel / bias / activity regularisers, JacRegLatentLayer's add_loss --
        is never added there): every regularisation term of the engine is switched off for the evaluation and restored after"""
        o = self._owner
        reg, act, sreg = getattr(o, "_reg", (0.0, 0.0)), getattr(o, "_act_reg", (0.0, 0.0)), getattr(o, "_sreg", (0.0, 0.0))
        n_pnet = o._n_pnet_params() if reg != (0.0, 0.0) else 0
        e.set_jac_regularizer(0.0)
        if hasattr(e, "set_loss"):
            e.set_loss(loss)
        if reg != (0.0, 0.0):
            e.set_regularizer(0.0, 0.0, 0, n_pnet)
        if act != (0.0, 0.0):
            e.set_activity_regularizer(0.0, 0.0)
        if sreg != (0.0, 0.0):
            e.set_shapenet_regularizer(0.0, 0.0)
        try:
            yield
        finally:
            if hasattr(e, "set_loss"):
                e.set_loss("mse")
            if reg != (0.0, 0.0):
                e.set_regularizer(reg[0], reg[1], 0, n_pnet)
            if act != (0.0, 0.0):
                e.set_activity_regularizer(*act)
            if sreg != (0.0, 0.0):
                e.set_shapenet_regularizer(*sreg)

    # ---- weights ---------------------------------------------------------------------------------
    @property
    def _engine(self):
        return self._owner._engine

    def get_weights(self):
        return self._engine.get_weights()

    def set_weights(self, weights):
        self._engine.set_weights(weights)

    @property
    def trainable_variables(self):
        return [Variable(self, i, nm, s) for i, (nm, s) in enumerate(self._engine.shapes)]

    weights = trainable_variables

    def count_params(self):
        return self._engine.n_params

    def summary(self, print_fn=print):
        print_fn('Model: "%s" (%s)' % (self._owner.__class__.__name__, self._role))
        for nm, s in self._engine.shapes:
            print_fn("  %-24s %-16s %d" % (nm, str(tuple(s)), int(np.prod(s))))
        print_fn("Total params: %d" % self._engine.n_params)

    def save_weights(self, filepath):
        """Flat parameters in Keras variable order + Adam slots, as .npz (the reference's TF-checkpoint
        format, README.md:179-195, is a TensorFlow artefact and out of scope).  Compiled with another optimizer than plain Adam: the
        weights + opt_kind, opt_step and that optimizer's slots by index (opt_m slot 0; opt_v slot 1; opt_vhat slot 2 -- amsgrad's
        vhat, centered RMSprop's mean gradient) and, for AdamW and centered RMSprop, opt_flags instead.  Compiled with use_ema: opt_ema,
        the weights' moving average (slot 3), in either layout once it exists (the slot reads all zeros before)."""
        ws = self.get_weights()
        arrs = {"w%03d" % i: w for i, w in enumerate(ws)}
        if ema_of(self.optimizer) is not None:
            avg = self._engine.get_opt_slot(3)
            if avg.any():
                arrs["opt_ema"] = avg
        path = filepath if str(filepath).endswith(".npz") else str(filepath) + ".npz"
        names = np.array([nm for nm, _ in self._engine.shapes])
        opt = self.optimizer
        if opt is not None and not self._plain_adam_slots(opt):
            e = self._engine
            kind, flags, second, third = slot_layout(opt)
            m, v, step = e.get_opt_state()
            slots = {"opt_m": m}
            if second:
                slots["opt_v"] = v
            if third:
                slots["opt_vhat"] = e.get_opt_slot(2)
            if flags & ~_lib.OPT_AMSGRAD:                # (amsgrad is read from opt_vhat's presence, as in the files written so far)
                slots["opt_flags"] = np.int32(flags)
            np.savez(path, names=names, opt_kind=np.int32(kind), opt_step=np.int64(step), **slots, **arrs, **self._extra_arrays())
            return
        m, v, step = self._engine.get_opt_state()
        np.savez(path, names=names, adam_m=m, adam_v=v, adam_step=np.int64(step), **arrs, **self._extra_arrays())

    @staticmethod
    def _plain_adam_slots(opt):
        """Adam's m and v alone (a schedule does not change the slots): the adam_m / adam_v / adam_step file"""
        return isinstance(opt, Adam) and slot_layout(opt)[1] == 0

    def _extra_arrays(self):
        """hook: arrays a wrapper adds to save_weights' file (sparsity.PrunedModel: masks, thresholds, step)"""
        return {}

    def _load_extra(self, d):
        """hook: what load_weights restores beyond the weights and the optimizer slots"""

    def load_weights(self, filepath):
        f = filepath if str(filepath).endswith(".npz") else str(filepath) + ".npz"
        d = np.load(f)
        n = len(self._engine.shapes)
        self.set_weights([d["w%03d" % i] for i in range(n)])
        opt = self.optimizer
        restored = False
        if "adam_m" in d:
            if opt is None or self._plain_adam_slots(opt):
                self._engine.set_opt_state(d["adam_m"], d["adam_v"], int(d["adam_step"]))
                self._fresh_slots = False
                restored = True
            else:
                warnings.warn("load_weights: the file holds Adam slots, the model is compiled with %s: weights loaded, "
                              "optimizer state not restored" % type(opt).__name__)
        elif "opt_kind" in d:
            kind, ams = int(d["opt_kind"]), "opt_vhat" in d
            flags = int(d["opt_flags"]) if "opt_flags" in d else (_lib.OPT_AMSGRAD if ams else 0)
            if opt is not None and not self._plain_adam_slots(opt) and slot_layout(opt)[:2] == (kind, flags):
                e = self._engine
                m = d["opt_m"]
                e.set_opt_state(m, d["opt_v"] if "opt_v" in d else np.zeros_like(m), int(d["opt_step"]))
                if ams:
                    e.set_opt_slot(2, d["opt_vhat"])
                self._fresh_slots = False
                restored = True
            else:
                warnings.warn("load_weights: the file holds the slots of another optimizer (kind %d%s) than the compiled one (%s): "
                              "weights loaded, optimizer state not restored"
                              % (kind, ", amsgrad" if ams else "", type(opt).__name__ if opt is not None else "none"))
        if restored and "opt_ema" in d and ema_of(opt) is not None:      # (behind the other slots: set_opt_state resets the average)
            self._engine.set_opt_slot(3, d["opt_ema"])
        self._load_extra(d)

    # ---- inference -------------------------------------------------------------------------------
    def _run(self, x):
        e = self._engine
        if self._role == "full":
            return e.forward(x)
        if self._role == "p_to_lr":
            return e.p_to_lr(x)
        if self._role == "p_to_w":
            if self._owner._spec.connectivity == "last_layer":   # pnet output IS the last-layer weight vector (model.py:583-585)
                return e.p_to_lr(x)
            return e.lr_to_w(e.p_to_lr(x))
        if self._role == "lr_to_w":
            return e.lr_to_w(x)
        if self._role == "x_to_u_given_w":
            if not (isinstance(x, (list, tuple)) and len(x) == 2):
                raise ValueError("model_x_to_u_given_w expects [x, w]")
            return e.x_to_u_given_w(x[0], x[1])
        if self._role == "x_to_phi":
            return e.x_to_phi(x)
        raise NotImplementedError(self._role)

    _PREDICT_CHUNK = 1 << 21

    def predict(self, x, batch_size=None, verbose=0, **kwargs):
        """Keras Model.predict: the result does not depend on batch_size; rows are staged through the device in chunks
        of max(batch_size, 2^21) so that an input table larger than the staging buffers never has to fit at once."""
        chunk = max(int(batch_size or 0), self._PREDICT_CHUNK)
        xs = list(x) if isinstance(x, (list, tuple)) else [x]
        n = int(np.shape(xs[0])[0])
        if n <= chunk:
            return self._run(x)
        outs = []
        for lo in range(0, n, chunk):
            part = [np.asarray(a)[lo:lo + chunk] for a in xs]
            outs.append(self._run(part if isinstance(x, (list, tuple)) else part[0]))
        if isinstance(outs[0], (list, tuple)):
            return [np.concatenate([o[i] for o in outs], axis=0) for i in range(len(outs[0]))]
        return np.concatenate(outs, axis=0)

    def __call__(self, x, training=False):
        return self._run(x)

    _SNAPSHOT_CHUNK_BYTES = 1 << 28

    def predict_snapshots(self, x, p=None, latent=None, batch_size=None):
        """The field of T snapshots on whole meshes: snapshot t is ONE ParameterNet input p[t] (or one latent vector latent[t], as
        model_p_to_lr returns it) for every point of its mesh -- the use the reference serves with its three-stage factorisation
        (README.md:99-117, model.py:956-986).  x [M, si]: one mesh shared by all snapshots, returns [T, M, so]; x a list / tuple of T
        arrays [M_t, si]: returns a list of T arrays [M_t, so].  out[t] is predict(hstack([tile(p[t], M_t), x_t])) without that table:
        the rows are expanded on the device, the ParameterNet runs once per snapshot and, for the last-layer class on a shared mesh,
        the ShapeNet once per mesh chunk.  Device staging is bounded by _SNAPSHOT_CHUNK_BYTES (snapshots, and the points of a long
        snapshot, go through in chunks; a shared mesh is uploaded once); the result does not depend on it nor on batch_size, which
        only raises the points per chunk."""
        s = self._owner._spec
        e = self._engine
        per_point = 4 * (s.pi_dim + s.si_dim + s.so_dim + s.pi_hidden * (1 + (s.so_dim if s.connectivity == "last_layer" else 0)))
        out = self._snapshot_run("predict_snapshots", x, p, latent, batch_size, per_point, [(s.so_dim,)],
                                 lambda *a: (e.forward_snapshots(*a),), lambda *a: (e.forward_snapshots_ragged(*a),))
        return out[0]

    def _snapshot_run(self, who, x, p, latent, batch_size, per_point, tails, shared_call, ragged_call, extra=None):
        """What the snapshot-wise calls share: the checks of x, p | latent, and the chunk plan.  tails: the trailing shape of every
        output; shared_call(rows, is_latent, mesh, lo, hi) -> arrays [T', hi - lo, *tail]; ragged_call(rows, is_latent, xs) -> arrays
        [sum M_t, *tail].  extra: a second per-snapshot array [T, ...]; the calls then get the pair (rows, extra) of their snapshots in
        the place of rows.  Returns a tuple of arrays [T, M, *tail] (shared mesh) or of lists of [M_t, *tail]."""
        if self._role != "full":
            raise ValueError("%s exists on the full model only (%s is a sub-model view)" % (who, self._role))
        if (p is None) == (latent is None):
            raise ValueError("%s: exactly one of p [T, pi] and latent [T, r]" % who)
        s = self._owner._spec
        is_latent = latent is not None
        width = s.pi_hidden if is_latent else s.pi_dim
        rows = np.asarray(latent if is_latent else p, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != width:
            raise ValueError("%s: expected %s of shape (T, %d), got %s" % (who, "latent" if is_latent else "p", width, rows.shape))
        T = rows.shape[0]
        take = (lambda idx: rows[idx]) if extra is None else (lambda idx: (rows[idx], extra[idx]))

        def mesh_of(a):
            a = np.asarray(a, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != s.si_dim:
                raise ValueError("%s: expected coordinates of shape (M, %d), got %s" % (who, s.si_dim, a.shape))
            return a

        pts = max(1, int(self._SNAPSHOT_CHUNK_BYTES) // per_point, int(batch_size or 0))
        e = self._engine
        if not isinstance(x, (list, tuple)):
            x = mesh_of(x)
            M = x.shape[0]
            outs = tuple(np.empty((T, M) + tuple(tail), dtype=np.float32) for tail in tails)
            if T == 0 or M == 0:
                return outs
            mc = min(M, pts)
            tc = max(1, pts // mc)
            mesh = e.snapshot_mesh(x)
            try:
                for lo in range(0, M, mc):
                    hi = min(M, lo + mc)
                    for t0 in range(0, T, tc):
                        for out, part in zip(outs, shared_call(take(slice(t0, t0 + tc)), is_latent, mesh, lo, hi)):
                            out[t0:t0 + tc, lo:hi] = part
            finally:
                mesh.free()
            return outs
        xs = [mesh_of(a) for a in x]
        if len(xs) != T:
            raise ValueError("%s: %d meshes for %d snapshots" % (who, len(xs), T))
        outs = tuple([np.empty((a.shape[0],) + tuple(tail), dtype=np.float32) for a in xs] for tail in tails)
        group, held = [], 0

        def flush():
            parts = ragged_call(take([t for t, _, _ in group]), is_latent, [xs[t][lo:hi] for t, lo, hi in group])
            for out, u in zip(outs, parts):
                at = 0
                for t, lo, hi in group:
                    out[t][lo:hi] = u[at:at + hi - lo]
                    at += hi - lo

        for t, a in enumerate(xs):
            for lo in range(0, a.shape[0], pts):
                hi = min(a.shape[0], lo + pts)
                if group and held + hi - lo > pts:
                    flush()
                    group, held = [], 0
                group.append((t, lo, hi))
                held += hi - lo
        if group:
            flush()
        return outs

    def predict_snapshot_derivatives(self, x, p=None, latent=None, x_index=None, y_index=None, order=1, batch_size=None):
        """predict_snapshots with the field's first (order=1) and second (order=2) derivatives in the coordinates: x, p | latent and
        batch_size as there.  x_index: distinct coordinate indices 0 <= j < si (JacobianLayer's x_index minus pi_dim; default: every
        coordinate); y_index: outputs, any order, repeats allowed, at most 16 (default: every output).  Shared mesh: returns
        (u [T, M, so], dudx [T, M, ny, nx]) and for order=2 also d2udx2 [T, M, ny, nx, nx]; a list / tuple of meshes: a tuple of lists
        of [M_t, ...] arrays.  For snapshot t they are what HessianLayer(model, y_index, [pi + j for j in x_index]) returns on
        hstack([tile(p[t], M_t), x_t]), without that table: the ParameterNet runs once per snapshot and the hypernetwork classes run
        one set of hidden products per layer and tangent stream on the snapshot's combined matrices.  Device staging is
        bounded by _SNAPSHOT_CHUNK_BYTES as in predict_snapshots; the result does not depend on it."""
        who = "predict_snapshot_derivatives"
        s = self._owner._spec
        if self._role != "full":
            raise ValueError("%s exists on the full model only (%s is a sub-model view)" % (who, self._role))
        if order not in (1, 2):
            raise ValueError("%s: order must be 1 or 2, got %r" % (who, order))
        xi = list(range(s.si_dim)) if x_index is None else [int(j) for j in x_index]
        yi = list(range(s.so_dim)) if y_index is None else [int(i) for i in y_index]
        if not xi or any(j < 0 or j >= s.si_dim for j in xi):
            raise ValueError("%s: x_index lists coordinates 0 <= j < %d (parameter columns are not built), got %r" % (who, s.si_dim, xi))
        if len(set(xi)) != len(xi):
            raise ValueError("%s: x_index repeats an index: %r" % (who, xi))
        if not yi or len(yi) > 16 or any(i < 0 or i >= s.so_dim for i in yi):
            raise ValueError("%s: y_index lists 1 to 16 outputs 0 <= i < %d, got %r" % (who, s.so_dim, yi))
        ny, nx = len(yi), len(xi)
        tails = [(s.so_dim,), (ny, nx)] + ([(ny, nx, nx)] if order == 2 else [])
        e = self._engine
        # what a point holds on the device: the forward's operands, its result rows and the kernels' rows over every output
        # (so of them; last-layer class: the so * r rows of phi)
        krows = s.so_dim * (s.pi_hidden if s.connectivity == "last_layer" else 1)
        per_point = 4 * (s.pi_dim + s.si_dim + s.so_dim + s.pi_hidden + krows + (ny + krows) * (nx + nx * nx))
        return self._snapshot_run(who, x, p, latent, batch_size, per_point, tails,
                                  lambda rows, il, mesh, lo, hi: e.snapshot_derivatives(rows, il, mesh, lo, hi, yi, xi, order),
                                  lambda rows, il, xs: e.snapshot_derivatives_ragged(rows, il, xs, yi, xi, order))

    def predict_snapshot_parameter_derivatives(self, x, p=None, p_index=None, latent=None, dlatent=None, y_index=None, order=1, d2latent=None,
                                               x_index=None, batch_size=None):
        """predict_snapshots with the field's first derivative in the other half of the input vector: x, p | latent and batch_size as
        there.  With p [T, pi]: p_index lists distinct ParameterNet input columns 0 <= c < pi (default: all of them), and
        dudp[t][m, i, c] = d u_{y_index[i]} / d p_{p_index[c]} -- for snapshot t what JacobianLayer(model, y_index, p_index) returns on
        hstack([tile(p[t], M_t), x_t]), without that table.  With latent [T, r] and dlatent [T, nd, r], 1 <= nd <= 16 directions in
        latent space per snapshot: dudp[t][m, i, d] = sum_k du_i/dz_k (latent[t]; x_m) dlatent[t, d, k] (last-layer class: the latent is
        the coefficient vector a).  y_index: outputs, any order, repeats allowed, at most 16 (default: every output).  Shared mesh:
        returns (u [T, M, so], dudp [T, M, ny, nd]); a list / tuple of meshes: a tuple of lists of [M_t, ...] arrays.  The ParameterNet
        and its tangents run once per snapshot; the hypernetwork classes run 1 + 2 g hidden products per layer for a group of g <= 3
        directions on the snapshot's combined matrices and their tangents.  Device staging is bounded by
        _SNAPSHOT_CHUNK_BYTES as in predict_snapshots; the result does not depend on it.
        order=2 (at most 8 columns or directions) adds d2udp2 [T, M, ny, nd, nd] and, with x_index (distinct coordinates 0 <= j < si),
        dudx [T, M, ny, nx] and the mixed block d2udpdx [T, M, ny, nd, nx]: returns (u, dudp, d2udp2[, dudx, d2udpdx]).  With p they are
        the blocks of what HessianLayer(model, y_index, p_index + [pi + j for j in x_index]) returns on the same table (d2udx2 stays
        with predict_snapshot_derivatives).  With latent: d2udp2[t][m, i, a, b] = d2u_i/dz2 [dlatent[t, a], dlatent[t, b]] +
        du_i/dz . d2latent[t, a, b] and d2udpdx[t][m, i, a, j] = d2u_i/dz dx_j [dlatent[t, a]]; d2latent [T, nd, nd, r] (default: zeros)
        is symmetric in its two direction axes.  u and dudp are bit for bit the order=1 call's, and d2udp2[..., a, b] and [..., b, a] are
        one value.  The hypernetwork classes run one launch per pair on the snapshot's combined matrices, their tangents and second
        tangents."""
        who = "predict_snapshot_parameter_derivatives"
        s = self._owner._spec
        if self._role != "full":
            raise ValueError("%s exists on the full model only (%s is a sub-model view)" % (who, self._role))
        if order not in (1, 2):
            raise ValueError("%s: order must be 1 or 2, got %r" % (who, order))
        if order == 1 and (d2latent is not None or x_index is not None):
            raise ValueError("%s: d2latent and x_index go with order=2" % who)
        if (p is None) == (latent is None):
            raise ValueError("%s: exactly one of p [T, pi] and latent [T, r]" % who)
        if (latent is None) != (dlatent is None):
            raise ValueError("%s: latent [T, r] and dlatent [T, nd, r] go together" % who)
        yi = list(range(s.so_dim)) if y_index is None else [int(i) for i in y_index]
        if not yi or len(yi) > 16 or any(i < 0 or i >= s.so_dim for i in yi):
            raise ValueError("%s: y_index lists 1 to 16 outputs 0 <= i < %d, got %r" % (who, s.so_dim, yi))
        if latent is not None:
            if p_index is not None:
                raise ValueError("%s: p_index goes with p, not with latent" % who)
            lat = np.asarray(latent, dtype=np.float32)
            if lat.ndim != 2 or lat.shape[1] != s.pi_hidden:
                raise ValueError("%s: expected latent of shape (T, %d), got %s" % (who, s.pi_hidden, lat.shape))
            dl = np.ascontiguousarray(dlatent, dtype=np.float32)
            if dl.ndim != 3 or dl.shape[0] != lat.shape[0] or dl.shape[2] != s.pi_hidden:
                raise ValueError("%s: expected dlatent of shape (%d, nd, %d), got %s" % (who, lat.shape[0], s.pi_hidden, dl.shape))
            if not 1 <= dl.shape[1] <= 16:
                raise ValueError("%s: 1 to 16 directions in dlatent, got %d" % (who, dl.shape[1]))
            pi_, nd = None, dl.shape[1]
        else:
            dl = None
            pi_ = list(range(s.pi_dim)) if p_index is None else [int(c) for c in p_index]
            if not pi_ or len(pi_) > 16 or any(c < 0 or c >= s.pi_dim for c in pi_):
                raise ValueError("%s: p_index lists 1 to 16 ParameterNet input columns 0 <= c < %d, got %r" % (who, s.pi_dim, pi_))
            if len(set(pi_)) != len(pi_):
                raise ValueError("%s: p_index repeats an index: %r" % (who, pi_))
            nd = len(pi_)
        ny = len(yi)
        e = self._engine
        # what a point holds on the device: the forward's operands, its result rows and the kernels' rows over every output
        # (last-layer class: also the so * r rows of phi)
        per_point = 4 * (s.pi_dim + s.si_dim + s.so_dim + s.pi_hidden * (1 + min(nd, 3)) + (ny + s.so_dim) * nd +
                         (s.so_dim * s.pi_hidden if s.connectivity == "last_layer" else 0))
        if order == 2:
            if nd > 8:
                raise ValueError("%s: order=2 takes at most 8 %s, got %d" % (who, "parameter columns" if dl is None else "directions", nd))
            xi = [] if x_index is None else [int(j) for j in x_index]
            if x_index is not None and (not xi or any(j < 0 or j >= s.si_dim for j in xi)):
                raise ValueError("%s: x_index lists coordinates 0 <= j < %d, got %r" % (who, s.si_dim, xi))
            if len(set(xi)) != len(xi):
                raise ValueError("%s: x_index repeats an index: %r" % (who, xi))
            d2 = None
            if d2latent is not None:
                if dl is None:
                    raise ValueError("%s: d2latent goes with latent and dlatent, not with p" % who)
                d2 = np.ascontiguousarray(d2latent, dtype=np.float32)
                if d2.shape != (dl.shape[0], nd, nd, s.pi_hidden):
                    raise ValueError("%s: expected d2latent of shape (%d, %d, %d, %d), got %s" % (who, dl.shape[0], nd, nd, s.pi_hidden, d2.shape))
                if not np.array_equal(d2.view(np.uint32), np.ascontiguousarray(d2.transpose(0, 2, 1, 3)).view(np.uint32)):
                    raise ValueError("%s: d2latent must be symmetric in its two direction axes (bit for bit)" % who)
            nx = len(xi)
            tails = [(s.so_dim,), (ny, nd), (ny, nd, nd)] + ([(ny, nx), (ny, nd, nx)] if nx else [])
            # the new rows: the pair and mixed results over every output, the gathered ones, and the first-order coordinate rows
            per_point += 4 * ((ny + s.so_dim) * (nd * nd + nd * nx + nx))
            if dl is None:
                return self._snapshot_run(
                    who, x, p, latent, batch_size, per_point, tails,
                    lambda rows, il, mesh, lo, hi: e.snapshot_param_second_derivatives(rows, None, None, mesh, lo, hi, yi, pi_, xi),
                    lambda rows, il, xs: e.snapshot_param_second_derivatives_ragged(rows, None, None, xs, yi, pi_, xi))
            # (one per-snapshot array beside the rows: the directions, then the nd * nd second directions)
            both = dl if d2 is None else np.concatenate([dl, d2.reshape(dl.shape[0], nd * nd, s.pi_hidden)], axis=1)
            split = (lambda b: (b, None)) if d2 is None else (lambda b: (b[:, :nd], b[:, nd:].reshape(b.shape[0], nd, nd, s.pi_hidden)))
            return self._snapshot_run(
                who, x, p, latent, batch_size, per_point, tails,
                lambda rd, il, mesh, lo, hi: e.snapshot_param_second_derivatives(rd[0], *split(rd[1]), mesh, lo, hi, yi, None, xi),
                lambda rd, il, xs: e.snapshot_param_second_derivatives_ragged(rd[0], *split(rd[1]), xs, yi, None, xi), extra=both)
        if dl is None:
            return self._snapshot_run(who, x, p, latent, batch_size, per_point, [(s.so_dim,), (ny, nd)],
                                      lambda rows, il, mesh, lo, hi: e.snapshot_param_derivatives(rows, None, mesh, lo, hi, yi, pi_),
                                      lambda rows, il, xs: e.snapshot_param_derivatives_ragged(rows, None, xs, yi, pi_))
        return self._snapshot_run(who, x, p, latent, batch_size, per_point, [(s.so_dim,), (ny, nd)],
                                  lambda rd, il, mesh, lo, hi: e.snapshot_param_derivatives(rd[0], rd[1], mesh, lo, hi, yi, None),
                                  lambda rd, il, xs: e.snapshot_param_derivatives_ragged(rd[0], rd[1], xs, yi, None), extra=dl)

    def encode_snapshots(self, x, u, latent0=None, p0=None, sample_weight=None, max_iter=20, tol=1e-8):
        """The inverse of predict_snapshots(x, latent=...): for each of T snapshots the latent whose field fits the samples u best in
        weighted least squares, by Levenberg-Marquardt from latent0 [T, r] (or from the ParameterNet's latents of p0 [T, pi]; exactly
        one of the two).  x [M, si] shared with u [T, M, so] (sample_weight [T, M]), or x and u lists / tuples of T arrays [M_t, si] and
        [M_t, so] (sample_weight a list of [M_t]); M_t = 0 is allowed and leaves that snapshot's latent as given.  The device forms every
        snapshot's normal equations in one pass per iteration (at most max_iter + 1 passes); the r x r solves and the accept / reject
        logic run on the host in float64 (nif_amd/encode.py).  With fewer samples than latent dimensions the normal matrix is
        singular: the damping keeps the step in the directions the samples see, the rest of the latent stays at its start value.
        On the device the loss bottoms out at the fp32 floor of the forward pass: with the default tol (below float32 resolution)
        later trials are rejected until max_iter and `converged` stays False although the latent has settled; a tol of about 1e-5
        stops there.
        Returns EncodeResult(latent [T, r] float32, loss [T] -- Keras' mse of each snapshot --, iterations [T], converged [T])."""
        from .encode import lm_encode
        if self._role != "full":
            raise ValueError("encode_snapshots exists on the full model only (%s is a sub-model view)" % self._role)
        if (latent0 is None) == (p0 is None):
            raise ValueError("encode_snapshots: exactly one of latent0 [T, r] and p0 [T, pi]")
        s = self._owner._spec
        from_p = p0 is not None
        width = s.pi_dim if from_p else s.pi_hidden
        rows = np.asarray(p0 if from_p else latent0, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != width:
            raise ValueError("encode_snapshots: expected %s of shape (T, %d), got %s" % ("p0" if from_p else "latent0", width, rows.shape))
        T, so, si = rows.shape[0], s.so_dim, s.si_dim
        e = self._engine

        def arr(a, ncol, what):
            a = np.asarray(a, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != ncol:
                raise ValueError("encode_snapshots: expected %s of shape (M, %d), got %s" % (what, ncol, a.shape))
            return a

        if not isinstance(x, (list, tuple)):
            x = arr(x, si, "coordinates")
            y = np.asarray(u, dtype=np.float32)
            if y.shape != (T, x.shape[0], so):
                raise ValueError("encode_snapshots: expected samples of shape (%d, %d, %d), got %s" % (T, x.shape[0], so, y.shape))
            w = None if sample_weight is None else np.asarray(sample_weight, dtype=np.float32)
            if w is not None and w.shape != (T, x.shape[0]):
                raise ValueError("encode_snapshots: expected sample_weight of shape (%d, %d), got %s" % (T, x.shape[0], w.shape))
            counts, kcounts = np.full(T, x.shape[0], dtype=np.int64), None
        else:
            if not isinstance(u, (list, tuple)) or len(x) != T or len(u) != T:
                raise ValueError("encode_snapshots: %d meshes and samples for %d snapshots" % (len(x), T))
            xs, ys = [arr(a, si, "coordinates") for a in x], [arr(a, so, "samples") for a in u]
            counts = np.array([a.shape[0] for a in xs], dtype=np.int64)
            if [a.shape[0] for a in ys] != list(counts):
                raise ValueError("encode_snapshots: samples and coordinates of a snapshot differ in length")
            w = None
            if sample_weight is not None:
                ws = [np.asarray(a, dtype=np.float32).reshape(-1) for a in sample_weight]
                if [a.size for a in ws] != list(counts):
                    raise ValueError("encode_snapshots: sample_weight and coordinates of a snapshot differ in length")
                w = np.concatenate(ws) if T else np.empty((0,), np.float32)
            x = np.concatenate(xs, axis=0) if T else np.empty((0, si), np.float32)
            y = np.concatenate(ys, axis=0) if T else np.empty((0, so), np.float32)
            kcounts = counts
        z0 = e.p_to_lr(rows) if from_p else rows
        if T == 0 or not counts.any():
            return lm_encode(None, z0, counts, so, max_iter, tol)
        samples = e.snapshot_samples(x, y, w, kcounts)
        try:
            return lm_encode(lambda lat: e.snapshot_normal_eq(lat, samples), z0, counts, so, max_iter, tol)
        finally:
            samples.free()

    def select_sensors(self, x, n_sensors=None, mask=None, rtol=None):
        """Where to put sensors on the mesh x [M, si] so that encode_snapshots recovers a field's latent well from readings there:
        QDEIM on the learned basis.  For NIFMultiScaleLastLayerParameterized u_t(x) = phi(x) . a(p_t) + bias, and the candidates are
        the M so rows of model_x_to_phi(x) reshaped [M so, r], a sensor being a (point, component) pair; the device runs the greedy
        column-pivoted QR of Phi^T (include/nif_hip_sensors.h): each step takes the candidate with the largest residual norm d_k
        (ties: the lowest row) and projects its direction out of every row.  n_sensors defaults to r and cannot exceed it (more
        sensors than r is oversampling, a different algorithm); mask [M] bool marks the points where a sensor can stand (None: all).
        The result is cut at the first step with d_k <= rtol d_0 (default rtol: r float32 epsilons; rtol=0 keeps every step that found
        a row): `rank` sensors are returned, fewer than asked for when the candidates or the rank of phi run out.
        Returns SensorResult(point [K'] int64, component [K'] int64, x [K', si] -- x[point] --, diag [K'] float32 -- the d_k --, rank
        = K').  To use it, pass xs = x[np.unique(point)] and the readings u[:, np.unique(point), :] there to
        encode_snapshots(xs, readings, ...): a sensor that reads all so components at its point only adds rows to the least-squares
        problem.  Not built: the hypernetwork classes (their basis du/dz depends on the latent), n_sensors > r, whole points as
        pivots, weighted candidates, more than one GPU."""
        if self._role != "full":
            raise ValueError("select_sensors exists on the full model only (%s is a sub-model view)" % self._role)
        s = self._owner._spec
        if s.kind != "NIFMultiScaleLastLayerParameterized":
            raise NotImplementedError("select_sensors: built for NIFMultiScaleLastLayerParameterized, whose fields are linear in the "
                                      "fixed basis phi(x); the basis of %s depends on the latent, and selection on du/dz at a given "
                                      "latent is not built" % s.kind)
        r, so = s.pi_hidden, s.so_dim
        x = np.asarray(x, dtype=np.float32)
        if x.ndim == 1 and s.si_dim == 1:
            x = x[:, None]
        if x.ndim != 2 or x.shape[1] != s.si_dim or x.shape[0] < 1:
            raise ValueError("select_sensors: x must have shape (M >= 1, si_dim=%d), got %r" % (s.si_dim, x.shape))
        k = r if n_sensors is None else int(n_sensors)
        if k < 1 or k > r:
            raise ValueError("select_sensors: n_sensors = %d outside 1 .. latent_dim = %d (more sensors than latent dimensions is "
                             "oversampling, which is not built)" % (k, r))
        if mask is not None:
            mask = np.asarray(mask)
            if mask.shape != (x.shape[0],):
                raise ValueError("select_sensors: mask must have shape (M=%d,), got %r" % (x.shape[0], mask.shape))
            mask = mask != 0
        rtol = float(r * np.finfo(np.float32).eps if rtol is None else rtol)
        if rtol < 0.0:
            raise ValueError("select_sensors: rtol >= 0")
        piv, diag = self._engine.select_sensors(x, k, mask)
        piv, diag = np.asarray(piv, dtype=np.int64), np.asarray(diag, dtype=np.float32)
        keep = (piv >= 0) & (diag > np.float32(rtol) * diag[0])
        rank = int(k if keep.all() else np.argmin(keep))
        piv, diag = piv[:rank], diag[:rank]
        point, component = piv // so, piv % so
        return SensorResult(point, component, x[point], diag, rank)

    # ---- training --------------------------------------------------------------------------------
    # Keras' compile(metrics=[...]): names / metric objects -> (history key, kind).  Unweighted (Keras applies sample_weight to
    # `weighted_metrics` only); the value of an epoch is the running mean over every sample the epoch saw, evaluated with the weights
    # each batch's loss was evaluated with (before its update).  Computed on the host from a forward pass per batch: metrics are off
    # the hot path and cost nothing unless asked for
    _METRIC_KINDS = {"mse": "mse", "mean_squared_error": "mse", "MSE": "mse", "mae": "mae", "mean_absolute_error": "mae", "MAE": "mae",
                     "root_mean_squared_error": "rmse", "rmse": "rmse"}

    def _parse_metrics(self, metrics):
        out = []
        for mtr in ([metrics] if isinstance(metrics, str) else list(metrics or [])):
            key = mtr if isinstance(mtr, str) else (getattr(mtr, "name", None) or getattr(mtr, "__name__", None))
            if key not in self._METRIC_KINDS:
                raise NotImplementedError("compile(metrics=[%r]): built are 'mse' / 'mean_squared_error', 'mae' / 'mean_absolute_error' and "
                                          "RootMeanSquaredError (by name or Keras object)" % (mtr,))
            out.append((key, self._METRIC_KINDS[key]))
        return out

    @staticmethod
    def _metric_sums(kinds, u, y):
        """per-batch sums whose ratio to the sample count is the metric (rmse: the root is taken at the end)"""
        d = np.asarray(u, dtype=np.float64) - np.asarray(y, dtype=np.float64)
        return [float(np.abs(d).mean(axis=1).sum()) if k == "mae" else float((d * d).mean(axis=1).sum()) for _, k in kinds]

    @staticmethod
    def _metric_values(kinds, sums, count):
        return {key: (np.sqrt(s_ / max(count, 1)) if k == "rmse" else s_ / max(count, 1)) for (key, k), s_ in zip(kinds, sums)}

    def compile(self, optimizer="adam", loss="mse", metrics=None, **kwargs):
        if self._role != "full":
            raise ValueError("only the full model can be compiled for training")
        name = loss if isinstance(loss, str) else (getattr(loss, "name", None) or getattr(loss, "__name__", None))
        if not isinstance(loss, str):      # a loss OBJECT: only its defaults are built (huber: delta = 1 in the kernels; Keras' default reduction)
            if float(getattr(loss, "delta", 1.0)) != 1.0:
                raise NotImplementedError("loss=%r: huber with delta != 1" % (loss,))
            red = getattr(loss, "reduction", None)
            if red is not None and str(red).lower().rsplit(".", 1)[-1] not in ("auto", "sum_over_batch_size"):
                raise NotImplementedError("loss=%r: reduction %r (built: the default SUM_OVER_BATCH_SIZE)" % (loss, red))
        if name not in _lib.LOSS_IDS:
            raise NotImplementedError("loss=%r: built are 'mse' (README.md:33), 'mae', 'huber' (delta 1), 'log_cosh'" % (loss,))
        if kwargs:
            raise NotImplementedError("compile(%s): not on the built hot path" % ", ".join(sorted(kwargs)))
        self._metrics = self._parse_metrics(metrics)
        if self._metrics and self._n_tangents() != 0:
            raise NotImplementedError("compile(metrics=...) on the two-output model")
        new = get_optimizer(optimizer)
        grad_transform_of(new)           # (a marker of centralized_gradients_for_optimizer on new.get_gradients, Adam's clip keywords:
                                         # checked here, read again at the start of every fit())
        if new is not self.optimizer:
            self._fresh_slots = True     # Keras: a newly compiled optimizer starts with zero slots and iteration 0
        self.optimizer = new
        self.loss = ("mse", "mae", "huber", "log_cosh")[_lib.LOSS_IDS[name]]

    _EVAL_CHUNK = 1 << 18
    # fit(): epochs of at least four batches no larger than _GRAPH_MAX_BATCH can be captured into a hipGraph (NIF_GRAPH=1 or
    # model._graph_epochs = True).  OFF by default: measured on configs[0] (10 k points, batch 512, tools/exp/small_batch.py) the
    # replayed epoch runs 83.3 us per step against 84.8 us eager -- the step is the sum of its 11 kernels' EXECUTION times (fixed
    # prologue / epilogue costs of persistent kernels built for 1e6 points: DESIGN 8.6), not host launch cost or dispatch gaps
    _GRAPH_MAX_BATCH = 16384
    _graph_epochs = os.environ.get("NIF_GRAPH", "0") == "1"

    def evaluate(self, x, y, sample_weight=None, verbose=0, **kwargs):
        """Keras Model.evaluate: the TOTAL loss -- sample-weighted mse plus every regularisation loss of the model (kernel / bias
        L1 / L2, the ParameterNet activity regulariser, the latent Jacobian regulariser of build()), as `fit` logs it; evaluated
        through the engine's loss kernels in chunks, each chunk's loss weighted by its rows (Keras' batch-weighted mean); only
        the scalar of a chunk travels back.  The sub-models (model_p_to_lr() ...) are never compiled -- in Keras their evaluate()
        raises, and so does this one."""
        if self._role != "full":
            raise RuntimeError("You must compile your model before training/testing. Use `model.compile(optimizer, loss)`. "
                               "(only the full model can be compiled; %s is an inference-only view of its variables)" % self._role)
        e = self._engine
        x = np.asarray(x); n = x.shape[0]
        if n == 0:
            return 0.0
        targets = self._targets(y, n)
        tot = 0.0
        try:
            for lo in range(0, n, self._EVAL_CHUNK):
                hi = min(n, lo + self._EVAL_CHUNK)
                sw = None if sample_weight is None else np.asarray(sample_weight)[lo:hi]
                self._push_losses(e, hi - lo)
                tot += (hi - lo) * self._loss_host(e, x[lo:hi], [t[lo:hi] for t in targets], sw)
        finally:
            self._pop_losses(e)
        kinds = getattr(self, "_metrics", [])
        if kinds:      # Keras: [loss, metric, ...] when metrics were compiled
            sums = self._metric_sums(kinds, self.predict(x), targets[0])
            vals = self._metric_values(kinds, sums, n)
            return [float(tot / n)] + [float(vals[k]) for k, _ in kinds]
        return float(tot / n)

    # hooks the two-output Sobolev model overrides
    def _targets(self, y, n_rows):
        y = np.ascontiguousarray(y, dtype=np.float32)
        if y.ndim == 1:
            y = y[:, None]
        if y.shape != (n_rows, self._owner._spec.so_dim):
            raise ValueError("y must have shape (N, so_dim=%d), got %r" % (self._owner._spec.so_dim, y.shape))
        return [y]

    def _loss_grad_dev(self, e, d_x, d_targets, d_sw, b, bg):
        e.loss_grad_dev(d_x, d_targets[0], d_sw, b, bg)

    def _loss_host(self, e, x, targets, sw):
        """total loss of one evaluation chunk (host arrays)"""
        return e.loss_and_grad(x, targets[0], sw, want_grad=False)[0]

    def _n_tangents(self):
        return 0

    def _scaled_weights(self, sw, n_rows):
        """sample weights as the engine sees them (hook of the two-output model: an overall loss weight rides on them)"""
        return sw

    def _batch_hook(self, e, callbacks):
        """hook: None, or what fit() runs at the start of every batch, before anything else the batch does (sparsity.PrunedModel:
        the pruning step, the mask update on a pruning turn, the masks applied); called once per fit after on_train_begin"""
        return None

    def fit(self, x=None, y=None, batch_size=None, epochs=1, verbose=1, callbacks=None, shuffle=True,
            sample_weight=None, initial_epoch=0, validation_data=None, validation_split=0.0, steps_per_epoch=None, **kwargs):
        """Keras Model.fit semantics for in-memory arrays (or one file of a shard dataset, nif_amd.data): per epoch
        optionally shuffle, walk batches of `batch_size` (default 32, last one partial), one Adam step per batch; the
        epoch 'loss' is the sample-weighted mean of the batch losses.  The table is made resident in HBM once; a
        shuffled epoch uploads only its permutation and gathers on the device; batches are device-pointer slices.  Under `nif_amd.distributed` every rank walks its own
        shard and the flat gradient is SUM-all-reduced (RCCL) before the identical Adam update
        (tf.distribute.MirroredStrategy, README.md:39-49).
        validation_data = (x_val, y_val[, sample_weight_val]): Keras' per-epoch evaluation, logged as 'val_loss' (seen by the
        callbacks and History; evaluated through predict on this rank's device)."""
        if validation_data is not None and not (isinstance(validation_data, (tuple, list)) and len(validation_data) in (2, 3)):
            raise ValueError("validation_data = (x_val, y_val) or (x_val, y_val, sample_weight_val)")
        if validation_split and validation_data is None:
            # Keras: "the validation data is selected from the last samples in the x and y data provided, before shuffling"
            if not 0.0 < float(validation_split) < 1.0:
                raise ValueError("`validation_split` must be between 0 and 1, received: %r" % (validation_split,))
            if isinstance(x, ShardBatches):
                raise ValueError("`validation_split` is only supported for arrays")
            n_all = int(np.shape(x)[0])
            at = int(np.floor(n_all * (1.0 - float(validation_split))))
            if at == 0 or at == n_all:
                raise ValueError("Training data contains %d samples, which is not sufficient to split it into a validation and "
                                 "training set as specified by `validation_split=%r`" % (n_all, validation_split))
            cut = lambda a, lo, hi: [np.asarray(t)[lo:hi] for t in a] if isinstance(a, (list, tuple)) else np.asarray(a)[lo:hi]
            val = (cut(x, at, n_all), cut(y, at, n_all)) + (() if sample_weight is None else (np.asarray(sample_weight)[at:],))
            return self.fit(cut(x, 0, at), cut(y, 0, at), batch_size=batch_size, epochs=epochs, verbose=verbose, callbacks=callbacks,
                            shuffle=shuffle, sample_weight=None if sample_weight is None else np.asarray(sample_weight)[:at],
                            initial_epoch=initial_epoch, validation_data=val, steps_per_epoch=steps_per_epoch, **kwargs)
        if self.optimizer is None:
            raise RuntimeError("You must compile your model before training/testing. Use `model.compile(optimizer, loss)`.")
        if kwargs:
            raise NotImplementedError("fit(%s): not on the built hot path (in-memory x, y, sample_weight only)"
                                      % ", ".join(sorted(kwargs)))
        ema = ema_of(self.optimizer)
        if ema is not None and getattr(self, "_is_pruned", False):
            raise NotImplementedError("fit() of a pruned model (nif_amd.sparsity) with %s(use_ema=True): not built (the average of "
                                      "unmasked weights written back over masked ones)" % type(self.optimizer).__name__)
        s = self._owner._spec
        e = self._engine
        kinds = getattr(self, "_metrics", [])
        if kinds and (isinstance(x, ShardBatches) or dist.get() is not None):
            raise NotImplementedError("compile(metrics=...): in-memory arrays on one GPU")
        self._push_losses(e, 1)                   # (raises here, not at first engine access, when the shape has no kernel for it)
        # the optimizer's gradient transform (Adam's clip keywords, centralized_gradients_for_optimizer), read now and engine state for
        # the length of this call: cleared in the `finally` below, like the loss terms (a later TFPLBFGS or another model on the
        # shared engine steps without it)
        grad_tf = grad_transform_of(self.optimizer)
        if grad_tf is not None:
            e.set_grad_transform(grad_tf)
        try:
            # Keras' use_ema: engine state for the length of this call as well (every optimizer step of the context keeps the average)
            if ema is not None:
                e.set_ema(*ema)
            return self._fit(e, s, kinds, x, y, batch_size, epochs, verbose, callbacks, shuffle, sample_weight, initial_epoch,
                             validation_data, steps_per_epoch)
        finally:
            if grad_tf is not None:
                e.set_grad_transform(None)
            if ema is not None:
                e.set_ema(None)

    def fit_snapshots(self, x, u, p, sample_weight=None, epochs=1, snapshots_per_step=None, shuffle=True, callbacks=None, verbose=0,
                      initial_epoch=0):
        """fit() for T snapshots u [T, M, so] on one shared mesh x [M, si] with the ParameterNet inputs p [T, pi], without the
        [T M, pi + si] table: for NIFMultiScaleLastLayerParameterized the field is phi(x) . a(p) + bias, so a step runs the ShapeNet
        over the M mesh points and the ParameterNet over its snapshots' rows of p, and only the head is O(T M)
        (include/nif_hip_snapfit.h).  A step is `snapshots_per_step` whole snapshots on the full mesh (None: all T; the last step of an
        epoch may be shorter); per epoch one permutation of the snapshots, gathered on the device.  It computes what fit() computes on
        the expanded table hstack([repeat(p, M), tile(x, T)]) with batch_size = snapshots_per_step * M and the same snapshots per
        batch.  sample_weight: [T, M], [M] (per mesh point) or [T] (per snapshot).  Behind every step the tail of fit(): the compiled
        optimizer with its gradient transform and weight average, the pruning hooks, the loss metric, callbacks and History["loss"].
        Not built: the hypernetwork classes, mesh blocks per step, ragged meshes, mixed policies, the activity and latent-Jacobian
        regularisers, more than one GPU, compile(metrics=...)."""
        if self._role != "full" or self.optimizer is None:
            raise RuntimeError("You must compile your model before training/testing. Use `model.compile(optimizer, loss)`.")
        s = self._owner._spec
        if s.kind != "NIFMultiScaleLastLayerParameterized":
            raise NotImplementedError("fit_snapshots: built for NIFMultiScaleLastLayerParameterized, whose field factors into "
                                      "phi(x) . a(p); %s needs a per-snapshot weight-gradient kernel that does not exist "
                                      "(fit() on the expanded table trains it)" % s.kind)
        if s.mixed_policy != "float32":
            raise NotImplementedError("fit_snapshots: not built for the %s policy" % s.mixed_policy)
        comm = dist.get()
        if comm is not None and comm.world > 1:
            raise NotImplementedError("fit_snapshots: one GPU (world = %d)" % comm.world)
        if getattr(self, "_metrics", []):
            raise NotImplementedError("fit_snapshots: compile(metrics=...) is not built (History carries 'loss')")
        if self._jac_reg or self._po_l1 or tuple(getattr(self._owner, "_act_reg", (0.0, 0.0))) != (0.0, 0.0):
            raise NotImplementedError("fit_snapshots: not built with an activity or latent-Jacobian regulariser")
        ema = ema_of(self.optimizer)
        if ema is not None and getattr(self, "_is_pruned", False):
            raise NotImplementedError("fit_snapshots() of a pruned model (nif_amd.sparsity) with %s(use_ema=True): not built"
                                      % type(self.optimizer).__name__)
        x = np.ascontiguousarray(x, dtype=np.float32)
        p = np.ascontiguousarray(p, dtype=np.float32)
        if p.ndim == 1 and s.pi_dim == 1:
            p = p[:, None]
        if x.ndim == 1 and s.si_dim == 1:
            x = x[:, None]
        if x.ndim != 2 or x.shape[1] != s.si_dim:
            raise ValueError("fit_snapshots: x must have shape (M, si_dim=%d), got %r" % (s.si_dim, x.shape))
        if p.ndim != 2 or p.shape[1] != s.pi_dim:
            raise ValueError("fit_snapshots: p must have shape (T, pi_dim=%d), got %r" % (s.pi_dim, p.shape))
        T, M = p.shape[0], x.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float32)
        if u.shape == (T, M) and s.so_dim == 1:
            u = u[:, :, None]
        if u.shape != (T, M, s.so_dim):
            raise ValueError("fit_snapshots: u must have shape (T=%d, M=%d, so_dim=%d), got %r" % (T, M, s.so_dim, u.shape))
        sw = None
        if sample_weight is not None:
            w = np.asarray(sample_weight, dtype=np.float32)
            if w.shape == (T, M):
                sw = w
            elif w.shape == (M,):           # (T == M: a vector weighs the mesh points)
                sw = np.broadcast_to(w[None, :], (T, M))
            elif w.shape == (T,):
                sw = np.broadcast_to(w[:, None], (T, M))
            else:
                raise ValueError("fit_snapshots: sample_weight must have shape (T, M), (M,) or (T,) = (%d, %d), got %r" % (T, M, w.shape))
            sw = np.ascontiguousarray(sw, dtype=np.float32)
        k = T if snapshots_per_step is None else int(snapshots_per_step)
        if T > 0 and k < 1:
            raise ValueError("snapshots_per_step must be a positive integer")
        e = self._engine
        self._push_losses(e, 1)
        grad_tf = grad_transform_of(self.optimizer)
        if grad_tf is not None:
            e.set_grad_transform(grad_tf)
        try:
            if ema is not None:
                e.set_ema(*ema)
            return self._fit_snapshots(e, s, x, u, p, sw, T, M, k, epochs, shuffle, callbacks, verbose, initial_epoch)
        finally:
            if grad_tf is not None:
                e.set_grad_transform(None)
            if ema is not None:
                e.set_ema(None)

    def _fit_snapshots(self, e, s, x, u, p, sw, T, M, k, epochs, shuffle, callbacks, verbose, initial_epoch):
        self.stop_training = False
        is_adam = self._fresh_slots_init(e)
        pi, row = s.pi_dim, M * s.so_dim          # a snapshot's row of p, and of u as [T][M so]
        callbacks = list(callbacks or [])
        hist = History()
        owned = []

        def resident(host, n):
            d = e.alloc(max(1, n)); owned.append(d)
            if host is not None and n:
                d.upload(host)
            return d
        try:
            d_x = resident(x, x.size)
            src_p, src_u = resident(p, p.size), resident(u, u.size)
            src_w = resident(sw, sw.size) if sw is not None else None
            for cb in callbacks:
                if hasattr(cb, "set_model"):
                    cb.set_model(self)
            for cb in callbacks:
                if hasattr(cb, "on_train_begin"):
                    cb.on_train_begin({})
            gather = bool(shuffle) and T > 0 and M > 0
            d_p, d_u, d_w = src_p, src_u, src_w
            if gather:      # one permutation of the snapshots per epoch: 4 bytes per snapshot travel, the rows move on the device
                d_p, d_u = resident(None, p.size), resident(None, u.size)
                d_w = resident(None, sw.size) if sw is not None else None
                d_perm = resident(None, T)
            rng = np.random.default_rng(getattr(self, "_shuffle_seed", None))
            steps = [min(k, T - t0) for t0 in range(0, T, k)] if T > 0 and M > 0 else []
            batch_hook = self._batch_hook(e, callbacks)
            for epoch in range(initial_epoch, epochs):
                if self.stop_training:
                    break
                for cb in callbacks:
                    if hasattr(cb, "on_epoch_begin"):
                        cb.on_epoch_begin(epoch, {})
                t_start = time.time()
                if gather:
                    perm = rng.permutation(T).astype(np.int32)
                    d_perm.upload(perm.view(np.float32))
                    e.gather_rows(src_p, d_perm, T, pi, d_p)
                    e.gather_rows(src_u, d_perm, T, row, d_u)
                    if sw is not None:
                        e.gather_rows(src_w, d_perm, T, M, d_w)
                adam = self.optimizer.as_struct() if is_adam else self.optimizer.as_opt()
                step_dev = e.adam_step_dev if is_adam else e.opt_step_dev
                self._push_losses(e, 1)           # (a callback of the previous epoch may have evaluated another model on the shared engine)
                e.metric_read(reset=True)
                t0 = 0
                for ts in steps:
                    bg = ts * M
                    if batch_hook is not None:
                        batch_hook()
                    e.snapshot_loss_grad_dev(d_p.at(t0 * pi), ts, d_x.at(0), M, d_u.at(t0 * row),
                                             d_w.at(t0 * M) if d_w is not None else None, bg)
                    self._step_tail(e, None, step_dev, adam, bg)
                    t0 += ts
                tot, cnt = e.metric_read(reset=True)   # accumulated on the device: one host sync per epoch
                logs = {"loss": tot / max(cnt, 1.0)}
                for cb in callbacks:
                    if hasattr(cb, "on_epoch_end"):
                        cb.on_epoch_end(epoch, logs)
                hist.epoch.append(epoch)
                for key, v in logs.items():
                    hist.history.setdefault(key, []).append(v)
                if verbose:
                    print("Epoch %d/%d - %.2fs - loss: %.4e" % (epoch + 1, epochs, time.time() - t_start, logs["loss"]))
        finally:
            self._pop_losses(e)
            e.sync()
            for arr in owned:
                arr.free()
        if ema_of(self.optimizer) is not None and epochs > initial_epoch:
            self.optimizer.finalize_variable_values(self)
        for cb in callbacks:
            if hasattr(cb, "on_train_end"):
                cb.on_train_end({})
        self.history = hist
        return hist

    # what fit() and fit_snapshots() share around their loss-and-gradient calls
    def _fresh_slots_init(self, e):
        """a newly compiled optimizer starts with zero slots and iteration 0; returns whether the step travels as a plain Adam struct
        (else as a nif_opt)"""
        if getattr(self, "_fresh_slots", False):
            z = np.zeros((e.n_params,), dtype=np.float32)
            acc0 = getattr(self.optimizer, "initial_accumulator_value", None)      # Adagrad's slot 0 starts there
            e.set_opt_state(z if acc0 is None else np.full_like(z, acc0), z, 0)
            if slot_layout(self.optimizer)[3]:
                e.set_opt_slot(2, z)
            if ema_of(self.optimizer) is not None:
                e.set_opt_slot(3, e.get_flat())      # Keras creates the average with the variable's value (exists before a captured epoch)
            self._fresh_slots = False
        return isinstance(self.optimizer, Adam) and self.optimizer.is_plain

    @staticmethod
    def _step_tail(e, comm, step_dev, adam, bg):
        """behind a step's [grad | loss]: the cross-rank sum (comm: more than one rank), the optimizer step (with it the gradient
        transform, the regularisers' term and the weight average, all engine state) and Keras' loss metric -- the sample-weighted mean
        over the batches"""
        if comm is not None:
            comm.all_reduce_grad(e)
        step_dev(adam)
        e.metric_accumulate(bg)

    def _fit(self, e, s, kinds, x, y, batch_size, epochs, verbose, callbacks, shuffle, sample_weight, initial_epoch, validation_data,
             steps_per_epoch):
        self.stop_training = False
        is_adam = self._fresh_slots_init(e)
        ncol = s.pi_dim + s.si_dim
        shard = x if isinstance(x, ShardBatches) else None
        if shard is not None:
            # one file of a sharded dataset (nif_amd.data.NPZShardDataset, the TFRDataset replacement): its columns are
            # already on their way to (or in) HBM through the double-buffered copy stream; fit() trains on the slot
            if y is not None or sample_weight is not None:
                raise ValueError("a shard dataset carries its own targets and weights")
            if batch_size is not None and int(batch_size) != shard.batch_size:
                raise ValueError("the batch size was fixed by gen_dataset_from_batch_file")
            batch_size = shard.batch_size
            shuffle = shard.shuffle
            N = shard.n_rows
            widths = shard.widths(self)
            if self._scaled_weights(None, 1) is not None:
                raise NotImplementedError("loss_weights[0] != 1 with a shard dataset: fold the factor into the shards' sample weights")
            src_x, src_t, src_sw = shard.device_tables(e, self)
            has_sw = src_sw is not None
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            targets = self._targets(y, x.shape[0])   # list of [N, width] tables that travel with x
            if x.shape[1] != ncol:
                x = np.ascontiguousarray(x[:, :ncol])
            N = x.shape[0]
            sw = None if sample_weight is None else np.ascontiguousarray(sample_weight, dtype=np.float32)
            sw = self._scaled_weights(sw, N)
            widths = [t.shape[1] for t in targets]
            has_sw = sw is not None
            # the table is made resident in HBM ONCE; a shuffled epoch uploads its permutation (4 bytes per row) and
            # gathers on the device
            src_x = e.alloc(N * ncol); src_x.upload(x)
            src_t = []
            for t in targets:
                dt = e.alloc(t.size); dt.upload(t); src_t.append(dt)
            src_sw = None
            if has_sw:
                src_sw = e.alloc(N); src_sw.upload(sw)
        bs = 32 if batch_size is None else int(batch_size)
        callbacks = list(callbacks or [])
        hist = History()
        owned = [] if shard is not None else [src_x] + src_t + ([src_sw] if has_sw else [])
        try:
            for cb in callbacks:
                if hasattr(cb, "set_model"):
                    cb.set_model(self)
            for cb in callbacks:
                if hasattr(cb, "on_train_begin"):
                    cb.on_train_begin({})
            # a shuffled epoch gathers the resident table into a second one on the device (4 bytes of permutation per row
            # travel); when HBM has no room for the second copy the epoch is permuted on the host and uploaded instead
            dev_shuffle = bool(shuffle) and N > 0
            if dev_shuffle:
                try:
                    d_x = e.alloc(N * ncol); owned.append(d_x)
                    d_t = []
                    for w in widths:
                        d_t.append(e.alloc(N * w)); owned.append(d_t[-1])
                    d_sw = None
                    if has_sw:
                        d_sw = e.alloc(N); owned.append(d_sw)
                    d_perm = e.alloc(N); owned.append(d_perm)
                except _lib.NifError:
                    if shard is not None:
                        raise
                    for arr in owned[1 + len(src_t) + (1 if has_sw else 0):]:
                        arr.free()
                    del owned[1 + len(src_t) + (1 if has_sw else 0):]
                    dev_shuffle = False
            if not dev_shuffle:
                d_x, d_t, d_sw = src_x, src_t, src_sw
            host_shuffle = bool(shuffle) and N > 0 and not dev_shuffle
            rng = np.random.default_rng(getattr(self, "_shuffle_seed", None))
            comm = dist.get()
            world = comm.world if comm is not None else 1
            # every rank walks its own shard; the global size of every step's batch is agreed ONCE per call, ranks whose
            # shard is a batch shorter (or empty) join the collectives of the steps they lack with a zero gradient
            sizes, gsizes = dist.plan_steps(N, bs, comm, e)
            e.reserve(max(1, max(sizes, default=0)), self._n_tangents())
            graph_id = None
            batch_hook = self._batch_hook(e, callbacks)
            use_graph = (self._graph_epochs and world == 1 and shard is None and not self._po_l1 and not kinds and len(sizes) >= 4
                         and batch_hook is None
                         and max(sizes) <= self._GRAPH_MAX_BATCH and hasattr(e, "graph_begin") and epochs - initial_epoch >= 2)
            stream = [-1, 0]          # steps_per_epoch: (pass, next batch of the pass) of the one iterator over `epochs` passes
            cur_perm = [None]         # the permutation of the pass the resident table holds (a pass may span epochs under steps_per_epoch:
                                      # the metric forward of a batch reads the host rows through it -- ADVICE r4)
            if steps_per_epoch is not None:
                if int(steps_per_epoch) < 1:
                    raise ValueError("steps_per_epoch must be a positive integer")
                if world > 1 or shard is not None:
                    raise NotImplementedError("steps_per_epoch: in-memory arrays on one GPU (ranks with uneven shards would disagree on the stream)")
            for epoch in range(initial_epoch, epochs):
                if self.stop_training:
                    break
                for cb in callbacks:
                    if hasattr(cb, "on_epoch_begin"):
                        cb.on_epoch_begin(epoch, {})
                t0 = time.time()

                msum, mcnt = [0.0] * len(kinds), [0]

                def new_pass():      # one pass over the table = one permutation (Keras: the adapter's dataset of `epochs` passes)
                    cur_perm[0] = None
                    if dev_shuffle:
                        perm = rng.permutation(N).astype(np.int32)
                        cur_perm[0] = perm
                        d_perm.upload(perm.view(np.float32))
                        e.gather_rows(src_x, d_perm, N, ncol, d_x)
                        for st_, dt, w in zip(src_t, d_t, widths):
                            e.gather_rows(st_, d_perm, N, w, dt)
                        if has_sw:
                            e.gather_rows(src_sw, d_perm, N, 1, d_sw)
                    elif host_shuffle:
                        perm = rng.permutation(N)
                        cur_perm[0] = perm
                        e.sync()                      # the previous pass's steps have read the table
                        src_x.upload(x[perm])
                        for dt, t in zip(src_t, targets):
                            dt.upload(t[perm])
                        if has_sw:
                            src_sw.upload(sw[perm])
                adam = self.optimizer.as_struct() if is_adam else self.optimizer.as_opt()    # (every other kind: a nif_opt)
                step_dev = e.adam_step_dev if is_adam else e.opt_step_dev
                self._push_losses(e, 1)           # (a callback of the previous epoch may have evaluated another model on the shared engine)
                e.metric_read(reset=True)

                def run_batches(lo=0, hi=None):
                    for ib in range(lo, len(sizes) if hi is None else hi):
                        b, bg = sizes[ib], gsizes[ib]
                        b0 = ib * bs
                        if batch_hook is not None:
                            batch_hook()
                        if self._po_l1:
                            self._push_losses(e, bg)
                        if kinds and b > 0:      # compile(metrics=...): the batch's predictions with the weights its loss sees
                            rows = slice(b0, b0 + b) if cur_perm[0] is None else cur_perm[0][b0:b0 + b]
                            for i_, v_ in enumerate(self._metric_sums(kinds, e.forward(x[rows]), targets[0][rows])):
                                msum[i_] += v_
                            mcnt[0] += b
                        if b > 0:
                            self._loss_grad_dev(e, d_x.at(b0 * ncol), [dt.at(b0 * w) for dt, w in zip(d_t, widths)],
                                                d_sw.at(b0) if d_sw is not None else None, b, bg)
                        else:
                            e.zero_grad()
                        self._step_tail(e, comm if world > 1 else None, step_dev, adam, bg)
                if steps_per_epoch is not None:
                    # Keras with array inputs and steps_per_epoch (TensorLikeDataAdapter: ONE iterator over `epochs` successive passes,
                    # never recreated): an epoch takes its steps from where the last one stopped, a new permutation whenever a pass is
                    # used up; when the passes run out Keras warns ("Your input ran out of data") and interrupts training
                    left = int(steps_per_epoch)
                    while left > 0 and not self.stop_training:
                        if stream[1] >= len(sizes) or stream[0] < 0:
                            stream[0] += 1; stream[1] = 0
                            if stream[0] >= epochs - initial_epoch:
                                import warnings
                                warnings.warn("Your input ran out of data; interrupting training. Make sure that your dataset can "
                                              "generate at least `steps_per_epoch * epochs` batches.")
                                self.stop_training = True
                                break
                            new_pass()
                        take = min(left, len(sizes) - stream[1])
                        run_batches(stream[1], stream[1] + take)
                        stream[1] += take; left -= take
                else:
                    new_pass()
                # launch-bound epochs (many small batches on one GPU: configs[0]'s batch 512 is 13 kernels of a few microseconds per
                # step) are recorded ONCE into a hipGraph -- the batch pointers into the resident table do not change between
                # epochs -- and replayed with one submission per epoch; Keras runs its steps from one traced graph as well
                if steps_per_epoch is not None:
                    pass
                elif use_graph and graph_id is None:
                    began = False
                    try:
                        e.graph_begin()           # (raises before anything is recorded: nothing to end then -- ADVICE r4)
                        began = True
                        run_batches()
                        graph_id = e.graph_end()
                        began = False
                    except _lib.NifError:
                        use_graph, graph_id = False, None       # (a workspace that had to grow, a call that cannot be captured): plain launches
                    finally:
                        if began:                 # ANY exception inside the capture (a NifError, a KeyboardInterrupt, an error of the
                            try:                  # communicator ...): end the capture (restores the step counter) and drop the graph, so
                                gid = e.graph_end()     # that the stream is usable again and the outer `finally`'s sync cannot mask the
                                if gid is not None:     # original error with "stream is capturing" 
                                    e.graph_destroy(gid)
                            except _lib.NifError:
                                pass
                if steps_per_epoch is not None:
                    pass
                elif use_graph and graph_id is not None:
                    if is_adam:
                        e.graph_launch(graph_id, adam)
                    else:
                        e.graph_launch_opt(graph_id, adam)
                else:
                    run_batches()
                tot, cnt = e.metric_read(reset=True)   # accumulated on the device: one host sync per epoch
                logs = {"loss": tot / max(cnt, 1.0)}
                logs.update({k: float(v) for k, v in self._metric_values(kinds, msum, mcnt[0]).items()})
                if validation_data is not None:
                    ev = self.evaluate(validation_data[0], validation_data[1],
                                       sample_weight=validation_data[2] if len(validation_data) == 3 else None)
                    if isinstance(ev, list):
                        logs["val_loss"] = ev[0]
                        logs.update({"val_" + k: v for (k, _), v in zip(kinds, ev[1:])})
                    else:
                        logs["val_loss"] = ev
                    self._push_losses(e, 1)       # evaluate() ends with _pop_losses: the next epoch trains with THIS model's loss / jac_reg again
                for cb in callbacks:
                    if hasattr(cb, "on_epoch_end"):
                        cb.on_epoch_end(epoch, logs)
                hist.epoch.append(epoch)          # Keras' History runs after the user callbacks: it records what they
                for k, v in logs.items():         # added to `logs` (LearningRateScheduler's 'lr')
                    hist.history.setdefault(k, []).append(v)
                if verbose:
                    print("Epoch %d/%d - %.2fs - loss: %.4e" % (epoch + 1, epochs, time.time() - t0, logs["loss"]))
        finally:
            self._pop_losses(e)
            if graph_id is not None:
                e.graph_destroy(graph_id)
            if shard is not None:
                shard.release(e)          # the slot's device buffers may be refilled once these steps have run
            e.sync()
            for arr in owned:
                arr.free()
        # Keras' fit: the weights become their average behind the last epoch, ahead of on_train_end; validation and metrics above saw
        # the current weights.  Not when no epoch ran, not when an exception ended the call
        if ema_of(self.optimizer) is not None and epochs > initial_epoch:
            self.optimizer.finalize_variable_values(self)
        for cb in callbacks:
            if hasattr(cb, "on_train_end"):
                cb.on_train_end({})
        self.history = hist
        return hist


class JacobianLayer(object):
    """reference nif/layers/gradient.py:4-49: `y, dys_dxs = JacobianLayer(model, y_index, x_index)(x)` with
    dys_dxs[a, i, j] = d y[a, y_index[i]] / d x[a, x_index[j]] w.r.t. the model *input vector* (parameter
    columns first, then coordinates).  Built as a forward-mode tangent HIP kernel for coordinate columns of
    the NIF / NIFMultiScale models (`k_jac`); the reference runs len(y_index) extra reverse sweeps."""

    def __init__(self, model, y_index, x_index, **kwargs):
        if not isinstance(model, Model) or model._role != "full":
            raise TypeError("JacobianLayer expects the model returned by NIF(...).build() / .model()")
        self.model = model
        self.y_index = [y_index] if isinstance(y_index, int) else list(y_index)
        self.x_index = [x_index] if isinstance(x_index, int) else list(x_index)

    def call(self, x, **kwargs):
        return self.model._engine.jacobian(x, self.y_index, self.x_index)

    __call__ = call


class HessianLayer(object):
    """reference nif/layers/gradient.py:130-180: `y, dys_dxs, dys2_dxs2 = HessianLayer(model, y_index, x_index)(x)` with
    dys2_dxs2[a, i, j, k] = d^2 y[a, y_index[i]] / d x[a, x_index[j]] d x[a, x_index[k]].  Second-order forward-mode
    tangents in one HIP kernel per coordinate pair (the reference nests two GradientTapes and batch_jacobian, :251-261);
    built for any input columns of all three classes."""

    def __init__(self, model, y_index, x_index, **kwargs):
        if not isinstance(model, Model) or model._role != "full":
            raise TypeError("HessianLayer expects the model returned by NIF(...).build() / .model()")
        self.model = model
        self.y_index = [y_index] if isinstance(y_index, int) else list(y_index)
        self.x_index = [x_index] if isinstance(x_index, int) else list(x_index)

    def call(self, x, **kwargs):
        return self.model._engine.hessian(x, self.y_index, self.x_index)

    __call__ = call


class SobolevModel(Model):
    """The Keras idiom  `tf.keras.Model(inp, JacobianLayer(nif_model, y_index, x_index)(inp))`  compiled with
    loss='mse' and loss_weights=[1, w]: a two-output model (u, du/dx) whose training differentiates through
    the Jacobian (reference nif/layers/gradient.py:36-49, SURVEY 3.4 / BASELINE config 5 "Sobolev training").
    Built for all three classes, any distinct outputs in y_index and any distinct input columns in x_index (coordinates and / or
    ParameterNet inputs, as gradient.py:207-231 allows; more than three columns run as passes over groups of three tangent streams),
    any positive loss_weights[0].
        m = SobolevModel(JacobianLayer(model, y_index, x_index)); m.compile("adam", "mse", loss_weights=[1, .1])
        m.fit(x, [y, dydx], ...);  u, dudx = m.predict(x)
    Over a HessianLayer it is the three-output model (u, du/dx, d2u/dx2) of gradient.py:130-180 compiled with loss_weights=[w0, w1, w2]:
        m = SobolevModel(HessianLayer(model, y_index, x_index)); m.compile("adam", "mse", loss_weights=[1, .1, .01])
        m.fit(x, [y, dydx, d2ydx2], ...);  u, dudx, d2udx2 = m.predict(x)
    built for NIFMultiScale (SIREN ShapeNet, with or without resblocks) and NIFMultiScaleLastLayerParameterized, coordinate columns in
    x_index, policy float32 (nif_sobolev2_loss_grad_dev: the first-order step plus one second-order pass per coordinate pair)."""

    _HESS_BUILT = ("built: NIFMultiScale (SIREN ShapeNet, with or without resblocks) and NIFMultiScaleLastLayerParameterized, "
                   "coordinate columns in x_index, policy float32")

    def __init__(self, jac_layer):
        if not isinstance(jac_layer, (JacobianLayer, HessianLayer)):
            raise TypeError("SobolevModel wraps a JacobianLayer or a HessianLayer")
        self._order = 2 if isinstance(jac_layer, HessianLayer) else 1
        base = jac_layer.model
        if self._order == 2:
            owner = base._owner
            if owner._spec.kind == "NIF":
                raise NotImplementedError("SobolevModel(HessianLayer(...)) of class NIF is not built (%s)" % self._HESS_BUILT)
            if owner.mixed_policy_name != "float32":
                raise NotImplementedError("SobolevModel(HessianLayer(...)) under mixed_policy=%r is not built (%s)"
                                          % (owner.mixed_policy_name, self._HESS_BUILT))
            if any(int(i) < owner._spec.pi_dim for i in jac_layer.x_index):
                raise NotImplementedError("SobolevModel(HessianLayer(...)) with parameter columns in x_index is not built (%s)"
                                          % self._HESS_BUILT)
        Model.__init__(self, base._owner, "full")
        so, ncol = base._owner._spec.so_dim, base._owner._spec.pi_dim + base._owner._spec.si_dim
        # any subset / order of outputs and input columns (gradient.py:207-231); a column or output listed twice would make the
        # reference build duplicated Jacobian entries -- not a training set-up, refused
        self.y_index = [int(i) for i in jac_layer.y_index]
        self.x_index = [int(i) for i in jac_layer.x_index]
        if len(set(self.y_index)) != len(self.y_index) or not all(0 <= i < so for i in self.y_index):
            raise ValueError("y_index: distinct outputs in [0, %d)" % so)
        if len(set(self.x_index)) != len(self.x_index) or not all(0 <= i < ncol for i in self.x_index):
            raise ValueError("x_index: distinct input columns in [0, %d)" % ncol)
        self._all_y = self.y_index == list(range(so))
        self.loss_weights = [1.0] * (1 + self._order)

    def compile(self, optimizer="adam", loss="mse", loss_weights=None, **kwargs):
        if isinstance(loss, (list, tuple)):
            if len(set(loss)) != 1:
                raise NotImplementedError("both outputs of the two-output model take the same loss")
            loss = loss[0]
        Model.compile(self, optimizer=optimizer, loss=loss, **kwargs)
        if loss_weights is not None:
            lw = [float(v) for v in loss_weights]
            if self._order == 2:
                if len(lw) != 3 or lw[0] <= 0.0 or lw[1] < 0.0 or lw[2] < 0.0:
                    raise ValueError("loss_weights = [w_u > 0, w_dudx >= 0, w_d2udx2 >= 0] (three outputs)")
            elif len(lw) != 2 or lw[0] <= 0.0:
                raise ValueError("loss_weights = [w_u > 0, w_dudx]")
            self.loss_weights = lw

    def fit_snapshots(self, *args, **kwargs):
        raise NotImplementedError("SobolevModel.fit_snapshots: the snapshot-wise step has no derivative outputs (fit() on the expanded "
                                  "table trains the two- and three-output models)")

    def select_sensors(self, *args, **kwargs):
        """Model.select_sensors of the wrapped model: the basis phi(x) has no derivative outputs to select on"""
        return Model.select_sensors(self, *args, **kwargs)

    def _run(self, x):
        if self._order == 2:      # HessianLayer(model, y_index, x_index)(x), the layer the model wraps
            return list(self._engine.hessian(x, self.y_index, self.x_index))
        u, j = self._engine.sobolev_forward(x, self.x_index)
        return [u, j if self._all_y else np.ascontiguousarray(j[:, self.y_index, :])]

    def _loss_host(self, e, x, targets, sw):
        """Model.evaluate's chunk loss for the two-output model: w0 mse(u) + w1 mse(du/dx) + the regularisation losses -- the
        same total `fit` logs (r3 returned the data term alone, computed on the host)"""
        if self._order == 2:
            w0, w1, w2 = self.loss_weights
            return e.sobolev2_loss_and_grad(x, targets[0], targets[1], targets[2], self.x_index, w1 / w0, w2 / w0,
                                            self._scaled_weights(sw, x.shape[0]), want_grad=False,
                                            y_index=None if self._all_y else self.y_index)[0]
        w0, w1 = self.loss_weights
        return e.sobolev_loss_and_grad(x, targets[0], targets[1], self.x_index, w1 / w0, self._scaled_weights(sw, x.shape[0]),
                                       want_grad=False, y_index=None if self._all_y else self.y_index)[0]

    def _targets(self, y, n_rows):
        if self._order == 2:
            if not (isinstance(y, (list, tuple)) and len(y) == 3):
                raise ValueError("the Sobolev model over a HessianLayer has three outputs: fit(x, [y, dydx, d2ydx2])")
            ty, tj = SobolevModel._targets_first(self, y[:2], n_rows)
            so, nx, ny = self._owner._spec.so_dim, len(self.x_index), len(self.y_index)
            th = np.ascontiguousarray(y[2], dtype=np.float32)
            if th.shape != (n_rows, ny, nx, nx):
                raise ValueError("d2ydx2 must have shape (N, len(y_index)=%d, len(x_index)=%d, %d), got %r" % (ny, nx, nx, th.shape))
            if not self._all_y:   # engine rows [so][nx][nx]: the listed outputs' blocks in place, the others unused (zeros)
                full = np.zeros((n_rows, so, nx, nx), dtype=np.float32)
                full[:, self.y_index] = th
                th = full
            return [ty, tj, th.reshape(n_rows, so * nx * nx)]
        if not (isinstance(y, (list, tuple)) and len(y) == 2):
            raise ValueError("the Sobolev model has two outputs: fit(x, [y, dydx])")
        return SobolevModel._targets_first(self, y, n_rows)

    def _targets_first(self, y, n_rows):
        so, nx, ny = self._owner._spec.so_dim, len(self.x_index), len(self.y_index)
        ty = Model._targets(self, y[0], n_rows)[0]
        tj = np.ascontiguousarray(y[1], dtype=np.float32).reshape(n_rows, ny, nx)
        if not self._all_y:       # the engine's table rows are [so][nx]: the listed outputs' rows in place, the others unused (zeros)
            full = np.zeros((n_rows, so, nx), dtype=np.float32)
            full[:, self.y_index, :] = tj
            tj = full
        return [ty, tj.reshape(n_rows, so * nx)]

    def _n_tangents(self):
        return 3 if self._order == 2 else len(self.x_index)     # (the second-order pair passes carry three tangent streams)

    def _scaled_weights(self, sw, n_rows):
        """Keras total loss = w0 mse(u) + w1 mse(du/dx) (+ regularisers, unscaled).  The kernels compute
        1/B sum_a sw_a (mse_a(u) + wj mse_a(du/dx)): w0 rides on the sample weights (sw_a <- w0 sw_a, a constant column when the
        caller gave none) and wj = w1 / w0 -- the data term and its gradient are scaled, the regularisation losses are not."""
        w0 = self.loss_weights[0]
        if w0 == 1.0:
            return sw
        if sw is None:
            return np.full((n_rows,), w0, dtype=np.float32)
        return np.ascontiguousarray(np.asarray(sw, dtype=np.float32) * np.float32(w0))

    def _loss_grad_dev(self, e, d_x, d_targets, d_sw, b, bg):
        if self._order == 2:
            w0, w1, w2 = self.loss_weights
            e.sobolev2_loss_grad_dev(d_x, d_targets[0], d_targets[1], d_targets[2], d_sw, b, bg, self.x_index, w1 / w0, w2 / w0,
                                     None if self._all_y else self.y_index)
            return
        w0, w1 = self.loss_weights
        e.sobolev_loss_grad_dev(d_x, d_targets[0], d_targets[1], d_sw, b, bg, self.x_index, w1 / w0,
                                None if self._all_y else self.y_index)


def _is_number(v):
    return isinstance(v, (float, int))        # the reference's test (model.py:109, :1031): True / False count as numbers there too


def shapenet_regularizer_coefficients(s_l1, s_l2, p_l1, p_l2):
    """(l1, l2) of the last-layer class's ShapeNet regulariser as the reference builds it (model.py:1031-1039)"""
    keras_default = 0.01
    if _is_number(s_l2):
        return (0.0, float(p_l2) if p_l2 is not None else keras_default)
    if _is_number(s_l1):
        return (float(p_l1) if p_l1 is not None else keras_default, 0.0)
    return (0.0, 0.0)


class NIF(object):
    """reference nif/model.py:48 `class NIF(object)`: a factory of Keras-like models that share one set
    of variables."""
    _KIND = "NIF"

    def __init__(self, cfg_shape_net, cfg_parameter_net, mixed_policy="float32"):
        self._spec = Spec(self._KIND, cfg_shape_net, cfg_parameter_net, mixed_policy)
        s = self._spec
        # attribute names of the reference (model.py:83-99)
        self.cfg_shape_net = cfg_shape_net
        self.cfg_parameter_net = cfg_parameter_net
        self.si_dim, self.so_dim, self.n_sx, self.l_sx = s.si_dim, s.so_dim, s.n_sx, s.l_sx
        self.pi_dim, self.pi_hidden, self.n_st, self.l_st = s.pi_dim, s.pi_hidden, s.n_st, s.l_st
        self.p_jac_reg = cfg_parameter_net.get("jac_reg", None)
        self.p_l1_reg = cfg_parameter_net.get("l1_reg", None)
        self.p_l2_reg = cfg_parameter_net.get("l2_reg", None)
        self.p_act_l1_reg = cfg_parameter_net.get("act_l1_reg", None)
        self.p_act_l2_reg = cfg_parameter_net.get("act_l2_reg", None)
        # activity regulariser of the ParameterNet output: L2 wins over L1 (model.py:118-125)
        self._act_reg = (0.0, 0.0)
        if isinstance(self.p_act_l2_reg, (float, int)):
            self._act_reg = (0.0, float(self.p_act_l2_reg))
        elif isinstance(self.p_act_l1_reg, (float, int)):
            self._act_reg = (float(self.p_act_l1_reg), 0.0)
        # kernel/bias regularisers of every ParameterNet layer: L2 wins over L1 (model.py:109-117)
        self._reg = (0.0, 0.0)
        if isinstance(self.p_l2_reg, (float, int)):
            self._reg = (0.0, float(self.p_l2_reg))
        elif isinstance(self.p_l1_reg, (float, int)):
            self._reg = (float(self.p_l1_reg), 0.0)
        # last-layer class only: cfg_shape_net['l2_reg' / 'l1_reg'] (model.py:1028-1039) -- read by the subclass constructor
        self._sreg = (0.0, 0.0)
        self.mixed_policy_name = mixed_policy
        self.variable_Dtype = "float32"
        self.compute_Dtype = {"mixed_bfloat16": "bfloat16", "mixed_float16": "float16"}.get(mixed_policy, "float32")
        self.po_dim = s.po_dim
        self.pnet_list = [nm for nm, _ in s.param_shapes() if nm.startswith("pnet_") and nm.endswith("_w")]
        self.__engine = None
        self._init_weights = s.initial_weights(_global_rng[0])

    @property
    def _engine(self):
        # the HIP context is created on first use (constructing the object needs no GPU, like the
        # reference's constructor needs no data)
        if self.__engine is None:
            self.__engine = Engine(self._spec, device_id=dist.local_device())
            self.__engine.set_weights(self._init_weights)
            if self._reg != (0.0, 0.0):
                self.__engine.set_regularizer(self._reg[0], self._reg[1], 0, self._n_pnet_params())
            if self._act_reg != (0.0, 0.0):
                self.__engine.set_activity_regularizer(*self._act_reg)
            if self._sreg != (0.0, 0.0):
                self.__engine.set_shapenet_regularizer(*self._sreg)
        return self.__engine

    def _n_pnet_params(self):
        return sum(int(np.prod(s)) for nm, s in self._spec.param_shapes() if nm.startswith("pnet_"))

    def call(self, inputs, training=None, mask=None):
        """model.py:130-154 / :510-539 / :1044-1068"""
        return self._engine.forward(inputs)

    def build(self):
        """model.py:345-377: with cfg_parameter_net['jac_reg'] the reference returns the model wrapped in JacRegLatentLayer
        (same outputs, + l1 * mean((d latent / d parameter)^2) in the loss); here the returned Model carries l1 and hands it to
        the engine when it trains or evaluates -- .model() and the sub-models stay without it, as in the reference."""
        l1 = float(self.p_jac_reg) if isinstance(self.p_jac_reg, (float, int)) and not isinstance(self.p_jac_reg, bool) else 0.0
        return Model(self, "full", jac_reg=l1)

    def model(self):
        """model.py:379-389"""
        return Model(self, "full")

    def model_p_to_w(self):
        """model.py:391-404"""
        return Model(self, "p_to_w")

    def model_p_to_lr(self):
        """model.py:406-420"""
        return Model(self, "p_to_lr")

    def model_lr_to_w(self):
        """model.py:422-433"""
        return Model(self, "lr_to_w")

    def model_x_to_u_given_w(self):
        """model.py:435-464 / :956-986"""
        return Model(self, "x_to_u_given_w", n_inputs=2)

    def save_config(self, filename="config.json"):
        """model.py:466-480"""
        config = {
            "cfg_shape_net": self.cfg_shape_net,
            "cfg_parameter_net": self.cfg_parameter_net,
            "mixed_policy": self.mixed_policy_name,
        }
        with open(filename, "w") as write_file:
            json.dump(config, write_file, indent=4)


class NIFMultiScale(NIF):
    """reference nif/model.py:483"""
    _KIND = "NIFMultiScale"


class NIFMultiScaleLastLayerParameterized(NIFMultiScale):
    """reference nif/model.py:989"""
    _KIND = "NIFMultiScaleLastLayerParameterized"

    def __init__(self, cfg_shape_net, cfg_parameter_net, mixed_policy="float32"):
        super(NIFMultiScaleLastLayerParameterized, self).__init__(cfg_shape_net, cfg_parameter_net, mixed_policy)
        # model.py:1028-1039: kernel AND bias regulariser of every layer of the shared ShapeNet (siren.py:266-269, :393-398).
        # WHICH one is chosen by cfg_shape_net's keys (L2 wins over L1); its COEFFICIENT is the reference's quirk: it passes
        # self.p_l2_reg / self.p_l1_reg -- cfg_parameter_net's number -- to regularizers.L2 / L1, and Keras 2.11 turns a None
        # there into its default 0.01 (keras/regularizers.py: `l2 = 0.01 if l2 is None else l2`).  Restated as is.
        self.s_l1_reg = cfg_shape_net.get("l1_reg", None)
        self.s_l2_reg = cfg_shape_net.get("l2_reg", None)
        self._sreg = shapenet_regularizer_coefficients(self.s_l1_reg, self.s_l2_reg, self.p_l1_reg, self.p_l2_reg)

    def model_lr_to_w(self):
        """model.py:1106-1115"""
        raise ValueError("In this class: NIFMultiScaleLastLayerParameterization, `w` is the same as `lr`")

    def model_x_to_phi(self):
        """model.py:1085-1104"""
        return Model(self, "x_to_phi")
