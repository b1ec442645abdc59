"""C-ABI call orders: the op alphabet, the lazy and the eager runner, the pair sweep, the seeded walks and the shrinker.

nif_ctx keeps lazy state between calls (a deferred row reduction, a loss-metric accumulation waiting for the next k_small launch, plane
images of theta, "already applied" markers).  Every entry point must run or invalidate the part it touches.  This module walks call
orders through nif_amd.engine.Engine and compares two runs of the same sequence:

  lazy    the ops back to back
  eager   observe() behind every op, which forces every deferred piece to run at once

Both must leave the same observables BIT FOR BIT (every sum of the library has a fixed order, fused forms equal unfused forms).  What
the eager run cannot see (a plane image that was not invalidated: reads do not repack) is anchored against the NumPy oracle, and the
metric sum against a float64 restatement of k_metric's expression.

An op is a named closure over a Ctx (an engine, its fixture of device buffers and the little Python-side bookkeeping an op needs, e.g. the
id of the last captured graph).  Nothing here imports torch; the GPU is only touched through the engine handed in."""
import ctypes as C
import itertools
from collections import OrderedDict

import numpy as np

from nif_amd import _lib
from nif_amd._lib import NifError

# ops that may differ between the runners in the last bits, with the cause (none: every op of the alphabet is bit-reproducible)
NOT_BITWISE = {}
LOSS_BAR, GRAD_BAR, FWD_BAR = 3e-6, 3e-5, 1e-5      # tests/test_gpu_tail.py's bars against the oracle

B_SMALL, B_TILE = 512, 4099                         # k_small's batch; a batch above NIF_SMALL_MAX_B (2048): the tile kernels
N_ROWS, N_W = 64, 8                                 # rows of the read-only inference ops; of those that carry a [rows, po] weight table
SET_FLAT_SCALE = np.float32(1.0 + 2.0 ** -10)
METRIC_W = 0.75

PREFIXES = OrderedDict([
    ("tile", ["loss_grad_tile"]),                                   # tail pending
    ("small_metric", ["loss_grad_a", "metric_accumulate"]),         # tail and metric pending
    ("capture", ["capture"]),                                       # recorded small steps, nothing run
    ("capture_replay", ["capture", "replay"]),
    ("reg_applied", ["set_regularizer_on", "loss_grad_a", "adam_step"]),
    ("gt_ran1", ["set_gt_clipvalue", "loss_grad_a", "grad_transform_dev"]),      # a transform without a norm stage ran
])
SMALL_PREFIXES = ("small_metric",)

# Kept out of the cartesian product, with the cause; swept behind every prefix against COMM_PARTNERS instead (comm_attach_sequences).
# ncclCommInitRank takes 0.3 s to seconds per call and ncclCommDestroy 0.25 s (measured on one MI355X, world 1): the 2 x 71 x 6 pairs
# that hold comm_attach, each on two contexts, would alone run for ten minutes per net.
SWEEP_EXCLUDED = {"comm_attach": "RCCL communicator construction and teardown cost about a second per sequence"}
COMM_PARTNERS = ("comm_selftest", "allreduce_grad")

# ops behind which theta, or the plane images the next step reads, changed: the oracle anchor follows them
THETA_OPS = ("set_flat", "adam_step", "lion_step", "adabelief_step", "replay", "replay_opt", "prune_apply", "flip_small_step",
             "flip_fuse_gw", "flip_fp32_mfma", "f64_round_into_model")


class GpuError(RuntimeError):
    """a HIP / RCCL error (not a refusal of the library): the sequence that met it is reported and never run again"""

    def __init__(self, op, message):
        RuntimeError.__init__(self, "%s: %s" % (op, message))
        self.op, self.message = op, message


def is_gpu_error(ex):
    s = str(ex)
    return s.startswith("libnif_hip error -2") or s.startswith("libnif_hip error -5")


# ---- the fixture and the context -------------------------------------------------------------------------------------------------
class Fixture(object):
    """device buffers of one engine: two small batches (the first one weighted), one tile-path batch, Sobolev targets of the first small
    batch, a prediction buffer, float64 copies for the double-precision closure; fixed optimizer structs"""

    def __init__(self, engine, spec, seed=20240):
        import nif_amd
        from nif_amd.optimizers import AdaBeliefOptimizer, Lion
        e = self.e = engine
        self.spec = spec
        ncol, so = spec.pi + spec.si, spec.so
        rng = np.random.default_rng(seed)

        def batch(b):
            return (rng.uniform(-1, 1, size=(b, ncol)).astype(np.float32), rng.uniform(-1, 1, size=(b, so)).astype(np.float32),
                    rng.uniform(0.5, 1.5, size=(b,)).astype(np.float32))
        self.host = {"a": batch(B_SMALL), "b": batch(B_SMALL), "t": batch(B_TILE)}
        self.dev = {}
        for k, (x, y, sw) in self.host.items():
            d = (e.alloc(x.size), e.alloc(y.size), e.alloc(sw.size))
            d[0].upload(x); d[1].upload(y); d[2].upload(sw)
            self.dev[k] = d
        self.x_index = [spec.pi]                                     # the first coordinate column
        g = rng.uniform(-1, 1, size=(B_SMALL, so, 1)).astype(np.float32)
        h = rng.uniform(-1, 1, size=(B_SMALL, so, 1, 1)).astype(np.float32)
        self.d_g, self.d_h = e.alloc(g.size), e.alloc(h.size)
        self.d_g.upload(g); self.d_h.upload(h)
        self.d_u = e.alloc(B_TILE * so)
        # the read-only inference entries: N_ROWS rows of batch a; a permutation for the device gather; a latent and a weight table
        es = e.spec
        self.d_hy, self.d_hd, self.d_h2 = e.alloc(N_ROWS * so), e.alloc(N_ROWS), e.alloc(N_ROWS)
        self.d_perm, self.d_gath = e.alloc(N_ROWS), e.alloc(N_ROWS * ncol)
        self.d_perm.upload(rng.permutation(N_ROWS).astype(np.int32).view(np.float32))
        self.d_lr, self.d_w = e.alloc(N_W * es.pi_hidden), e.alloc(N_W * es.po_dim)
        self.d_lr.upload(rng.uniform(-1, 1, size=(N_W * es.pi_hidden,)).astype(np.float32))
        self.d_w.upload(rng.uniform(-0.1, 0.1, size=(N_W * es.po_dim,)).astype(np.float32))
        self.d_xs, self.d_gu = e.alloc(N_W * es.si_dim), e.alloc(N_W * so)
        self.d_xs.upload(self.host["a"][0][:N_W, spec.pi:spec.pi + spec.si])
        self.theta0 = e.get_flat()
        self.zeros = np.zeros_like(self.theta0)
        self.adam = nif_amd.Adam(1e-3).as_struct()
        self.adam_opt = _lib.nif_opt()                               # the same Adam as a nif_opt (nif_opt_step_dev, nif_graph_launch_opt)
        self.adam_opt.kind = _lib.OPT_ADAM
        self.adam_opt.lr, self.adam_opt.beta1, self.adam_opt.beta2, self.adam_opt.eps = 1e-3, 0.9, 0.999, 1e-7
        self.lion = Lion().as_opt()
        self.adabelief = AdaBeliefOptimizer(amsgrad=True).as_opt()
        lay = e.layout()
        nm, off, rows, cols = max(lay, key=lambda t: t[2] * max(t[3], 1))      # the largest tensor: the pruned segment
        self.prune_seg = (off, rows * max(cols, 1))
        self.reg_range = (0, e.n_params)
        self.d64 = None
        self.caps = set()

    def grad_view(self):
        """[grad | loss] through the raw device pointer (nif_grad_dev runs the deferred reduction, adds no regulariser term)"""
        out = np.empty((self.e.n_params + 1,), dtype=np.float32)
        p = self.e.grad_dev_ptr()
        _check(self.e.lib.nif_d2h(self.e.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.size * 4))
        return out

    def alloc_f64(self):
        x, y, _ = self.host["a"]
        self.d64 = (self.e.alloc_f64(x.size), self.e.alloc_f64(y.size), self.e.alloc_f64(y.size))
        self.d64[0].upload(x.astype(np.float64)); self.d64[1].upload(y.astype(np.float64))


def _check(rc):
    _lib.check(rc)


class Ctx(object):
    """an engine, its fixture and the Python-side bookkeeping of the ops (a function of the op sequence alone: equal in both runners)"""

    def __init__(self, engine, fixture):
        self.e, self.fix = engine, fixture
        self.gid = None
        self.clear()

    def clear(self):
        self.reads = []            # what the read ops returned, as bytes
        self.reg_on = False        # a weight regulariser is set: nif_grad_read WRITES (adds the term), observe() then reads the raw buffer
        self.plain = True          # loss 'mse', no regulariser of any kind: the oracle's plain loss_and_grad is the reference
        self.flags = {"wreg": False, "sreg": False, "jac": False, "act": False, "mae": False}
        self.opts = {"fuse_tail": 1, "small_step": 1, "fuse_gw": 1, "fp32_mfma": 0}
        self.prune_on = False
        self.f64_set = False

    def flag(self, key, on):
        self.flags[key] = bool(on)
        self.reg_on = self.flags["wreg"] or self.flags["sreg"]
        self.plain = not any(self.flags.values())

    def read(self, *arrays):
        for a in arrays:
            self.reads.append(np.ascontiguousarray(a).tobytes())


def probe_caps(c):
    """which optional ops this net takes: tried once on the fresh context (a refusal is NIF_ERR_INVALID, nothing has run), then reset"""
    e, f = c.e, c.fix
    a = f.dev["a"]

    def takes(fn):
        try:
            fn()
            return True
        except NifError as ex:
            if is_gpu_error(ex):
                raise
            return False
    e.reserve(B_TILE + 29, 1)
    if takes(lambda: e.sobolev_loss_grad_dev(a[0].at(0), a[1].at(0), f.d_g.at(0), None, B_SMALL, B_SMALL, f.x_index, 0.5)):
        f.caps.add("sob")
    if takes(lambda: e.sobolev2_loss_grad_dev(a[0].at(0), a[1].at(0), f.d_g.at(0), f.d_h.at(0), None, B_SMALL, B_SMALL, f.x_index, 0.5, 0.25)):
        f.caps.add("sob2")
    if takes(lambda: e.f64_set_flat(f.theta0.astype(np.float64))):
        f.caps.add("f64")
        f.alloc_f64()
    if takes(lambda: e.set_shapenet_regularizer(0.0, 1e-3)):
        f.caps.add("sreg")

    def fp32():
        e.set_option("fp32_mfma", 1)
        try:
            t = f.dev["t"]
            e.loss_grad_dev(t[0].at(0), t[1].at(0), None, B_TILE, B_TILE)
            e.forward_dev(t[0].at(0), B_TILE, f.d_u.at(0))
        finally:
            e.set_option("fp32_mfma", 0)
    if takes(fp32):
        f.caps.add("fp32_mfma")
    # every step kind once, so that no later call (a capture least of all) has to grow a workspace
    for k, b in (("t", B_TILE), ("a", B_SMALL)):
        d = f.dev[k]
        e.loss_grad_dev(d[0].at(0), d[1].at(0), d[2].at(0), b, b)
    e.metric_accumulate(0.0)
    reset(c)
    return f.caps


def reset(c):
    """back to the state of a fresh context with theta0: what a sequence may have left behind is settled and cleared"""
    e, f = c.e, c.fix
    e.comm_destroy()
    if c.gid is not None:
        e.graph_destroy(c.gid)
        c.gid = None
    for k, v in (("fuse_tail", 1), ("small_step", 1), ("fuse_gw", 1), ("fp32_mfma", 0)):
        e.set_option(k, v)
    e.profile_enable(0)
    e.set_regularizer(0.0, 0.0, 0, 0)
    e.set_jac_regularizer(0.0)
    e.set_activity_regularizer(0.0, 0.0)
    e.set_shapenet_regularizer(0.0, 0.0)
    e.set_loss("mse")
    e.set_grad_transform(None)
    e.prune_config([], [])
    e.set_flat(f.theta0)
    e.set_opt_state(f.zeros, f.zeros, 0)
    e.set_opt_slot(2, f.zeros)
    e.zero_grad()
    e.set_grad_transform(global_clipnorm=1.0)      # the norms of the last transform are context state too: those of a zero gradient
    e.grad_transform_dev()
    e.set_grad_transform(None)
    e.metric_read(reset=True)
    if "f64" in f.caps:
        e.f64_set_flat(f.theta0.astype(np.float64))
    c.clear()


# ---- the alphabet ----------------------------------------------------------------------------------------------------------------
def _steps(A):
    def lg(key, b, weighted):
        def op(c):
            d = c.fix.dev[key]
            c.e.loss_grad_dev(d[0].at(0), d[1].at(0), d[2].at(0) if weighted else None, b, b)
        return op
    A["loss_grad_a"] = lg("a", B_SMALL, False)
    A["loss_grad_a_weighted"] = lg("a", B_SMALL, True)
    A["loss_grad_b"] = lg("b", B_SMALL, False)
    A["loss_grad_tile"] = lg("t", B_TILE, False)

    def sob(c):
        f, a = c.fix, c.fix.dev["a"]
        c.e.sobolev_loss_grad_dev(a[0].at(0), a[1].at(0), f.d_g.at(0), None, B_SMALL, B_SMALL, f.x_index, 0.5)

    def sob2(c):
        f, a = c.fix, c.fix.dev["a"]
        c.e.sobolev2_loss_grad_dev(a[0].at(0), a[1].at(0), f.d_g.at(0), f.d_h.at(0), None, B_SMALL, B_SMALL, f.x_index, 0.5, 0.25)
    A["sobolev_loss_grad"] = sob
    A["sobolev2_loss_grad"] = sob2
    A["adam_step"] = lambda c: c.e.adam_step_dev(c.fix.adam)
    A["lion_step"] = lambda c: c.e.opt_step_dev(c.fix.lion)
    A["adabelief_step"] = lambda c: c.e.opt_step_dev(c.fix.adabelief)
    A["zero_grad"] = lambda c: c.e.zero_grad()


def _reads(A):
    A["metric_accumulate"] = lambda c: c.e.metric_accumulate(METRIC_W)
    A["metric_read"] = lambda c: c.read(np.array(c.e.metric_read(reset=False)))
    A["metric_read_reset"] = lambda c: c.read(np.array(c.e.metric_read(reset=True)))

    def grad_read(c):
        loss, g = c.e.grad_read()
        c.read(np.float32(loss), g)
    A["grad_read"] = grad_read
    A["last_loss"] = lambda c: c.read(np.float32(c.e.last_loss()))
    A["grad_dev_ptr"] = lambda c: c.read(c.fix.grad_view())
    A["get_flat"] = lambda c: c.read(c.e.get_flat())
    A["set_flat"] = lambda c: c.e.set_flat(c.fix.theta0 * SET_FLAT_SCALE)

    def set_opt_state(c):
        t = c.fix.theta0
        c.e.set_opt_state(t * np.float32(0.125), np.abs(t) * np.float32(0.25), 7)
    A["set_opt_state"] = set_opt_state
    A["get_opt_slots"] = lambda c: c.read(*[c.e.get_opt_slot(i) for i in range(3)])

    def set_opt_slots(c):
        t = c.fix.theta0
        for i, s in enumerate((0.5, 0.03125, 0.0625)):
            c.e.set_opt_slot(i, np.abs(t) * np.float32(s) if i else t * np.float32(s))
    A["set_opt_slots"] = set_opt_slots

    def forward(c):
        f, t = c.fix, c.fix.dev["t"]
        c.e.forward_dev(t[0].at(0), B_TILE, f.d_u.at(0))
        c.read(f.d_u.download(B_TILE * f.spec.so))
    A["forward"] = forward


def _settings(A):
    def setter(name, key, fn_on, fn_off):
        def on(c):
            fn_on(c); c.flag(key, True)

        def off(c):
            fn_off(c); c.flag(key, False)
        A[name + "_on"], A[name + "_off"] = on, off
    setter("set_regularizer", "wreg", lambda c: c.e.set_regularizer(0.0, 0.5, *c.fix.reg_range), lambda c: c.e.set_regularizer(0.0, 0.0, 0, 0))
    setter("set_jac_regularizer", "jac", lambda c: c.e.set_jac_regularizer(0.01), lambda c: c.e.set_jac_regularizer(0.0))
    setter("set_activity_regularizer", "act", lambda c: c.e.set_activity_regularizer(0.0, 1e-3),
           lambda c: c.e.set_activity_regularizer(0.0, 0.0))

    def sreg(c):
        c.e.set_shapenet_regularizer(0.0, 1e-3); c.flag("sreg", True)
    A["set_shapenet_regularizer"] = sreg

    def loss(name):
        def op(c):
            c.e.set_loss(name); c.flag("mae", name == "mae")
        return op
    A["set_loss_mae"], A["set_loss_mse"] = loss("mae"), loss("mse")
    A["set_gt_global_clipnorm"] = lambda c: c.e.set_grad_transform(global_clipnorm=0.05)
    A["set_gt_clipvalue"] = lambda c: c.e.set_grad_transform(clipvalue=0.01)
    A["set_gt_none"] = lambda c: c.e.set_grad_transform(None)
    A["grad_transform_dev"] = lambda c: c.e.grad_transform_dev()

    def grad_norms(c):
        per, g = c.e.grad_norms()
        c.read(per, np.float32(g))
    A["grad_norms"] = grad_norms

    def prune_config_update(c):
        off, size = c.fix.prune_seg
        c.e.prune_config([off], [size])
        c.prune_on = True
        c.e.prune_update([max(1, size // 2)])
    A["prune_config_update"] = prune_config_update
    A["prune_apply"] = lambda c: c.e.prune_apply()

    def prune_state(c):
        masks, thr = c.e.get_prune_state()
        c.read(thr, *masks)
        c.e.set_prune_state(masks, thr)
    A["prune_state_round_trip"] = prune_state
    A["reserve"] = lambda c: c.e.reserve(2 * B_SMALL)

    def flip(key):
        def op(c):
            c.opts[key] ^= 1
            c.e.set_option(key, c.opts[key])
        return op
    for key in ("fuse_tail", "small_step", "fuse_gw", "fp32_mfma"):
        A["flip_" + key] = flip(key)
    A["profile_on"] = lambda c: c.e.profile_enable(1)
    A["profile_off"] = lambda c: c.e.profile_enable(0)


def _graphs_comm_f64(A):
    def capture(c):
        e, a = c.e, c.fix.dev["a"]
        e.graph_begin()
        try:
            for _ in range(2):
                e.loss_grad_dev(a[0].at(0), a[1].at(0), None, B_SMALL, B_SMALL)
                e.metric_accumulate(1.0)
                e.opt_step_dev(c.fix.adam_opt)
        except NifError:
            e.graph_destroy(e.graph_end())      # leave the capture; the half-recorded graph is dropped
            raise
        old, c.gid = c.gid, e.graph_end()
        if old is not None:
            e.graph_destroy(old)
    A["capture"] = capture

    def replay(c):
        if c.gid is not None:
            c.e.graph_launch(c.gid, c.fix.adam)

    def replay_opt(c):
        if c.gid is not None:
            c.e.graph_launch_opt(c.gid, c.fix.adam_opt)
    A["replay"], A["replay_opt"] = replay, replay_opt

    def graph_destroy(c):
        if c.gid is not None:
            c.e.graph_destroy(c.gid)
            c.gid = None
    A["graph_destroy"] = graph_destroy
    A["comm_attach"] = lambda c: c.e.comm_init_rank(c.e.comm_unique_id(), 0, 1)
    A["allreduce_grad"] = lambda c: c.e.allreduce_grad()
    A["comm_selftest"] = lambda c: c.read(np.int32(c.e.comm_selftest()))
    A["comm_destroy"] = lambda c: c.e.comm_destroy()

    def f64_set_flat(c):
        c.e.f64_set_flat(c.fix.theta0.astype(np.float64) * (1.0 + 2.0 ** -30))
        c.f64_set = True
    A["f64_set_flat"] = f64_set_flat

    def f64_loss_grad(c):
        d = c.fix.d64
        c.e.f64_loss_grad_dev(d[0].at(0), d[1].at(0), None, B_SMALL, B_SMALL)
        loss, g = c.e.f64_grad_read()
        c.read(np.float64(loss), g)
    A["f64_loss_grad_read"] = f64_loss_grad
    A["f64_forward"] = lambda c: c.read(c.e.f64_forward(c.fix.host["a"][0]))
    A["f64_round_into_model"] = lambda c: c.e.set_flat(c.e.f64_get_flat().astype(np.float32))


def _inference_and_plumbing(A):
    """read-only entry points: they run the deferred reduction, read theta or its plane images, and must leave everything else alone"""
    def rows(c):
        return c.fix.host["a"][0][:N_ROWS]

    def cols(c):
        return c.fix.spec.pi, c.fix.spec.si
    A["jacobian"] = lambda c: c.read(*c.e.jacobian(rows(c), [0], [c.fix.spec.pi]))

    def hessian_dev(c):
        f = c.fix
        c.e.hessian_dev(f.dev["a"][0].at(0), N_ROWS, [0], [f.spec.pi], f.d_hy.at(0), f.d_hd.at(0), f.d_h2.at(0))
        c.read(f.d_hy.download(), f.d_hd.download(), f.d_h2.download())
    A["hessian_dev"] = hessian_dev
    A["sobolev_forward"] = lambda c: c.read(*c.e.sobolev_forward(rows(c), c.fix.x_index))
    A["pnet_latent"] = lambda c: c.read(c.e.p_to_lr(rows(c)[:, :cols(c)[0]]))
    A["x_to_phi"] = lambda c: c.read(c.e.x_to_phi(rows(c)[:, cols(c)[0]:sum(cols(c))]))

    def latent_to_w_dev(c):
        f = c.fix
        _check(c.e.lib.nif_latent_to_w_dev(c.e.ctx, f.d_lr.at(0), N_W, f.d_w.at(0)))
        c.read(f.d_w.download())
    A["latent_to_w_dev"] = latent_to_w_dev

    def shapenet_given_w_dev(c):
        f = c.fix
        _check(c.e.lib.nif_shapenet_given_w_dev(c.e.ctx, f.d_xs.at(0), f.d_w.at(0), N_W, f.d_gu.at(0)))
        c.read(f.d_gu.download())
    A["shapenet_given_w_dev"] = shapenet_given_w_dev

    def gather_rows(c):
        f = c.fix
        c.e.gather_rows(f.dev["a"][0], f.d_perm, N_ROWS, f.spec.pi + f.spec.si, f.d_gath)
        c.read(f.d_gath.download())
    A["gather_rows"] = gather_rows

    def profile_read(c):      # the launch counts are state; the milliseconds are a measurement
        d = c.e.profile_read(reset=True)
        c.read(np.array([d[k][1] for k in _lib.PROF_NAMES], dtype=np.int64))
    A["profile_read"] = profile_read

    def sobolev_plain(c):      # nif_sobolev_loss_grad_dev, the entry without y_index
        f, a = c.fix, c.fix.dev["a"]
        xi = (C.c_int32 * 1)(f.x_index[0])
        _check(c.e.lib.nif_sobolev_loss_grad_dev(c.e.ctx, a[0].at(0), a[1].at(0), f.d_g.at(0), None, B_SMALL, B_SMALL, xi, 1, 0.5))
    A["sobolev_loss_grad_plain"] = sobolev_plain

    def debug_timeline(c):
        buf = (C.c_int64 * 8)()
        _check(c.e.lib.nif_debug_timeline(c.e.ctx, buf, 4))
    A["debug_timeline"] = debug_timeline

    def comm_plumbing(c):
        e, f = c.e, c.fix
        _check(e.lib.nif_comm_barrier(e.ctx))
        _check(e.lib.nif_comm_allreduce(e.ctx, f.d_gath.at(0), 4, _lib.DT_F32, _lib.OP_SUM))
        rank, world = C.c_int32(), C.c_int32()
        _check(e.lib.nif_comm_info(e.ctx, C.byref(rank), C.byref(world)))
        c.read(np.array([rank.value, world.value]), f.d_gath.download(4))
    A["comm_plumbing"] = comm_plumbing

    def memory_plumbing(c):
        """the allocation, copy, staging-slot and stopwatch primitives (each runs the deferred reduction first)"""
        e = c.e
        lib, ctx = e.lib, e.ctx
        host = np.arange(64, dtype=np.float32)
        back = np.empty_like(host)
        d, h = C.c_void_p(), C.c_void_p()
        _check(lib.nif_dev_alloc(ctx, 256, C.byref(d)))
        _check(lib.nif_host_alloc(ctx, 256, C.byref(h)))
        try:
            _check(lib.nif_h2d(ctx, d, host.ctypes.data_as(C.c_void_p), 256))
            C.memmove(h.value, host.ctypes.data, 256)
            _check(lib.nif_h2d_async(ctx, d, h, 256, 0))
            _check(lib.nif_copy_acquire(ctx, 0))
            _check(lib.nif_copy_release(ctx, 0))
            _check(lib.nif_copy_wait_host(ctx, 0))
            _check(lib.nif_d2h(ctx, back.ctypes.data_as(C.c_void_p), d, 256))
        finally:
            _check(lib.nif_host_free(ctx, h))
            _check(lib.nif_dev_free(ctx, d))
        e.timer_start()
        _check(lib.nif_sync(ctx))
        e.timer_stop()
        c.read(back, np.array([lib.nif_stream(ctx) == e.stream_ptr(), bool(lib.nif_params_dev(ctx))]))
    A["memory_plumbing"] = memory_plumbing

    def lifetime_and_info(c):
        """a second context of the same model comes and goes; the sizes and the layout of this one"""
        e = c.e
        cfg, other = e.spec.to_cfg(), C.c_void_p()
        _check(e.lib.nif_create(C.byref(cfg), 0, C.byref(other)))
        _check(e.lib.nif_destroy(other))
        n, po = C.c_int64(), C.c_int64()
        _check(e.lib.nif_param_count(e.ctx, C.byref(n)))
        _check(e.lib.nif_po_dim(e.ctx, C.byref(po)))
        c.read(np.array([n.value, po.value] + [v for t in e.layout() for v in t[1:]]))
    A["lifetime_and_info"] = lifetime_and_info


NEEDS = {"sobolev_loss_grad_plain": "sob", "sobolev_loss_grad": "sob", "sobolev2_loss_grad": "sob2", "set_shapenet_regularizer": "sreg", "flip_fp32_mfma": "fp32_mfma",
         "f64_set_flat": "f64", "f64_loss_grad_read": "f64", "f64_forward": "f64", "f64_round_into_model": "f64"}


def full_alphabet():
    A = OrderedDict()
    _steps(A); _reads(A); _settings(A); _graphs_comm_f64(A); _inference_and_plumbing(A)
    return A


def alphabet(caps):
    """the ops this net takes (caps: Fixture.caps of probe_caps)"""
    return OrderedDict((k, v) for k, v in full_alphabet().items() if NEEDS.get(k) is None or NEEDS[k] in caps)


# ---- observation -----------------------------------------------------------------------------------------------------------------
def observe(c):
    """forces every deferred piece to run and reads the state back: sync, [grad | loss], the metric, theta, the optimizer slots.
    [grad | loss] comes from nif_grad_read -- except while a weight regulariser is set: nif_grad_read then ADDS the term (once, and marks
    it applied), which is a write the lazy run does not make; the raw buffer behind nif_grad_dev is read instead."""
    e = c.e
    e.sync()
    if c.reg_on:
        gl = c.fix.grad_view()
    else:
        loss, g = e.grad_read()
        gl = np.concatenate([g, np.array([loss], dtype=np.float32)])
    msum, mcnt = e.metric_read(reset=False)
    m, v, step = e.get_opt_state()
    slots = [e.get_opt_slot(i) for i in range(3)]
    return OrderedDict([("theta", e.get_flat()), ("m", m), ("v", v), ("vhat", slots[2]), ("slot0", slots[0]), ("slot1", slots[1]),
                        ("step", np.int64(step)), ("grad_loss", gl), ("metric", np.array([msum, mcnt]))])


def observe_full(c):
    """observe() plus grad_norms, the prune state and the float64 master"""
    o = observe(c)
    e = c.e
    try:
        per, g = e.grad_norms()
        o["grad_norms"] = np.concatenate([per, np.array([g], dtype=np.float32)])
    except NifError as ex:
        if is_gpu_error(ex):
            raise GpuError("grad_norms", str(ex))
        o["grad_norms"] = np.frombuffer(str(ex).encode(), dtype=np.uint8)
    if c.prune_on:
        masks, thr = e.get_prune_state()
        o["prune"] = np.concatenate([thr] + list(masks))
    if c.f64_set:
        o["f64_master"] = e.f64_get_flat()
    return o


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def diff(oa, ob):
    """names of the observables that differ bit for bit (with the largest absolute difference where that means something)"""
    out = []
    for k in oa:
        if k not in ob or not same_bits(oa[k], ob[k]):
            d = ""
            if k in ob and oa[k].shape == ob[k].shape and oa[k].dtype.kind == "f":
                with np.errstate(all="ignore"):
                    d = " (max |d| %.3g)" % float(np.nanmax(np.abs(oa[k].astype(np.float64) - ob[k].astype(np.float64))))
            out.append(k + d)
    out += [k for k in ob if k not in oa]
    return out


# ---- the runners -----------------------------------------------------------------------------------------------------------------
def run_ops(c, ops, seq, eager, observe_fn=observe, after=None):
    """runs seq on c; returns (errors, observations behind every op -- eager only).  A refusal of the library is recorded by its message
    (an observable of its own); a HIP / RCCL error ends the run (GpuError).  after(c, index, name): the oracle anchor's hook."""
    errors, obs = [], []
    for i, name in enumerate(seq):
        try:
            ops[name](c)
        except NifError as ex:
            if is_gpu_error(ex):
                raise GpuError(name, str(ex))
            errors.append((name, str(ex)))
        if eager:
            obs.append(observe_fn(c))
        if after is not None:
            after(c, i, name)
    return errors, obs


def metric_tally(seq, obs0, obs):
    """float64 restatement of k_metric (acc[0] += (double) weight * (double) grad[P]; acc[1] += (double) weight) over the losses the eager
    runner observed: the loss in front of every metric_accumulate is the one its observation behind the previous op holds.  A replay
    accumulates inside the graph, where nothing can be observed: its contribution is the change the eager runner reads around it.  A
    change of the metric behind any other op is reported (third value)."""
    s = n = 0.0
    prev = obs0
    bad = []
    for name, o in zip(seq, obs):
        if name == "metric_accumulate":
            s += float(np.float32(METRIC_W)) * float(prev["grad_loss"][-1])
            n += float(np.float32(METRIC_W))
        elif name == "metric_read_reset":
            s = n = 0.0
        elif not same_bits(o["metric"], prev["metric"]):
            if name in ("replay", "replay_opt"):      # taken as observed
                s, n = float(o["metric"][0]), float(o["metric"][1])
            else:
                bad.append(name)
        prev = o
    return s, n, bad


def compare(cl, ce, ops, seq, reset_fn=reset, observe_fn=observe, full_fn=observe_full, midpoints=(), check_metric=True):
    """one sequence on the lazy context cl and the eager context ce (both reset first): None, or a string that says what differs"""
    reset_fn(ce)
    o0 = observe_fn(ce)
    err_e, obs = run_ops(ce, ops, seq, True, observe_fn)
    fin_e = full_fn(ce)
    reset_fn(cl)
    err_l, _ = run_ops(cl, ops, seq, False, observe_fn)
    fin_l = full_fn(cl)
    if err_l != err_e:
        return "errors differ: lazy %r, eager %r" % (err_l, err_e)
    d = diff(fin_l, fin_e)
    if d:
        return "lazy and eager differ in " + ", ".join(d)
    if cl.reads != ce.reads:
        bad = [i for i, (a, b) in enumerate(zip(cl.reads, ce.reads)) if a != b]
        return "read op results differ (read %s of the sequence)" % (bad[:3] if bad else "count")
    if check_metric:
        s, n, bad = metric_tally(seq, o0, obs)
        if bad:
            return "the metric changed behind %s, which accumulate nothing" % ", ".join(bad)
        got = fin_l["metric"]
        if not (got[0] == s and got[1] == n):
            return "metric (%r, %r) is not the tally of weight * loss (%r, %r)" % (float(got[0]), float(got[1]), s, n)
    for k in midpoints:
        reset_fn(cl)
        run_ops(cl, ops, seq[:k], False, observe_fn)
        d = diff(observe_fn(cl), obs[k - 1])
        if d:
            return "behind op %d (%s) lazy and eager differ in %s" % (k, seq[k - 1], ", ".join(d))
    return None


# ---- sequences -------------------------------------------------------------------------------------------------------------------
def sweep_names(names):
    return [n for n in names if n not in SWEEP_EXCLUDED]


def pair_sequences(names, prefixes=None):
    """every (prefix, X, Y) over the alphabet without SWEEP_EXCLUDED: prefix ops, then X, then Y"""
    names = sweep_names(names)
    for pname, pre in (prefixes or PREFIXES).items():
        for x, y in itertools.product(names, repeat=2):
            yield pname, x, y, list(pre) + [x, y]


def comm_attach_sequences(prefixes=None):
    """behind every prefix: comm_attach, then each op that reads or rewrites [grad | loss] through the communicator"""
    for pname, pre in (prefixes or PREFIXES).items():
        for y in COMM_PARTNERS:
            yield pname, "comm_attach", y, list(pre) + ["comm_attach", y]


def walk(names, seed, length=16):
    rng = np.random.default_rng(seed)
    names = list(names)
    return [names[int(i)] for i in rng.integers(0, len(names), size=length)]


def walk_midpoints(seed, length=16):
    rng = np.random.default_rng(seed + 7919)
    return sorted(int(k) for k in rng.choice(np.arange(1, length), size=2, replace=False))


def shrink(seq, outcome):
    """shortest failing subsequence by dropping one op at a time.  outcome(candidate) replays it on fresh contexts and returns None
    (passes), a string (mismatch) or raises GpuError.  Stops at the first candidate that meets a GPU error and reports it: a faulting
    sequence is never run twice.  Returns (sequence, what it fails with)."""
    seq = list(seq)
    what = outcome(seq)
    if what is None:
        return seq, None
    progress = True
    while progress and len(seq) > 1:
        progress = False
        for i in range(len(seq)):
            cand = seq[:i] + seq[i + 1:]
            try:
                w = outcome(cand)
            except GpuError as ex:
                return cand, "GPU error: %s" % ex
            if w is not None:
                seq, what, progress = cand, w, True
                break
    return seq, what


# ---- the oracle anchor -----------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def anchor(c, oracle):
    """behind a theta-changing op of the LAZY run: the next loss_grad and the next forward against the oracle at the theta the library
    reports (a plane image that missed its invalidation still holds the old theta).  Returns None or what is off."""
    O = oracle
    e, f = c.e, c.fix
    theta = e.get_flat()
    ws = O.unflatten(f.spec, theta.astype(np.float64))
    x, y, sw = f.host["t"]
    t = f.dev["t"]
    bad = []
    e.forward_dev(t[0].at(0), B_TILE, f.d_u.at(0))
    u = f.d_u.download(B_TILE * f.spec.so).reshape(B_TILE, f.spec.so)
    r = _rel(u, O.forward(f.spec, ws, x.astype(np.float64)))
    if not r < FWD_BAR:
        bad.append("forward rel-L2 %.3g" % r)
    if c.plain:
        for key, b in (("a", B_SMALL), ("t", B_TILE)):
            xx, yy, ss = f.host[key]
            d = f.dev[key]
            lref, gref = O.loss_and_grad(f.spec, ws, xx.astype(np.float64), yy.astype(np.float64), ss.astype(np.float64))
            gref = O.flatten(gref)
            e.loss_grad_dev(d[0].at(0), d[1].at(0), d[2].at(0), b, b)
            gl = f.grad_view()
            if not abs(gl[-1] - lref) <= LOSS_BAR * abs(lref):
                bad.append("loss (%s) %.9g, oracle %.9g" % (key, gl[-1], lref))
            rg = _rel(gl[:-1], gref)
            if not rg < GRAD_BAR:
                bad.append("gradient (%s) rel-L2 %.3g" % (key, rg))
    return "; ".join(bad) if bad else None


def anchor_sequences(names):
    """prefix + T for every theta-changing op T of the alphabet: the oracle anchor runs behind T"""
    for pname, pre in PREFIXES.items():
        for t in THETA_OPS:
            if t in names:
                yield pname, t, list(pre) + [t]
