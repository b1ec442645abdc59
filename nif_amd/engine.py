"""Engine: one libnif_hip context + the host-side conveniences around it (weights as a list of
NumPy arrays in Keras order, device-resident datasets, the train step)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class DeviceArray(object):
    """A float32 device buffer owned by an Engine (hipMalloc through the C-ABI)."""

    def __init__(self, engine, n_floats):
        self.engine = engine
        self.n = int(n_floats)
        p = C.c_void_p()
        check(engine.lib.nif_dev_alloc(engine.ctx, self.n * 4, C.byref(p)))
        self.ptr = p.value

    def at(self, float_offset):
        return C.c_void_p(self.ptr + 4 * int(float_offset))

    def upload(self, host, float_offset=0):
        host = _f32(host)
        assert host.size + float_offset <= self.n
        check(self.engine.lib.nif_h2d(self.engine.ctx, self.at(float_offset), ptr(host), host.size * 4))

    def download(self, n_floats=None, float_offset=0):
        n = self.n - float_offset if n_floats is None else int(n_floats)
        out = np.empty((n,), dtype=np.float32)
        check(self.engine.lib.nif_d2h(self.engine.ctx, ptr(out), self.at(float_offset), n * 4))
        return out

    def free(self):
        if self.ptr:
            self.engine.lib.nif_dev_free(self.engine.ctx, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceArray64(object):
    """A float64 device buffer owned by an Engine: inputs, targets, sample weights and predictions of the double-precision
    L-BFGS closure (Engine.f64_*)."""

    def __init__(self, engine, n_doubles):
        self.engine = engine
        self.n = int(n_doubles)
        p = C.c_void_p()
        check(engine.lib.nif_dev_alloc(engine.ctx, max(self.n, 1) * 8, C.byref(p)))
        self.ptr = p.value

    def at(self, double_offset):
        return C.c_void_p(self.ptr + 8 * int(double_offset))

    def upload(self, host, double_offset=0):
        host = np.ascontiguousarray(host, dtype=np.float64)
        assert host.size + double_offset <= self.n
        check(self.engine.lib.nif_h2d(self.engine.ctx, self.at(double_offset), ptr(host), host.size * 8))

    def download(self, n_doubles=None, double_offset=0):
        n = self.n - double_offset if n_doubles is None else int(n_doubles)
        out = np.empty((n,), dtype=np.float64)
        check(self.engine.lib.nif_d2h(self.engine.ctx, ptr(out), self.at(double_offset), n * 8))
        return out

    free = DeviceArray.free
    __del__ = DeviceArray.__del__


class PinnedArray(object):
    """page-locked host staging buffer (hipHostMalloc through the C-ABI), exposed as a float32 NumPy view"""

    def __init__(self, engine, n_floats):
        self.engine = engine
        self.n = int(n_floats)
        p = C.c_void_p()
        check(engine.lib.nif_host_alloc(engine.ctx, self.n * 4, C.byref(p)))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_float * max(self.n, 1)).from_address(self.ptr))[:self.n]

    def free(self):
        if self.ptr:
            self.array = None
            self.engine.lib.nif_host_free(self.engine.ctx, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SnapshotSamples(object):
    """Engine.snapshot_samples: coordinates, targets and weights of T snapshots, resident on the device"""

    def __init__(self, engine, x, y, w, offsets, t, m, n):
        self.engine, self.offsets, self.t, self.m, self.n = engine, offsets, int(t), int(m), int(n)
        self.d_x = self.d_y = self.d_w = None
        try:
            if n:
                self.d_x, self.d_y = DeviceArray(engine, x.size), DeviceArray(engine, y.size)
                self.d_x.upload(x); self.d_y.upload(y)
                if w is not None:
                    self.d_w = DeviceArray(engine, w.size)
                    self.d_w.upload(w)
        except Exception:
            self.free()
            raise

    def args(self, d_latents, d_s):
        """the nif_encode_args of one call on these samples"""
        a = _lib.nif_encode_args()
        a.abi_version, a.ctx, a.T, a.M = _lib.NIF_ENCODE_ABI_VERSION, self.engine.ctx, self.t, self.m
        a.latents, a.S_out = d_latents.at(0), d_s.at(0)
        a.x = self.d_x.at(0) if self.d_x else None
        a.y = self.d_y.at(0) if self.d_y else None
        a.w = self.d_w.at(0) if self.d_w else None
        if self.offsets is not None:
            a.offsets_host = self.offsets.ctypes.data_as(C.POINTER(C.c_int64))
        return a

    def free(self):
        for d in (self.d_x, self.d_y, self.d_w):
            if d is not None:
                d.free()
        self.d_x = self.d_y = self.d_w = None


class Engine(object):
    def __init__(self, spec, device_id=0):
        self.spec = spec
        self.lib = _lib.load()
        if self.lib.nif_device_count() <= 0:
            raise _lib.NifError("no HIP device visible: nif_amd runs on MI355X (gfx950) only, there is no CPU path")
        cfg = spec.to_cfg()
        ctx = C.c_void_p()
        check(self.lib.nif_create(C.byref(cfg), int(device_id), C.byref(ctx)))
        self.ctx = ctx
        n = C.c_int64()
        check(self.lib.nif_param_count(self.ctx, C.byref(n)))
        self.n_params = int(n.value)
        assert self.n_params == spec.n_params(), (self.n_params, spec.n_params())
        self.shapes = spec.param_shapes()

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.nif_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc(self, n_floats):
        """float32 device buffer on this context's GPU"""
        return DeviceArray(self, n_floats)

    def alloc_pinned(self, n_floats):
        return PinnedArray(self, n_floats)

    def gather_rows(self, src, d_perm, n, ncol, dst):
        """dst[i][:] = src[perm[i]][:] on the device (perm: int32 bit patterns in a DeviceArray)"""
        check(self.lib.nif_gather_rows_dev(self.ctx, src.at(0), d_perm.at(0), int(n), int(ncol), dst.at(0)))

    # shard streaming (include/nif_hip.h: nif_h2d_async / nif_copy_*)
    def h2d_async(self, dst, pinned, n_floats, slot):
        check(self.lib.nif_h2d_async(self.ctx, dst.at(0), C.c_void_p(pinned.ptr), int(n_floats) * 4, int(slot)))

    def copy_acquire(self, slot):
        check(self.lib.nif_copy_acquire(self.ctx, int(slot)))

    def copy_release(self, slot):
        check(self.lib.nif_copy_release(self.ctx, int(slot)))

    def copy_wait_host(self, slot):
        check(self.lib.nif_copy_wait_host(self.ctx, int(slot)))

    # ---- parameters -----------------------------------------------------------------------------
    def layout(self):
        n = C.c_int32(0)
        check(self.lib.nif_param_layout(self.ctx, None, C.byref(n)))
        descs = (_lib.nif_tensor_desc * n.value)()
        check(self.lib.nif_param_layout(self.ctx, descs, C.byref(n)))
        return [(d.name.decode(), int(d.offset), int(d.rows), int(d.cols)) for d in descs]

    def set_weights(self, weights):
        if len(weights) != len(self.shapes):
            raise ValueError("You called `set_weights(weights)` with a weight list of length %d, but the model "
                             "was expecting %d weights." % (len(weights), len(self.shapes)))
        for w, (nm, s) in zip(weights, self.shapes):
            if tuple(np.shape(w)) != tuple(s):
                raise ValueError("Layer weight shape %s not compatible with provided weight shape %s (%s)"
                                 % (tuple(s), tuple(np.shape(w)), nm))
        flat = np.concatenate([_f32(w).ravel() for w in weights])
        self.set_flat(flat)

    def set_flat(self, flat):
        flat = _f32(flat)
        check(self.lib.nif_set_params(self.ctx, ptr(flat), flat.size))

    def get_flat(self):
        out = np.empty((self.n_params,), dtype=np.float32)
        check(self.lib.nif_get_params(self.ctx, ptr(out), out.size))
        return out

    def get_weights(self):
        flat = self.get_flat()
        out, off = [], 0
        for _, s in self.shapes:
            k = int(np.prod(s))
            out.append(flat[off:off + k].reshape(s).copy())
            off += k
        return out

    def get_opt_state(self):
        m = np.empty((self.n_params,), dtype=np.float32)
        v = np.empty((self.n_params,), dtype=np.float32)
        step = C.c_int64()
        check(self.lib.nif_get_opt_state(self.ctx, ptr(m), ptr(v), m.size, C.byref(step)))
        return m, v, int(step.value)

    def set_opt_state(self, m, v, step):
        m, v = _f32(m), _f32(v)
        check(self.lib.nif_set_opt_state(self.ctx, ptr(m), ptr(v), m.size, int(step)))

    # ---- inference ------------------------------------------------------------------------------
    @staticmethod
    def _rows(a, ncol, what, allow_extra=False):
        """float32 C-contiguous [B, ncol] view of a caller array.  The C side copies B*ncol floats unconditionally, so
        the column count is checked here.  allow_extra: full-model inputs may carry more columns, the model reads the
        first pi+si (reference model.py:142-143 slices `inputs[:, :pi+si]`)."""
        x = np.asarray(a, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] < ncol or (x.shape[1] != ncol and not allow_extra):
            raise ValueError("%s: expected shape (batch, %d), got %s" % (what, ncol, x.shape))
        if x.shape[1] != ncol:
            x = x[:, :ncol]
        return np.ascontiguousarray(x)

    def _inputs(self, a):
        return self._rows(a, self.spec.pi_dim + self.spec.si_dim, "inputs", allow_extra=True)

    def forward(self, inputs):
        x = self._inputs(inputs)
        s = self.spec
        out = np.empty((x.shape[0], s.so_dim), dtype=np.float32)
        if x.shape[0]:
            check(self.lib.nif_forward(self.ctx, ptr(x), x.shape[0], ptr(out)))
        return out

    def forward_dev(self, d_x, b, d_u):
        """predictions of device-resident rows [b, pi+si] into a device buffer [b, so] (nif_forward_dev); asynchronous"""
        check(self.lib.nif_forward_dev(self.ctx, d_x, int(b), d_u))

    # ---- snapshot-wise inference (include/nif_hip_snapshots.h; Model.predict_snapshots plans the chunks) ----------
    def _not_capturing(self, who="nif_forward_snapshots"):
        # nif_forward_snapshots* and nif_snapshot_normal_eq* refuse a capture themselves (NIF_ERR_STATE); the staging around them
        # (allocations, synchronous copies) would break the capture before they are reached
        if getattr(self, "_capturing", False):
            raise _lib.NifError("libnif_hip error -4: %s: not capturable (inside nif_graph_begin / nif_graph_end)" % who)

    def snapshot_mesh(self, x):
        """a shared mesh [M, si] uploaded once: the handle that forward_snapshots reads slices of (free() it when done)"""
        self._not_capturing()
        x = self._rows(x, self.spec.si_dim, "coordinates")
        d = DeviceArray(self, max(x.size, 1))
        d.upload(x)
        return d

    # The three pieces every snapshot call below is made of.  A mesh reaches an entry as (d_x, x_off, offsets, m, n): the device
    # array of the coordinates and the float offset into it, the ragged offsets [T + 1] (else None, with m points per snapshot),
    # n points in all.
    def _snapshot_call(self, uploads, shapes, call, dtype=np.float32):
        """The device round trip of one call: the row arrays `uploads` side by side in one device array d_r; call(d_r, outs) ->
        the entry's return code, outs the device addresses of the outputs of `shapes`, side by side in another; the outputs back
        as NumPy arrays.  A first output without elements (no points, or no snapshots) makes no call"""
        outs = [np.empty(s, dtype=dtype) for s in shapes]
        if not outs[0].size:
            return outs
        at = [0]
        for o in outs:
            at.append(at[-1] + o.size)
        d_r = DeviceArray(self, sum(a.size for a in uploads))
        d_o = (DeviceArray64 if dtype == np.float64 else DeviceArray)(self, at[-1])
        try:
            d_r.upload(np.concatenate([a.ravel() for a in uploads]))
            check(call(d_r, [d_o.at(i) for i in at[:-1]]))
            for o, i in zip(outs, at):
                check(self.lib.nif_d2h(self.ctx, ptr(o), d_o.at(i), o.nbytes))
        finally:
            d_r.free(); d_o.free()
        return outs

    def _ragged(self, who, name, rows, xs, run):
        """T coordinate arrays [M_t, si] concatenated on the device: run(d_x, 0, offsets, 0, n)"""
        self._not_capturing(who)
        xs = [self._rows(a, self.spec.si_dim, "coordinates") for a in xs]
        if len(xs) != int(np.shape(rows)[0]):
            raise ValueError("%s: %d rows for %d meshes" % (name, int(np.shape(rows)[0]), len(xs)))
        offsets = np.concatenate([[0], np.cumsum([a.shape[0] for a in xs])]).astype(np.int64)
        n = int(offsets[-1])
        d_x = DeviceArray(self, n * self.spec.si_dim) if n else None      # (no points: no call reads it)
        try:
            if n:
                d_x.upload(np.concatenate(xs, axis=0))
            return run(d_x, 0, offsets, 0, n)
        finally:
            if n:
                d_x.free()

    def _shared(self, rows, mesh, lo, hi, run):
        """the points lo .. hi of a snapshot_mesh handle: run(mesh, x_off, None, m, n), every output [n, ...] back as [T, hi - lo, ...]"""
        t, m = int(np.shape(rows)[0]), int(hi) - int(lo)
        return tuple(o.reshape((t, m) + o.shape[1:]) for o in run(mesh, int(lo) * self.spec.si_dim, None, m, t * m))

    def _snapshot_rows(self, rows, is_latent):
        return self._rows(rows, self.spec.pi_hidden if is_latent else self.spec.pi_dim, "latent" if is_latent else "parameter inputs")

    @staticmethod
    def _snapshot_geometry(a, d_r, rows, is_latent, d_x, x_off, off, m, yi):
        """the members that nif_snapderiv_args and nif_snapparam_args share"""
        a.rows, a.rows_are_latent, a.T = d_r.at(0), 1 if is_latent else 0, rows.shape[0]
        a.x, a.M = d_x.at(x_off), int(m)
        a.offsets_host = None if off is None else off.ctypes.data_as(C.POINTER(C.c_int64))
        a.y_idx, a.ny = yi.ctypes.data_as(C.POINTER(C.c_int32)), yi.size

    def _snapshots(self, rows, is_latent, d_x, x_off, offsets, m, n):
        self._not_capturing()
        rows = self._snapshot_rows(rows, is_latent)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        return self._snapshot_call([rows], [(n, self.spec.so_dim)], lambda d_r, o: self.lib.nif_forward_snapshots_dev(
            self.ctx, d_r.at(0), 1 if is_latent else 0, rows.shape[0], d_x.at(x_off),
            None if off is None else off.ctypes.data_as(C.POINTER(C.c_int64)), int(m), o[0]))

    def forward_snapshots(self, rows, is_latent, mesh, lo, hi):
        """rows [T, pi] (or [T, r] latents) on the points lo .. hi of a snapshot_mesh handle -> [T, hi - lo, so]"""
        return self._shared(rows, mesh, lo, hi, lambda *g: self._snapshots(rows, is_latent, *g))[0]

    def forward_snapshots_ragged(self, rows, is_latent, xs):
        """rows [T, .] and T coordinate arrays [M_t, si] (M_t = 0 allowed) -> [sum M_t, so], snapshot after snapshot"""
        return self._ragged("nif_forward_snapshots", "forward_snapshots_ragged", rows, xs, lambda *g: self._snapshots(rows, is_latent, *g))[0]

    # ---- snapshot-wise derivatives (include/nif_hip_snapderiv.h; Model.predict_snapshot_derivatives plans the chunks) ----------
    def _snapshot_derivs(self, rows, is_latent, d_x, x_off, offsets, m, n, y_index, x_index, order):
        self._not_capturing("nif_snapshot_derivatives")
        rows = self._snapshot_rows(rows, is_latent)
        yi = np.ascontiguousarray(list(y_index), dtype=np.int32)
        xi = np.ascontiguousarray(list(x_index), dtype=np.int32)
        ny, nx = yi.size, xi.size
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)

        def call(d_r, o):
            a = _lib.nif_snapderiv_args()
            a.abi_version, a.order, a.ctx = _lib.NIF_SNAPDERIV_ABI_VERSION, int(order), self.ctx
            self._snapshot_geometry(a, d_r, rows, is_latent, d_x, x_off, off, m, yi)
            a.x_idx, a.nx = xi.ctypes.data_as(C.POINTER(C.c_int32)), nx
            a.u, a.dudx, a.d2udx2 = o[0], o[1], (o[2] if order == 2 else None)
            return self.lib.nif_snapshot_derivatives_dev(C.byref(a))
        return tuple(self._snapshot_call([rows], [(n, self.spec.so_dim), (n, ny, nx)] + ([(n, ny, nx, nx)] if order == 2 else []), call))

    def snapshot_derivatives(self, rows, is_latent, mesh, lo, hi, y_index, x_index, order):
        """rows [T, pi] (or [T, r] latents) on the points lo .. hi of a snapshot_mesh handle -> (u [T, hi - lo, so],
        dudx [T, hi - lo, ny, nx][, d2udx2 [T, hi - lo, ny, nx, nx]]); x_index counts coordinates from 0"""
        return self._shared(rows, mesh, lo, hi, lambda *g: self._snapshot_derivs(rows, is_latent, *g, y_index, x_index, order))

    def snapshot_derivatives_ragged(self, rows, is_latent, xs, y_index, x_index, order):
        """rows [T, .] and T coordinate arrays [M_t, si] (M_t = 0 allowed) -> the same outputs [sum M_t, ...], snapshot after snapshot"""
        return self._ragged("nif_snapshot_derivatives", "snapshot_derivatives_ragged", rows, xs,
                            lambda *g: self._snapshot_derivs(rows, is_latent, *g, y_index, x_index, order))

    # ---- snapshot-wise parameter derivatives (include/nif_hip_snapparam.h; Model.predict_snapshot_parameter_derivatives plans the chunks) ----
    def _snapshot_param_derivs(self, rows, drows, d_x, x_off, offsets, m, n, y_index, p_index):
        self._not_capturing("nif_snapshot_param_derivatives")
        s = self.spec
        is_latent = drows is not None
        rows = self._snapshot_rows(rows, is_latent)
        yi = np.ascontiguousarray(list(y_index), dtype=np.int32)
        if is_latent:
            drows = np.ascontiguousarray(drows, dtype=np.float32)
            if drows.ndim != 3 or drows.shape[0] != rows.shape[0] or drows.shape[2] != s.pi_hidden:
                raise ValueError("dlatent: expected shape (%d, nd, %d), got %s" % (rows.shape[0], s.pi_hidden, drows.shape))
            pi_, nd = None, drows.shape[1]
        else:
            pi_ = np.ascontiguousarray(list(p_index), dtype=np.int32)
            nd = pi_.size
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)

        def call(d_r, o):
            a = _lib.nif_snapparam_args()
            a.abi_version, a.ctx = _lib.NIF_SNAPPARAM_ABI_VERSION, self.ctx
            self._snapshot_geometry(a, d_r, rows, is_latent, d_x, x_off, off, m, yi)
            if is_latent:
                a.drows, a.nd = d_r.at(rows.size), nd
            else:
                a.p_idx, a.np = pi_.ctypes.data_as(C.POINTER(C.c_int32)), nd
            a.u, a.dudp = o
            return self.lib.nif_snapshot_param_derivatives_dev(C.byref(a))
        return tuple(self._snapshot_call([rows, drows] if is_latent else [rows], [(n, s.so_dim), (n, yi.size, nd)], call))

    def snapshot_param_derivatives(self, rows, drows, mesh, lo, hi, y_index, p_index):
        """rows [T, pi] with p_index (drows None), or latents [T, r] with directions drows [T, nd, r], on the points lo .. hi of a
        snapshot_mesh handle -> (u [T, hi - lo, so], dudp [T, hi - lo, ny, nd])"""
        return self._shared(rows, mesh, lo, hi, lambda *g: self._snapshot_param_derivs(rows, drows, *g, y_index, p_index))

    def snapshot_param_derivatives_ragged(self, rows, drows, xs, y_index, p_index):
        """rows [T, .] (and drows) and T coordinate arrays [M_t, si] (M_t = 0 allowed) -> the same outputs [sum M_t, ...], snapshot after snapshot"""
        return self._ragged("nif_snapshot_param_derivatives", "snapshot_param_derivatives_ragged", rows, xs,
                            lambda *g: self._snapshot_param_derivs(rows, drows, *g, y_index, p_index))

    # ---- their second order (include/nif_hip_snapparam2.h; Model.predict_snapshot_parameter_derivatives(order=2) plans the chunks) ----
    def _snapshot_param_second_derivs(self, rows, drows, ddrows, d_x, x_off, offsets, m, n, y_index, p_index, x_index):
        self._not_capturing("nif_snapshot_param_second_derivatives")
        s = self.spec
        is_latent = drows is not None
        rows = self._snapshot_rows(rows, is_latent)
        yi = np.ascontiguousarray(list(y_index), dtype=np.int32)
        xi = np.ascontiguousarray(list(x_index or []), dtype=np.int32)
        if is_latent:
            drows = np.ascontiguousarray(drows, dtype=np.float32)
            if drows.ndim != 3 or drows.shape[0] != rows.shape[0] or drows.shape[2] != s.pi_hidden:
                raise ValueError("dlatent: expected shape (%d, nd, %d), got %s" % (rows.shape[0], s.pi_hidden, drows.shape))
            pi_, nd = None, drows.shape[1]
            if ddrows is not None:
                ddrows = np.ascontiguousarray(ddrows, dtype=np.float32)
                if ddrows.shape != (rows.shape[0], nd, nd, s.pi_hidden):
                    raise ValueError("d2latent: expected shape (%d, %d, %d, %d), got %s" % (rows.shape[0], nd, nd, s.pi_hidden, ddrows.shape))
        else:
            pi_ = np.ascontiguousarray(list(p_index), dtype=np.int32)
            nd, ddrows = pi_.size, None
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        ny, nxc = yi.size, xi.size

        def call(d_r, o):
            a = _lib.nif_snapparam2_args()
            a.abi_version, a.ctx = _lib.NIF_SNAPPARAM2_ABI_VERSION, self.ctx
            self._snapshot_geometry(a, d_r, rows, is_latent, d_x, x_off, off, m, yi)
            if is_latent:
                a.drows, a.nd = d_r.at(rows.size), nd
                if ddrows is not None:
                    a.ddrows = d_r.at(rows.size + drows.size)
            else:
                a.p_idx, a.np = pi_.ctypes.data_as(C.POINTER(C.c_int32)), nd
            a.u, a.dudp, a.d2udp2 = o[0], o[1], o[2]
            if nxc:
                a.x_idx, a.nxc = xi.ctypes.data_as(C.POINTER(C.c_int32)), nxc
                a.dudx, a.d2udpdx = o[3], o[4]
            return self.lib.nif_snapshot_param_second_derivatives_dev(C.byref(a))
        uploads = [rows] + ([drows] if is_latent else []) + ([ddrows] if ddrows is not None else [])
        shapes = [(n, s.so_dim), (n, ny, nd), (n, ny, nd, nd)] + ([(n, ny, nxc), (n, ny, nd, nxc)] if nxc else [])
        return tuple(self._snapshot_call(uploads, shapes, call))

    def snapshot_param_second_derivatives(self, rows, drows, ddrows, mesh, lo, hi, y_index, p_index, x_index):
        """rows [T, pi] with p_index (drows, ddrows None), or latents [T, r] with directions drows [T, nd, r] and second directions
        ddrows [T, nd, nd, r] (or None), on the points lo .. hi of a snapshot_mesh handle -> (u [T, hi - lo, so],
        dudp [T, hi - lo, ny, nd], d2udp2 [T, hi - lo, ny, nd, nd][, dudx [T, hi - lo, ny, nx], d2udpdx [T, hi - lo, ny, nd, nx]]), the
        last two with a non-empty x_index (coordinates from 0)"""
        return self._shared(rows, mesh, lo, hi,
                            lambda *g: self._snapshot_param_second_derivs(rows, drows, ddrows, *g, y_index, p_index, x_index))

    def snapshot_param_second_derivatives_ragged(self, rows, drows, ddrows, xs, y_index, p_index, x_index):
        """rows [T, .] (and drows, ddrows) and T coordinate arrays [M_t, si] (M_t = 0 allowed) -> the same outputs [sum M_t, ...],
        snapshot after snapshot"""
        return self._ragged("nif_snapshot_param_second_derivatives", "snapshot_param_second_derivatives_ragged", rows, xs,
                            lambda *g: self._snapshot_param_second_derivs(rows, drows, ddrows, *g, y_index, p_index, x_index))

    # ---- encoding (include/nif_hip_encode.h; nif_amd/encode.py runs the Levenberg-Marquardt loop around these two) ----------
    def snapshot_samples(self, x, y, w=None, counts=None):
        """The samples of T snapshots on the device, uploaded once for all snapshot_normal_eq calls of one encode.  counts None: a
        shared mesh x [M, si] with y [T, M, so] (w [T, M]); else counts [T] (zeros allowed) with x [sum, si], y [sum, so] (w [sum])
        concatenated snapshot after snapshot.  free() it when done"""
        self._not_capturing("nif_snapshot_normal_eq")
        s = self.spec
        x = self._rows(x, s.si_dim, "coordinates")
        if counts is None:
            y = np.ascontiguousarray(y, dtype=np.float32)
            if y.ndim != 3 or y.shape[1:] != (x.shape[0], s.so_dim):
                raise ValueError("snapshot_samples: expected targets of shape (T, %d, %d), got %s" % (x.shape[0], s.so_dim, y.shape))
            t, m, n, offsets = y.shape[0], x.shape[0], y.shape[0] * x.shape[0], None
        else:
            counts = np.asarray(counts, dtype=np.int64)
            offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            t, m, n = counts.size, 0, int(offsets[-1])
            y = self._rows(y, s.so_dim, "targets")
            if x.shape[0] != n or y.shape[0] != n:
                raise ValueError("snapshot_samples: %d coordinates and %d targets for %d points" % (x.shape[0], y.shape[0], n))
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float32)
            if w.size != n:
                raise ValueError("snapshot_samples: %d weights for %d points" % (w.size, n))
        return SnapshotSamples(self, x, y, w, offsets, t, m, n)

    def snapshot_normal_eq(self, latents, samples):
        """latents [T, r] -> float64 [T, r + 1, r + 1]: every snapshot's Gram matrix of the augmented rows [du/dz, u - y] at its
        latent (A = J^T W J | g = J^T W e | c = sum w |e|^2), one device pass (nif_snapshot_normal_eq_dev)"""
        self._not_capturing("nif_snapshot_normal_eq")
        r = self.spec.pi_hidden
        lat = self._rows(latents, r, "latent")
        if lat.shape[0] != samples.t:
            raise ValueError("snapshot_normal_eq: %d latents for %d snapshots" % (lat.shape[0], samples.t))
        def call(d_l, o):
            a = samples.args(d_l, d_l)
            a.S_out = o[0]      # (args() reads arrays; the output is an address here)
            return self.lib.nif_snapshot_normal_eq_dev(C.byref(a))
        return self._snapshot_call([lat], [(samples.t, r + 1, r + 1)], call, dtype=np.float64)[0]

    def p_to_lr(self, p):
        p = self._rows(p, self.spec.pi_dim, "parameter inputs")
        out = np.empty((p.shape[0], self.spec.pi_hidden), dtype=np.float32)
        if p.shape[0]:
            check(self.lib.nif_pnet_latent(self.ctx, ptr(p), p.shape[0], ptr(out)))
        return out

    def jacobian(self, inputs, y_index, x_index):
        y_index, x_index = list(y_index), list(x_index)
        if len(set(y_index)) != len(y_index) or len(set(x_index)) != len(x_index):
            # repeated entries (gradient.py:207-231 would simply repeat rows / columns): computed once, gathered
            uy, ux = sorted(set(y_index)), sorted(set(x_index))
            yv, d = self.jacobian(inputs, uy, ux)
            return yv, np.ascontiguousarray(d[:, [uy.index(i) for i in y_index]][:, :, [ux.index(j) for j in x_index]])
        x = self._inputs(inputs)
        s = self.spec
        yi = np.ascontiguousarray(list(y_index), dtype=np.int32)
        xi = np.ascontiguousarray(list(x_index), dtype=np.int32)
        y = np.empty((x.shape[0], s.so_dim), dtype=np.float32)
        d = np.empty((x.shape[0], yi.size, xi.size), dtype=np.float32)
        check(self.lib.nif_jacobian(self.ctx, ptr(x), x.shape[0], yi.ctypes.data_as(C.POINTER(C.c_int32)), yi.size,
                                    xi.ctypes.data_as(C.POINTER(C.c_int32)), xi.size, ptr(y), ptr(d)))
        return y, d

    def hessian(self, inputs, y_index, x_index):
        y_index, x_index = list(y_index), list(x_index)
        if len(set(y_index)) != len(y_index) or len(set(x_index)) != len(x_index):
            uy, ux = sorted(set(y_index)), sorted(set(x_index))       # (also lifts the C side's limit of 16 y_index entries)
            yv, d, h = self.hessian(inputs, uy, ux)
            iy, ix = [uy.index(i) for i in y_index], [ux.index(j) for j in x_index]
            return yv, np.ascontiguousarray(d[:, iy][:, :, ix]), np.ascontiguousarray(h[:, iy][:, :, ix][:, :, :, ix])
        x = self._inputs(inputs)
        s = self.spec
        yi = np.ascontiguousarray(list(y_index), dtype=np.int32)
        xi = np.ascontiguousarray(list(x_index), dtype=np.int32)
        y = np.empty((x.shape[0], s.so_dim), dtype=np.float32)
        d = np.empty((x.shape[0], yi.size, xi.size), dtype=np.float32)
        h = np.empty((x.shape[0], yi.size, xi.size, xi.size), dtype=np.float32)
        check(self.lib.nif_hessian(self.ctx, ptr(x), x.shape[0], yi.ctypes.data_as(C.POINTER(C.c_int32)), yi.size,
                                   xi.ctypes.data_as(C.POINTER(C.c_int32)), xi.size, ptr(y), ptr(d), ptr(h)))
        return y, d, h

    def hessian_dev(self, d_x, b, y_index, x_index, d_y, d_dydx, d_d2):
        """HessianLayer on device-resident inputs / outputs (nif_hessian_dev): [b, pi+si] -> y [b, so], dydx [b, ny, nx],
        d2 [b, ny, nx, nx]; asynchronous on the context's stream"""
        yi = np.ascontiguousarray(list(y_index), dtype=np.int32)
        xi = np.ascontiguousarray(list(x_index), dtype=np.int32)
        check(self.lib.nif_hessian_dev(self.ctx, d_x, int(b), yi.ctypes.data_as(C.POINTER(C.c_int32)), yi.size,
                                       xi.ctypes.data_as(C.POINTER(C.c_int32)), xi.size, d_y, d_dydx, d_d2))

    def x_to_phi(self, x):
        x = self._rows(x, self.spec.si_dim, "coordinates")
        s = self.spec
        out = np.empty((x.shape[0], s.so_dim, s.pi_hidden), dtype=np.float32)
        if x.shape[0]:
            check(self.lib.nif_x_to_phi(self.ctx, ptr(x), x.shape[0], ptr(out)))
        return out

    def lr_to_w(self, lr):
        lr = self._rows(lr, self.spec.pi_hidden, "latent")
        out = np.empty((lr.shape[0], self.spec.po_dim), dtype=np.float32)
        if lr.shape[0]:
            check(self.lib.nif_latent_to_w(self.ctx, ptr(lr), lr.shape[0], ptr(out)))
        return out

    def x_to_u_given_w(self, x, w):
        x, w = self._rows(x, self.spec.si_dim, "coordinates"), _f32(w)
        if w.shape != (x.shape[0], self.spec.po_dim):
            raise ValueError("expected w of shape (%d, %d), got %s" % (x.shape[0], self.spec.po_dim, w.shape))
        out = np.empty((x.shape[0], self.spec.so_dim), dtype=np.float32)
        if x.shape[0]:
            check(self.lib.nif_shapenet_given_w(self.ctx, ptr(x), ptr(w), x.shape[0], ptr(out)))
        return out

    # ---- training -------------------------------------------------------------------------------
    def _targets(self, y, n_rows):
        y = _f32(y)
        if y.ndim == 1:
            y = y[:, None]
        if y.shape != (n_rows, self.spec.so_dim):
            raise ValueError("targets: expected shape (%d, %d), got %s" % (n_rows, self.spec.so_dim, y.shape))
        return y

    def _weights(self, sw, n_rows):
        if sw is None:
            return None
        sw = _f32(sw).reshape(-1)
        if sw.shape != (n_rows,):
            raise ValueError("sample_weight: expected shape (%d,), got %s" % (n_rows, sw.shape))
        return sw

    def loss_and_grad(self, inputs, y, sample_weight=None, want_grad=True):
        """(total loss, flat gradient); want_grad=False: (total loss, None) -- only the scalar travels back (evaluation)"""
        x = self._inputs(inputs)
        y = self._targets(y, x.shape[0])
        sw = self._weights(sample_weight, x.shape[0])
        g = np.empty((self.n_params,), dtype=np.float32) if want_grad else None
        loss = C.c_float()
        check(self.lib.nif_loss_and_grad(self.ctx, ptr(x), ptr(y), ptr(sw), x.shape[0], C.byref(loss), ptr(g)))
        return float(loss.value), g

    def train_step(self, inputs, y, sample_weight, adam):
        x = self._inputs(inputs)
        y = self._targets(y, x.shape[0])
        sw = self._weights(sample_weight, x.shape[0])
        loss = C.c_float()
        check(self.lib.nif_train_step(self.ctx, ptr(x), ptr(y), ptr(sw), x.shape[0], C.byref(adam), C.byref(loss)))
        return float(loss.value)

    # device-pointer flavour (datasets resident in HBM; optional cross-rank gradient all-reduce)
    def loss_grad_dev(self, d_x, d_y, d_sw, b_local, b_global):
        check(self.lib.nif_loss_grad_dev(self.ctx, d_x, d_y, d_sw, int(b_local), int(b_global)))

    # snapshot-wise step of the last-layer class (include/nif_hip_snapfit.h; Model.fit_snapshots plans the steps)
    def _snapfit_args(self, p, t, x, m, y, sw, batch_global):
        a = _lib.nif_snapfit_args()
        a.abi_version, a.ctx, a.T, a.M, a.batch_global = _lib.NIF_SNAPFIT_ABI_VERSION, self.ctx, int(t), int(m), int(batch_global)
        a.p, a.x, a.y, a.sw = p, x, y, sw
        return a

    def snapshot_loss_grad_dev(self, d_p, t, d_x, m, d_y, d_sw, batch_global=0):
        """[grad | loss] of nif_loss_grad_dev on the table [repeat(p, M) | tile(x, T)], from device pointers p [T, pi], x [M, si],
        y [T, M, so], sw [T, M] or None; batch_global 0 = T M.  Leaves the result where loss_grad_dev leaves it"""
        a = self._snapfit_args(d_p, t, d_x, m, d_y, d_sw, batch_global)
        check(self.lib.nif_snapshot_loss_grad_dev(C.byref(a)))

    def snapshot_loss_grad(self, p, x, y, sample_weight=None, batch_global=0, want_grad=True):
        """host arrays p [T, pi], x [M, si], y [T, M, so], sample_weight [T, M] or None -> (total loss, flat gradient)"""
        s = self.spec
        p = self._rows(p, s.pi_dim, "parameter inputs")
        x = self._rows(x, s.si_dim, "coordinates")
        t, m = p.shape[0], x.shape[0]
        y = _f32(y)
        if y.shape == (t, m) and s.so_dim == 1:
            y = y[:, :, None]
        if y.shape != (t, m, s.so_dim):
            raise ValueError("snapshot_loss_grad: expected targets of shape (%d, %d, %d), got %s" % (t, m, s.so_dim, y.shape))
        sw = None
        if sample_weight is not None:
            sw = _f32(sample_weight)
            if sw.shape != (t, m):
                raise ValueError("snapshot_loss_grad: expected sample_weight of shape (%d, %d), got %s" % (t, m, sw.shape))
        a = self._snapfit_args(ptr(p), t, ptr(x), m, ptr(y), ptr(sw), batch_global)
        check(self.lib.nif_snapshot_loss_grad(C.byref(a)))
        if not want_grad:
            return self.grad_read_loss(), None
        return self.grad_read()

    # sensor placement on the last-layer class's basis (include/nif_hip_sensors.h; Model.select_sensors cuts the result at the rank)
    def _sensors_args(self, x, m, mask, k, pivots, diag):
        a = _lib.nif_sensors_args()
        a.abi_version, a.ctx, a.M, a.K = _lib.NIF_SENSORS_ABI_VERSION, self.ctx, int(m), int(k)
        a.x, a.mask, a.pivots_out, a.diag_out = x, mask, pivots, diag
        return a

    def select_sensors_dev(self, d_x, m, d_mask, k, d_pivots, d_diag):
        """greedy pivoted QR of phi(x)^T from device pointers x [m, si], mask [m] bytes or None -> pivots [k] int64, diag [k] float32;
        asynchronous on the context's stream"""
        self._not_capturing("nif_select_sensors")
        a = self._sensors_args(d_x, m, d_mask, k, d_pivots, d_diag)
        check(self.lib.nif_select_sensors_dev(C.byref(a)))

    def select_sensors(self, x, n_sensors, mask=None):
        """host arrays x [M, si], mask [M] (nonzero = a sensor can stand there) or None -> (pivots [K] int64: rows m * so + s of
        model_x_to_phi(x) reshaped [M so, r], -1 from the step that found none; diag [K] float32)"""
        self._not_capturing("nif_select_sensors")
        x = self._rows(x, self.spec.si_dim, "coordinates")
        m, k = x.shape[0], int(n_sensors)
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            if mk.shape != (m,):
                raise ValueError("select_sensors: expected mask of shape (%d,), got %s" % (m, mk.shape))
        piv, diag = np.full((max(k, 0),), -1, dtype=np.int64), np.zeros((max(k, 0),), dtype=np.float32)
        a = self._sensors_args(ptr(x), m, ptr(mk), k, ptr(piv), ptr(diag))
        check(self.lib.nif_select_sensors(C.byref(a)))
        return piv, diag

    # Sobolev (two-output model u, du/dx; include/nif_hip.h nif_sobolev_*)
    def sobolev_loss_grad_dev(self, d_x, d_y, d_g, d_sw, b_local, b_global, x_index, w_jac, y_index=None):
        """y_index = None: the derivative term over every output; else over the listed outputs (d_g rows stay [so][nx])"""
        xi = (C.c_int32 * len(x_index))(*[int(i) for i in x_index])
        yi = None if y_index is None else (C.c_int32 * len(y_index))(*[int(i) for i in y_index])
        check(self.lib.nif_sobolev_loss_grad_dev_y(self.ctx, d_x, d_y, d_g, d_sw, int(b_local), int(b_global), xi, len(x_index),
                                                   yi, 0 if y_index is None else len(y_index), float(w_jac)))

    def sobolev2_loss_grad_dev(self, d_x, d_y, d_g, d_h, d_sw, b_local, b_global, x_index, w_jac, w_hess, y_index=None):
        """the three-output model's step (u, du/dx, d2u/dx2; nif_sobolev2_loss_grad_dev): d_g rows [so][nx], d_h rows [so][nx][nx]"""
        xi = (C.c_int32 * len(x_index))(*[int(i) for i in x_index])
        yi = None if y_index is None else (C.c_int32 * len(y_index))(*[int(i) for i in y_index])
        check(self.lib.nif_sobolev2_loss_grad_dev(self.ctx, d_x, d_y, d_g, d_h, d_sw, int(b_local), int(b_global), xi, len(x_index),
                                                  yi, 0 if y_index is None else len(y_index), float(w_jac), float(w_hess)))

    def sobolev2_loss_and_grad(self, inputs, y, dydx, d2ydx2, x_index, w_jac, w_hess, sample_weight=None, want_grad=True,
                               y_index=None):
        """(total loss incl. the weight regularisers, flat gradient) of the three-output model on host arrays"""
        x = self._inputs(inputs)
        B, so, nx = x.shape[0], self.spec.so_dim, len(x_index)
        y, g, h = self._targets(y, B), _f32(dydx), _f32(d2ydx2)
        if g.size != B * so * nx or h.size != B * so * nx * nx:
            raise ValueError("dydx / d2ydx2: expected %d x %d x %d (x %d) values, got shapes %s, %s" % (B, so, nx, nx, g.shape, h.shape))
        sample_weight = self._weights(sample_weight, B)
        d_x, d_y, d_g, d_h = DeviceArray(self, x.size), DeviceArray(self, y.size), DeviceArray(self, g.size), DeviceArray(self, h.size)
        d_sw = DeviceArray(self, B) if sample_weight is not None else None
        try:
            d_x.upload(x); d_y.upload(y); d_g.upload(g); d_h.upload(h)
            if d_sw is not None:
                d_sw.upload(_f32(sample_weight))
            self.sobolev2_loss_grad_dev(d_x.at(0), d_y.at(0), d_g.at(0), d_h.at(0), d_sw.at(0) if d_sw is not None else None, B, B,
                                        x_index, w_jac, w_hess, y_index)
            if want_grad:
                loss, grad = self.grad_read()
            else:
                loss, grad = self.grad_read_loss(), None
        finally:
            d_x.free(); d_y.free(); d_g.free(); d_h.free()
            if d_sw is not None:
                d_sw.free()
        return loss, grad

    def sobolev_forward(self, inputs, x_index):
        x = self._inputs(inputs)
        B, nx, so = x.shape[0], len(x_index), self.spec.so_dim
        xi = (C.c_int32 * nx)(*[int(i) for i in x_index])
        d_x, d_u, d_j = DeviceArray(self, x.size), DeviceArray(self, B * so), DeviceArray(self, B * so * nx)
        try:
            d_x.upload(x)
            check(self.lib.nif_sobolev_forward_dev(self.ctx, d_x.at(0), B, xi, nx, d_u.at(0), d_j.at(0)))
            u = d_u.download().reshape(B, so)
            j = d_j.download().reshape(B, so, nx)
        finally:
            d_x.free(); d_u.free(); d_j.free()
        return u, j

    def sobolev_loss_and_grad(self, inputs, y, dydx, x_index, w_jac, sample_weight=None, want_grad=True, y_index=None):
        """(total loss incl. the weight regularisers, flat gradient) of the two-output model on host arrays"""
        x = self._inputs(inputs)
        B = x.shape[0]
        y, g = self._targets(y, B), _f32(dydx)
        if g.size != B * self.spec.so_dim * len(x_index):
            raise ValueError("dydx: expected %d x %d x %d values, got shape %s" % (B, self.spec.so_dim, len(x_index), g.shape))
        sample_weight = self._weights(sample_weight, B)
        d_x, d_y, d_g = DeviceArray(self, x.size), DeviceArray(self, y.size), DeviceArray(self, g.size)
        d_sw = DeviceArray(self, B) if sample_weight is not None else None
        try:
            d_x.upload(x); d_y.upload(y); d_g.upload(g)
            if d_sw is not None:
                d_sw.upload(_f32(sample_weight))
            self.sobolev_loss_grad_dev(d_x.at(0), d_y.at(0), d_g.at(0), d_sw.at(0) if d_sw is not None else None, B, B,
                                       x_index, w_jac, y_index)
            if want_grad:
                loss, grad = self.grad_read()           # adds the kernel / bias regularisers once, like nif_loss_and_grad
            else:
                loss, grad = self.grad_read_loss(), None
        finally:
            d_x.free(); d_y.free(); d_g.free()
            if d_sw is not None:
                d_sw.free()
        return loss, grad

    def adam_step_dev(self, adam):
        check(self.lib.nif_adam_step_dev(self.ctx, C.byref(adam)))

    # Lion / AdaBelief (include/nif_hip.h nif_opt_*): `opt` is a _lib.nif_opt (optimizers.Lion / AdaBeliefOptimizer .as_opt())
    def opt_step_dev(self, opt):
        check(self.lib.nif_opt_step_dev(self.ctx, C.byref(opt)))

    def graph_launch_opt(self, gid, opt):
        check(self.lib.nif_graph_launch_opt(self.ctx, int(gid), C.byref(opt)))

    def get_opt_slot(self, slot):
        """slot 0 m, 1 v, 2 vhat (zeros before AMSGrad first used it), 3 the weight average of set_ema (zeros before it exists)"""
        out = np.empty((self.n_params,), dtype=np.float32)
        check(self.lib.nif_get_opt_slot(self.ctx, int(slot), ptr(out), out.size))
        return out

    def set_opt_slot(self, slot, values):
        values = _f32(values)
        check(self.lib.nif_set_opt_slot(self.ctx, int(slot), ptr(values), values.size))

    # Keras' use_ema behind every optimizer step of this context (nif_set_option "ema_momentum_bits" / "ema"; k_opt.hip)
    def set_ema(self, momentum=None, overwrite_frequency=None):
        """momentum None: off.  Else every optimizer step of any kind also updates average = momentum average + (1 - momentum) theta
        (slot 3; created as a copy of theta at the first such step), and with overwrite_frequency f >= 1 every f-th step writes the
        average back over theta.  Context state until set again: Model.fit sets it from its optimizer and clears it when it returns."""
        if momentum is None:
            self.set_option("ema", 0)
            return
        f = -1 if overwrite_frequency is None else int(overwrite_frequency)
        if f < 1 and overwrite_frequency is not None:
            raise ValueError("set_ema(overwrite_frequency=%r): None or an integer >= 1" % (overwrite_frequency,))
        self.set_option("ema_momentum_bits", int(np.array([momentum], dtype=np.float32).view(np.int32)[0]))
        self.set_option("ema", f)

    # gradient transform in front of every optimizer step (include/nif_hip.h nif_set_grad_transform; k_gradtf.hip)
    def set_grad_transform(self, spec=None, **kwargs):
        """spec: None (off) or a dict / keywords of centralize, gtcf (bool), clipnorm, clipvalue, global_clipnorm (None or 0 = off).
        Context state until set again: Model.fit sets it from its optimizer and clears it when it returns."""
        spec = dict(spec or {}, **kwargs)
        unknown = set(spec) - {"centralize", "gtcf", "clipnorm", "clipvalue", "global_clipnorm"}
        if unknown:
            raise TypeError("set_grad_transform(%s): unknown keyword" % ", ".join(sorted(unknown)))
        if not spec:
            check(self.lib.nif_set_grad_transform(self.ctx, None))
            return
        t = _lib.nif_grad_transform()
        t.flags = (_lib.GT_CENTRALIZE if spec.get("centralize") else 0) | (_lib.GT_GTCF if spec.get("gtcf") else 0)
        t.clipnorm = float(spec.get("clipnorm") or 0.0)
        t.clipvalue = float(spec.get("clipvalue") or 0.0)
        t.global_clipnorm = float(spec.get("global_clipnorm") or 0.0)
        check(self.lib.nif_set_grad_transform(self.ctx, C.byref(t)))

    def grad_transform_dev(self):
        """the configured transform once on the [grad | loss] buffer (for callers with their own update)"""
        check(self.lib.nif_grad_transform_dev(self.ctx))

    def grad_norms(self):
        """(per-tensor norms in layout order, global norm) of the last transform: the gradient in front of its norm stage"""
        n = len(self.layout())
        per = np.empty((n,), dtype=np.float32)
        g = C.c_float()
        check(self.lib.nif_grad_norms(self.ctx, ptr(per), n, C.byref(g)))
        return per, float(g.value)

    # low-magnitude pruning (include/nif_hip.h nif_prune_*; nif_amd.sparsity drives these)
    def prune_config(self, offsets, sizes):
        """register the pruned tensors as segments of theta (float offsets, sizes); empty lists: pruning off"""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        assert off.shape == sz.shape
        i64 = C.POINTER(C.c_int64)
        check(self.lib.nif_prune_config(self.ctx, int(off.size), off.ctypes.data_as(i64), sz.ctypes.data_as(i64)))
        self._prune_sizes = [int(v) for v in sz]

    def prune_update(self, ks):
        """masks of the current weights: per segment keep the k largest |w| (ties keep more)"""
        k = np.ascontiguousarray(ks, dtype=np.int64)
        if k.size != len(getattr(self, "_prune_sizes", [])):
            raise ValueError("prune_update: one k per configured segment")
        check(self.lib.nif_prune_update(self.ctx, k.ctypes.data_as(C.POINTER(C.c_int64))))

    def prune_apply(self):
        check(self.lib.nif_prune_apply(self.ctx))

    def get_prune_state(self):
        """(list of float32 0 / 1 masks, one per segment, float32 thresholds)"""
        sizes = getattr(self, "_prune_sizes", [])
        masks = np.empty((sum(sizes),), dtype=np.float32)
        thr = np.empty((len(sizes),), dtype=np.float32)
        check(self.lib.nif_get_prune_state(self.ctx, ptr(masks), masks.size, ptr(thr), thr.size))
        return np.split(masks, np.cumsum(sizes)[:-1]), thr

    def set_prune_state(self, masks, thresholds):
        flat = np.concatenate([_f32(mk).ravel() for mk in masks]) if len(masks) else np.zeros((0,), dtype=np.float32)
        thr = _f32(thresholds)
        check(self.lib.nif_set_prune_state(self.ctx, ptr(flat), flat.size, ptr(thr), thr.size))

    # captured training steps (include/nif_hip.h nif_graph_*)
    def graph_begin(self):
        check(self.lib.nif_graph_begin(self.ctx))
        self._capturing = True

    def graph_end(self):
        gid = C.c_int32(-1)
        self._capturing = False      # (the library leaves the capture whether or not it could be ended)
        check(self.lib.nif_graph_end(self.ctx, C.byref(gid)))
        return int(gid.value)

    def graph_launch(self, gid, adam):
        check(self.lib.nif_graph_launch(self.ctx, int(gid), C.byref(adam)))

    def graph_destroy(self, gid):
        check(self.lib.nif_graph_destroy(self.ctx, int(gid)))

    def zero_grad(self):
        check(self.lib.nif_zero_grad(self.ctx))

    def reserve(self, b_max, n_tangents=0):
        check(self.lib.nif_reserve(self.ctx, int(b_max), int(n_tangents)))

    def allreduce_grad(self):
        check(self.lib.nif_allreduce_grad(self.ctx))

    # the communicator of this context (include/nif_hip.h "multi-GPU"; nif_amd.distributed.RcclComm carries the id between processes)
    def comm_unique_id(self):
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        check(self.lib.nif_comm_unique_id(buf))
        return buf.raw

    def comm_init_rank(self, uid, rank, world):
        check(self.lib.nif_comm_init_rank(self.ctx, C.create_string_buffer(uid, _lib.COMM_ID_BYTES), int(rank), int(world)))

    def comm_selftest(self):
        n = C.c_int32()
        check(self.lib.nif_comm_selftest(self.ctx, C.byref(n)))
        return int(n.value)

    def comm_destroy(self):
        check(self.lib.nif_comm_destroy(self.ctx))

    def set_regularizer(self, l1, l2, lo, hi):
        check(self.lib.nif_set_regularizer(self.ctx, float(l1), float(l2), int(lo), int(hi)))

    def set_shapenet_regularizer(self, l1, l2):
        """last-layer class: cfg_shape_net l1_reg / l2_reg over the shared ShapeNet's kernels and biases (model.py:1028-1039)"""
        check(self.lib.nif_set_shapenet_regularizer(self.ctx, float(l1), float(l2)))

    def set_loss(self, name):
        """compile(loss=name): 'mse' | 'mae' | 'huber' | 'log_cosh' (and Keras' aliases)"""
        check(self.lib.nif_set_loss(self.ctx, int(_lib.LOSS_IDS[name])))

    def set_jac_regularizer(self, l1):
        check(self.lib.nif_set_jac_regularizer(self.ctx, float(l1)))

    def set_activity_regularizer(self, l1, l2):
        check(self.lib.nif_set_activity_regularizer(self.ctx, float(l1), float(l2)))

    def metric_accumulate(self, weight):
        check(self.lib.nif_metric_accumulate(self.ctx, float(weight)))

    def metric_read(self, reset=True):
        s, n = C.c_double(), C.c_double()
        check(self.lib.nif_metric_read(self.ctx, C.byref(s), C.byref(n), 1 if reset else 0))
        return float(s.value), float(n.value)

    # ---- the L-BFGS closure in double precision (include/nif_hip.h nif_f64_*; k_f64.hip) -------------------------------------
    # A precision of the fine-tuner, not a model policy: a float64 master vector next to the float32 parameters, and the loss and
    # its gradient evaluated in double on float64 device arrays.  Nothing of the float32 state is touched.
    def alloc_f64(self, n_doubles):
        """float64 device buffer on this context's GPU"""
        return DeviceArray64(self, n_doubles)

    def f64_set_flat(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float64)
        check(self.lib.nif_f64_set_params(self.ctx, ptr(flat), flat.size))

    def f64_get_flat(self):
        out = np.empty((self.n_params,), dtype=np.float64)
        check(self.lib.nif_f64_get_params(self.ctx, ptr(out), out.size))
        return out

    def f64_forward(self, inputs):
        """predictions [B, so] of the float64 master vector, float64"""
        x = np.asarray(inputs, dtype=np.float64)
        ncol = self.spec.pi_dim + self.spec.si_dim
        if x.ndim != 2 or x.shape[1] < ncol:
            raise ValueError("inputs: expected shape (batch, %d), got %s" % (ncol, x.shape))
        x = np.ascontiguousarray(x[:, :ncol])
        b, so = x.shape[0], self.spec.so_dim
        if not b:
            return np.empty((0, so), dtype=np.float64)
        d_x, d_u = DeviceArray64(self, x.size), DeviceArray64(self, b * so)
        try:
            d_x.upload(x)
            check(self.lib.nif_f64_forward_dev(self.ctx, d_x.at(0), b, d_u.at(0)))
            return d_u.download().reshape(b, so)
        finally:
            d_x.free(); d_u.free()

    def f64_loss_grad_dev(self, d_x, d_y, d_sw, b_local, b_global):
        check(self.lib.nif_f64_loss_grad_dev(self.ctx, d_x, d_y, d_sw, int(b_local), int(b_global)))

    def f64_grad_read(self):
        """(loss, flat gradient) of the last f64_loss_grad_dev, both float64"""
        g = np.empty((self.n_params,), dtype=np.float64)
        loss = C.c_double()
        check(self.lib.nif_f64_grad_read(self.ctx, C.byref(loss), ptr(g)))
        return float(loss.value), g

    def set_option(self, key, value):
        check(self.lib.nif_set_option(self.ctx, key.encode(), int(value)))

    def grad_read(self):
        """(loss, flat gradient) of the last loss_grad_dev, weight regulariser included"""
        g = np.empty((self.n_params,), dtype=np.float32)
        loss = C.c_float()
        check(self.lib.nif_grad_read(self.ctx, C.byref(loss), ptr(g)))
        return float(loss.value), g

    def grad_read_loss(self):
        """total loss of the last loss_grad_dev (weight regulariser included); the gradient stays on the device"""
        loss = C.c_float()
        check(self.lib.nif_grad_read(self.ctx, C.byref(loss), None))
        return float(loss.value)

    def last_loss(self):
        loss = C.c_float()
        check(self.lib.nif_last_loss(self.ctx, C.byref(loss)))
        return float(loss.value)

    def sync(self):
        check(self.lib.nif_sync(self.ctx))

    def grad_dev_ptr(self):
        return self.lib.nif_grad_dev(self.ctx)

    def stream_ptr(self):
        return self.lib.nif_stream(self.ctx)

    # ---- measurement ----------------------------------------------------------------------------
    def profile_enable(self, on=True):
        check(self.lib.nif_profile_enable(self.ctx, 1 if on else 0))

    def profile_read(self, reset=True):
        """{group: (total_ms, launches)} measured with HIP events on the context's stream."""
        n = len(_lib.PROF_NAMES)
        ms = (C.c_float * n)()
        cnt = (C.c_int64 * n)()
        check(self.lib.nif_profile_read(self.ctx, ms, cnt, n, 1 if reset else 0))
        return {nm: (float(ms[i]), int(cnt[i])) for i, nm in enumerate(_lib.PROF_NAMES)}

    def timer_start(self):
        check(self.lib.nif_timer_start(self.ctx))

    def timer_stop(self):
        ms = C.c_float()
        check(self.lib.nif_timer_stop(self.ctx, C.byref(ms)))
        return float(ms.value)
