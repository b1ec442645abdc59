"""Case table and reference helpers of tests/test_gpu_derivative_kernels.py (imported, not collected).

The reference is oracle.nif_oracle.hessian_analytic over ALL input columns in natural order, once per batch: every other index
form (a subset, a permutation, repeats) is a gather of it.  Next to it stands the same oracle under one ulp of weight noise
(_one_ulp_weights): its per-point movement s_a is the conditioning floor of the per-point bar."""
import ctypes as C

import numpy as np

from oracle import nif_oracle as O
from tests.test_gpu_parity import CONFIGS, WIDE, _cfg, _one_ulp_weights, _rel

ANCHOR_B = 190                        # rows of every anchor batch (three 64-point groups of k_jac, the last one ragged)
BAR_Y, BAR_J, BAR_H, BAR_HP = 1e-5, 2e-5, 1e-4, 2e-4      # the project's bars (BAR_HP: x_index holds a parameter column)
SENT = np.float32(-7.654321e33)       # sentinel around the _dev outputs (compared bit for bit)
NIF_ERR_INVALID = -1

# name: cfg.  Policy float32, weights from _make(boost=1.0)
CASES = {
    "ms_32x3_r2_pi3": _cfg("NIFMultiScale", 32, 3, 24, 1, 2, 2, 2, 3),     # NBL 2, 9 planes (odd), three parameter inputs
    "nif_32x2_pi3": _cfg("NIF", 32, 2, 20, 1, 2, 2, 2, 3),                 # class NIF (MODE 2), three parameter inputs
    "ms_res_48x2_pres": CONFIGS["ms_res_48x2_pres"][0],                    # NBL 3 (PEXACT false), resblocks (MODE 1)
    "ms_96x1_r2": _cfg("NIFMultiScale", 96, 1, 32, 1, 2, 2, 1, 1),         # NBL 6, grid cap 256, 3 planes (odd)
    "ms_128x6_r5_si2": WIDE["ms_128x6_r5_si2"],                            # NBL 8, one plane buffer
    "ms_tiny_b1": CONFIGS["ms_tiny_b1"][0],                                # NBL 1, 8 of 16 features padded
    "ll_32x2_pi3": _cfg("LL", 32, 2, 32, 1, 3, 2, 2, 3),                   # last-layer class, three parameter inputs
    "ll_res_48x2_r4": CONFIGS["ll_res_48x2_r4"][0],                        # last-layer class, resblocks
    "ll_cfg4_128x2_r10_so3": CONFIGS["ll_cfg4_128x2_r10_so3"][0],          # last-layer class, so * r = 30: k_mlp_jac<4>
}
PI3 = ["ms_32x3_r2_pi3", "nif_32x2_pi3", "ll_32x2_pi3"]     # columns 0-2 parameters, 3-4 coordinates
RAGGED_B = [1, 15, 17, 31, 33, 48, 49, 63, 65]
# k_jac's grid cap (launch_jac_impl): 512 groups of 64 points at NBL <= 4, 256 at NBL 6 / 8
WRAP = {"ms_32x3_r2_pi3": 512, "nif_32x2_pi3": 512, "ms_96x1_r2": 256, "ms_128x6_r5_si2": 256}


class Ref(object):
    """(y, J, H) of the fp64 oracle over every output and every input column in natural order, and the same under one ulp of
    weight noise; never modified after construction"""

    def __init__(self, spec, ws64, x):
        x64 = np.asarray(x, dtype=np.float64)
        yi, xi = list(range(spec.so)), list(range(spec.pi + spec.si))
        self.so = spec.so
        self.y, self.J, self.H = O.hessian_analytic(spec, ws64, x64, yi, xi)
        self.y1, self.J1, self.H1 = O.hessian_analytic(spec, _one_ulp_weights(ws64), x64, yi, xi)
        for a in (self.y, self.J, self.H, self.y1, self.J1, self.H1):
            a.setflags(write=False)

    def gather(self, y_index, x_index, rows=slice(None)):
        """tf.gather semantics: -> ((y, y'), (J, J'), (H, H')) of the request on the rows, ' = under the weight noise"""
        yi, xi = list(y_index), list(x_index)
        g1 = lambda J: J[rows][:, yi][:, :, xi]
        g2 = lambda H: H[rows][:, yi][:, :, xi][:, :, :, xi]
        return (self.y[rows], self.y1[rows]), (g1(self.J), g1(self.J1)), (g2(self.H), g2(self.H1))


def assert_bars(what, got, pair, bar):
    """whole tensor: rel-L2 < bar.  Per point a: max |got[a] - ref[a]| <= bar max |ref| + 3 s_a, s_a = that point's movement in
    the oracle under one ulp of weight noise (test_ill_conditioned_nets_move_with_one_ulp_of_weight_noise's rule)."""
    ref, ref1 = pair
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    B = ref.shape[0]
    err = np.abs(got - ref).reshape(B, -1).max(axis=1)
    s = np.abs(ref1 - ref).reshape(B, -1).max(axis=1)
    scale = float(np.abs(ref).max())
    lim = bar * scale + 3.0 * s
    rel = _rel(got, ref)
    worst = int(np.argmax(err - lim))
    print("%s: rel-L2 %.3g (bar %.0e), worst point %d: err / max|ref| %.3g, s_a / max|ref| %.3g"
          % (what, rel, bar, worst, err[worst] / max(scale, 1e-300), s[worst] / max(scale, 1e-300)))
    assert rel < bar, (what, "rel-L2", rel, bar)
    assert np.all(err <= lim), (what, "per point", worst, float(err[worst]), float(lim[worst]), int(np.sum(~(err <= lim))))


def hbar(spec, x_index):
    return BAR_HP if any(j < spec.pi for j in x_index) else BAR_H


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _i32(idx):
    return (C.c_int32 * len(idx))(*[int(i) for i in idx])


def c_jacobian(e, x, y_index, x_index):
    """nif_jacobian with the index arrays as they are (Engine.jacobian would de-duplicate): -> (rc, y [B, so], J [B, ny, nx])"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, ny, nx = x.shape[0], len(y_index), len(x_index)
    y = np.full((B, e.spec.so_dim), np.nan, dtype=np.float32)
    d = np.full((B, ny, nx), np.nan, dtype=np.float32)
    rc = e.lib.nif_jacobian(e.ctx, x.ctypes.data_as(C.c_void_p), B, _i32(y_index), ny, _i32(x_index), nx,
                            y.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
    return rc, y, d


def c_hessian(e, x, y_index, x_index):
    """nif_hessian with the index arrays as they are: -> (rc, y [B, so], J [B, ny, nx], H [B, ny, nx, nx])"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, ny, nx = x.shape[0], len(y_index), len(x_index)
    y = np.full((B, e.spec.so_dim), np.nan, dtype=np.float32)
    d = np.full((B, ny, nx), np.nan, dtype=np.float32)
    h = np.full((B, ny, nx, nx), np.nan, dtype=np.float32)
    rc = e.lib.nif_hessian(e.ctx, x.ctypes.data_as(C.c_void_p), B, _i32(y_index), ny, _i32(x_index), nx,
                           y.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p))
    return rc, y, d, h


class Fenced(object):
    """A device output of `rows` rows of `row` floats at float offset `off` from a 16-byte boundary, a front pad of 4 + off floats
    and a back pad of 32 rows (at least 64 floats) around it, all filled with SENT: the tail of a 32-point tile written past the
    last row lands in the back pad and is reported -- it cannot leave the allocation."""

    def __init__(self, e, rows, row, off):
        from nif_amd.engine import DeviceArray
        self.front, self.size = 4 + off, rows * row
        self.back = max(32 * row, 64)
        self.d = DeviceArray(e, self.front + self.size + self.back)
        self.d.upload(np.full(self.d.n, SENT, dtype=np.float32))

    def at(self):
        return self.d.at(self.front)

    def take(self, shape):
        """-> (the output, whether every pad word is untouched); frees the buffer"""
        full = self.d.download()
        self.d.free()
        pad = np.concatenate([full[:self.front], full[self.front + self.size:]])
        return full[self.front:self.front + self.size].reshape(shape), bool(np.all(pad.view(np.uint32) == SENT.view(np.uint32)))


def hessian_dev(e, x, y_index, x_index):
    """nif_hessian_dev with y, dydx, d2 at float offsets 1, 2, 3 from a 16-byte boundary inside sentinels
    -> (y, J, H, whether the pads of (y, J, H) are untouched)"""
    from nif_amd.engine import DeviceArray
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, so, ny, nx = x.shape[0], e.spec.so_dim, len(y_index), len(x_index)
    d_x = DeviceArray(e, x.size)
    d_x.upload(x)
    fy, fj, fh = Fenced(e, B, so, 1), Fenced(e, B, ny * nx, 2), Fenced(e, B, ny * nx * nx, 3)
    try:
        e.hessian_dev(d_x.at(0), B, y_index, x_index, fy.at(), fj.at(), fh.at())
        e.sync()
    finally:
        y, oky = fy.take((B, so))
        J, okj = fj.take((B, ny, nx))
        H, okh = fh.take((B, ny, nx, nx))
        d_x.free()
    return y, J, H, (oky, okj, okh)


def sobolev_forward_dev(e, x, x_index):
    """nif_sobolev_forward_dev with u, du/dx at float offsets 1, 2 inside sentinels -> (rc, u, du/dx, pads untouched)"""
    from nif_amd.engine import DeviceArray
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, so, nx = x.shape[0], e.spec.so_dim, len(x_index)
    d_x = DeviceArray(e, x.size)
    d_x.upload(x)
    fu, fj = Fenced(e, B, so, 1), Fenced(e, B, so * nx, 2)
    try:
        rc = e.lib.nif_sobolev_forward_dev(e.ctx, d_x.at(0), B, _i32(x_index), nx, fu.at(), fj.at())
        e.sync()
    finally:
        u, oku = fu.take((B, so))
        J, okj = fj.take((B, so, nx))
        d_x.free()
    return rc, u, J, (oku, okj)
