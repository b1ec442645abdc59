"""The snapshot-wise training step of NIFMultiScaleLastLayerParameterized in NumPy float64, from its factors (DESIGN 2.11;
include/nif_hip_snapfit.h): T snapshots u [T, M, so] on one shared mesh x [M, si] with the ParameterNet inputs p [T, pi].  The ShapeNet
sees the M mesh rows, the ParameterNet the T rows of p, and the head is the only sum over (t, m):

    E[t, m, s]      = sum_c phi[m, s, c] a[t, c] + bias[s] - y[t, m, s]
    du[t, m, s]     = loss'(E) sw[t, m] / (Bg so)
    dL/dphi[m, s, c] = sum_t du[t, m, s] a[t, c]          -> ShapeNet adjoint and weight gradients over M points
    dL/da[t, c]      = sum_m sum_s phi[m, s, c] du[t, m, s]   -> r x r layer and ParameterNet adjoint over T rows
    dL/dbias[s]      = sum_t sum_m du[t, m, s]

tests/test_fit_snapshots.py holds this equal to oracle.loss_and_grad on the expanded table; the engine double of that file and the GPU
tests (tests/test_gpu_fit_snapshots.py) use it and the nets below."""
import numpy as np

from oracle import nif_oracle as O
from tests.cfgs import cfg_ll

# the GPU tests' nets: (kind, cfg_shape_net, cfg_parameter_net); the third is w129x1 of tests/wide_ll_cases.py (the wide route)
NET_R10_SO3 = cfg_ll(n=32, L=2, nst=32, lst=1, r=10, si=2, so=3, pi=2)
SHAPES = [(1, 1), (1, 33), (7, 64), (9, 65), (40, 257)]      # (T, M)
LOSSES = ["mse", "mae", "huber", "log_cosh"]


def expanded_table(p, x):
    """[T M, pi + si]: snapshot after snapshot, each on the whole mesh -- the table fit() would train on"""
    p, x = np.asarray(p), np.asarray(x)
    return np.hstack([np.repeat(p, x.shape[0], axis=0), np.tile(x, (p.shape[0], 1))])


def loss_and_grad(spec, ws, p, x, y, sw=None, batch_global=None, loss="mse"):
    """(loss, [gradient per variable, Keras order]) by the factored formulas; y [T, M, so], sw [T, M] or None"""
    assert spec.kind == O.KIND_LL
    p, x, y = np.asarray(p, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    T, M = p.shape[0], x.shape[0]
    Bg = T * M if batch_global is None else batch_global
    a, _, ptape = O.pnet_forward(spec, ws, p, keep=True)          # [T, r]
    phi, stape = O.snet_phi(spec, ws, x, keep=True)               # [M, so, r]
    E = np.einsum("msc,tc->tms", phi, a) + ws[-1] - y
    lv, ld = O.loss_vd(loss)
    w = np.ones((T, M)) if sw is None else np.asarray(sw, dtype=np.float64)
    total = (lv(E).mean(axis=2) * w).sum() / Bg
    du = ld(E) * w[:, :, None] / (Bg * spec.so)
    g_phi = np.einsum("tms,tc->msc", du, a)
    g_a = np.einsum("msc,tms->tc", phi, du)
    g_bias = du.sum(axis=(0, 1))
    return total, O.pnet_backward(spec, ws, ptape, g_a) + O._snet_backward(spec, ws, stape, g_phi) + [g_bias]


def problem(spec, T, M, seed=0, zeros=True):
    """float32 (p, x, y, sw) of a (T, M) case; sw [T, M] in [0.5, 1.5), from 20 samples on with a fifth of its entries zero"""
    rng = np.random.default_rng(seed + 1000 * T + M)
    p = rng.uniform(-1, 1, size=(T, spec.pi)).astype(np.float32)
    x = rng.uniform(-1, 1, size=(M, spec.si)).astype(np.float32)
    y = rng.uniform(-1, 1, size=(T, M, spec.so)).astype(np.float32)
    sw = rng.uniform(0.5, 1.5, size=(T, M)).astype(np.float32)
    if zeros and T * M >= 20:
        sw[rng.uniform(size=(T, M)) < 0.2] = 0.0
    return p, x, y, sw
