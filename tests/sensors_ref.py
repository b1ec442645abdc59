"""Sensor placement on the basis of NIFMultiScaleLastLayerParameterized in NumPy float64 (include/nif_hip_sensors.h):
greedy column-pivoted QR (Businger-Golub, QDEIM) of Phi^T, Phi = model_x_to_phi(x) [M, so, r] as N = M so candidate rows of r values,
row m so + s = output component s at mesh point m.  For k = 0 .. K - 1

    j_k = argmax over the eligible rows of |res_row|^2      (ties: the lowest row; eligible: mask[m] and not yet chosen)
    d_k = |res_row(j_k)|,  q_k = res_row(j_k) / d_k
    every row: res_row -= (res_row . q_k) q_k               (row j_k becomes exactly 0)

and pivot -1, d = 0 from the first step at which no eligible row has a positive norm.  Besides pivots and d, select() returns per step
the gap 1 - s2 / s1 of the two best scores and d_k / d_0: a comparison of pivots with another implementation is meaningful only where
the gap is far above that implementation's rounding.  tests/test_select_sensors.py holds the pivots equal to SciPy's pivoted QR and
the conditions of the GPU cases true on the oracle's phi; tests/test_gpu_select_sensors.py re-asserts them on the device's phi."""
import collections

import numpy as np

from oracle import nif_oracle as O
from tests.cfgs import cfg_ll

SensorRef = collections.namedtuple("SensorRef", ["pivots", "diag", "gap", "rel"])

GAP_MIN, REL_MIN = 1e-3, 0.05      # the conditions of a compared step: gap >= GAP_MIN and d_k / d_0 >= REL_MIN


def select(phi, K, mask=None):
    """phi [M, so, r] -> SensorRef(pivots [K] int64, diag [K], gap [K], rel [K]) in float64; gap and rel are nan where no row was found"""
    phi = np.asarray(phi, dtype=np.float64)
    M, so, r = phi.shape
    res = phi.reshape(M * so, r).copy()
    elig = np.ones(M * so, dtype=bool) if mask is None else np.repeat(np.asarray(mask) != 0, so)
    piv, d = np.full(K, -1, dtype=np.int64), np.zeros(K)
    gap, rel = np.full(K, np.nan), np.full(K, np.nan)
    for k in range(K):
        sc = np.einsum("ij,ij->i", res, res)
        sc[~elig] = -1.0
        j = int(np.argmax(sc))      # (the first maximum: the lowest row)
        if not sc[j] > 0.0:
            break
        s2 = max(float(np.partition(sc, -2)[-2]), 0.0) if sc.size > 1 else 0.0
        piv[k], d[k], gap[k] = j, np.sqrt(sc[j]), 1.0 - s2 / sc[j]
        rel[k] = d[k] / d[0]
        q = res[j] / d[k]
        res -= np.outer(res @ q, q)
        res[j] = 0.0
        elig[j] = False
    return SensorRef(piv, d, gap, rel)


def conditions_hold(ref, upto=None):
    """(ok, min gap, min rel) over the steps 0 .. upto - 1 (None: every step that found a row)"""
    n = int((ref.pivots >= 0).sum()) if upto is None else upto
    if n == 0:
        return True, np.inf, np.inf
    g, q = float(np.min(ref.gap[:n])), float(np.min(ref.rel[:n]))
    return bool(g >= GAP_MIN and q >= REL_MIN), g, q


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------------------
# net: (kind, cfg_shape_net, cfg_parameter_net); seed: of the weights and of the mesh; M points uniform in [-span, span]^si; K sensors;
# policy; keep: None, or the number of points a random mask admits (the others cannot carry a sensor).
# A dense mesh of a smooth phi has near-ties by construction (neighbours of the best point): the large meshes admit a sparse subset, so
# that the gap condition can hold while every tile of the mesh, in every stride of the persistent grid, is still scored and reduced.
Case = collections.namedtuple("Case", ["net", "seed", "M", "K", "span", "policy", "keep"])


def _c(net, seed, M, K, span=1.0, policy="float32", keep=None):
    return Case(net, seed, M, K, span, policy, keep)


def weights(case):
    """float32 weights of a case, as the GPU tests set them"""
    spec = O.Spec(*case.net)
    return spec, O.init_weights(spec, np.random.default_rng(case.seed), dtype=np.float32)


def mesh(case):
    """(x [M, si] float32, mask [M] bool or None)"""
    si = case.net[1]["input_dim"]
    rng = np.random.default_rng(1000 + case.seed)
    x = rng.uniform(-case.span, case.span, size=(case.M, si)).astype(np.float32)
    mask = None
    if case.keep is not None:
        mask = np.zeros(case.M, dtype=bool)
        mask[rng.choice(case.M, size=case.keep, replace=False)] = True
    return x, mask


def _net(**k):
    return cfg_ll(nst=8, lst=1, pi=1, **k)


# The seeds were searched (a handful to a few dozen each) for gap >= GAP_MIN and d_k / d_0 >= REL_MIN at every compared step on the
# oracle's phi; tests/test_select_sensors.py asserts that they hold.  Grid strides: 1024 workgroups x 8 tiles x 32 points = 262144
# points up to r = 40, half of that above.
CASES = {
    "r1_so1_m1": _c(_net(n=16, L=1, r=1, so=1, si=1), 0, 1, 1),                        # one point, one row, one step
    "r3_so2_m31": _c(_net(n=16, L=1, r=3, so=2, si=2), 0, 31, 3),                      # less than a tile, K = r
    "r3_so2_m33_k2": _c(_net(n=16, L=1, r=3, so=2, si=2), 0, 33, 2),                   # a tile and one point, 1 < K < r
    "r10_so1_m257": _c(_net(n=32, L=2, r=10, so=1, si=2), 1, 257, 10),                 # more than one workgroup (8 tiles each)
    "r10_so3_m33": _c(_net(n=32, L=2, r=10, so=3, si=2), 0, 33, 10),
    "r10_so3_m500_k4": _c(_net(n=128, L=2, r=10, so=3, si=2), 3, 500, 4),              # configs[3]'s head on a 128-unit net
    "r16_so4_m257": _c(_net(n=64, L=1, r=16, so=4, si=3), 1, 257, 16),                 # so r = 64; the last form with q in scalar registers
    "r64_so1_m257": _c(_net(n=128, L=1, r=64, so=1, si=3), 23, 257, 64),               # the widest row, 64 steps, q through LDS
    "r64_so1_m2000_k1": _c(_net(n=128, L=1, r=64, so=1, si=3), 0, 2000, 1),            # K = 1: no update pass at all
    "w256_r10_so3_m129": _c(_net(n=256, L=1, r=10, so=3, si=3), 0, 129, 10),           # a 256-unit ShapeNet: phi by the k_wide route
    "res_r4_so2_m257": _c(_net(n=48, L=2, r=4, so=2, si=2, s_res=True), 0, 257, 4),    # resblocks
    "bf16_r4_so2_m97": _c(_net(n=64, L=2, r=4, so=2, si=2), 4, 97, 4, policy="mixed_bfloat16"),
    "r10_so1_m30000": _c(_net(n=32, L=2, r=10, so=1, si=3), 2, 30000, 10),             # every point a candidate
    "r3_so1_m400001_keep400": _c(_net(n=16, L=1, r=3, so=1, si=2), 4, 400001, 3, keep=400),      # a pivot in the second stride of 1024 workgroups
    "r48_so1_m135003_keep400": _c(_net(n=64, L=1, r=48, so=1, si=2), 0, 135003, 5, keep=400),    # more than one stride of 512
}
# r = 10 on a 6-unit ShapeNet: phi = [W | b] [h; 1] has rank 7.  Compared up to the rank; past it the residual is rounding
DEFICIENT = _c(_net(n=6, L=1, r=10, so=1, si=2), 36, 257, 10)
DEFICIENT_RANK = 7
RANK_DROP = 1e-4      # d_rank / d_0 is below this, on the oracle's phi and on the device


def oracle_phi(case):
    """model_x_to_phi of a case's mesh by the oracle in float64 (under the case's policy)"""
    spec, ws = weights(case)
    x, _ = mesh(case)
    rnd = O.bf16_round if case.policy == "mixed_bfloat16" else None
    return O.snet_phi(spec, [w.astype(np.float64) for w in ws], x.astype(np.float64), rnd=rnd)
