"""Snapshot-wise parameter derivatives against the point-wise JacobianLayer on the same rows, parameter columns, every output.

    A:  nif_jacobian on the expanded host table [T M, pi+si] (JacobianLayer has a host-pointer entry only: its copies are inside;
        building the table is not timed)
    B:  nif_snapshot_param_derivatives, the host-pointer entry, on p [T, pi] and the mesh: its copies are inside as well
    Bd: nif_snapshot_param_derivatives_dev on resident operands, for the device time alone

Each case runs on a shared mesh [M, si] and on per-snapshot meshes (the same points, handed over as T meshes with offsets).  One
process, A and B alternating, 3 warm-up and 10 timed repetitions each, every repetition synchronised with the host and timed on the
host's clock, medians; A2 is a second, independent series of A taken in the same alternation, whose distance from A is the run's
spread.

    python tools/bench_snapshot_param_derivatives.py [--out profiles/snapshot_param_derivatives.json] [--only NAME]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ms(n, L, nst, lst, r, si, so, pi, conn="full", p_act="sine"):
    cs = {"input_dim": si, "output_dim": so, "units": n, "nlayers": L, "use_resblock": False, "connectivity": conn,
          "omega_0": 30.0, "weight_init_factor": 0.01}
    cp = {"input_dim": pi, "latent_dim": r, "units": nst, "nlayers": lst, "activation": p_act, "use_resblock": False, "omega_0": 30.0}
    return cs, cp


LL = "NIFMultiScaleLastLayerParameterized"
CASES = [
    # the BASELINE-shaped nets of tools/bench_snapshot_derivatives.py: name, class, cfgs, T, M  (T M = 2^20 points)
    ("ms_cfg2_64x4_r1", "NIFMultiScale", ms(64, 4, 32, 2, 1, 1, 1, 1), 64, 1 << 14),
    ("ms_cfg3_128x3_r1", "NIFMultiScale", ms(128, 3, 64, 2, 1, 2, 1, 1), 64, 1 << 14),
    ("ll_cfg4_128x2_r10_so3", LL, ms(128, 2, 32, 2, 10, 3, 3, 1, conn="last_layer"), 64, 1 << 14),
    ("ms_cfg2_64x4_r3", "NIFMultiScale", ms(64, 4, 32, 2, 3, 1, 1, 1), 64, 1 << 14),
    # not a BASELINE shape, for the scaling in r and nd: ten latents, three parameter columns (one launch of three streams)
    ("ms_64x4_r10_pi3", "NIFMultiScale", ms(64, 4, 32, 2, 10, 1, 1, 3), 64, 1 << 14),
]
WARMUP, ITERS = 3, 10


def _i32(idx):
    return (C.c_int32 * len(idx))(*[int(i) for i in idx])


def run_case(name, cls, cfgs, T, M, ragged):
    import nif_amd
    from nif_amd import _lib
    from nif_amd._lib import check, ptr
    nif_amd.set_seed(0)
    m = getattr(nif_amd, cls)(*cfgs)
    m.build()
    e, s = m._engine, m._spec
    pi, si, so = s.pi_dim, s.si_dim, s.so_dim
    rng = np.random.default_rng(1)
    p = rng.uniform(-1, 1, size=(T, pi)).astype(np.float32)
    x = rng.uniform(-1, 1, size=(M, si)).astype(np.float32)
    table = np.ascontiguousarray(np.hstack([np.repeat(p, M, axis=0), np.tile(x, (T, 1))]))
    n = T * M
    xm = np.ascontiguousarray(np.tile(x, (T, 1))) if ragged else x
    off = (np.arange(T + 1, dtype=np.int64) * M) if ragged else None
    yi, cols = list(range(so)), list(range(pi))
    ny, nd = len(yi), len(cols)
    n_u, n_j = n * so, n * ny * nd
    d_p, d_x, d_b = e.alloc(p.size), e.alloc(xm.size), e.alloc(n_u + n_j)
    d_p.upload(p); d_x.upload(xm)
    cyi, cpi = _i32(yi), _i32(cols)

    def args(rows, xp, u, dj):
        a = _lib.nif_snapparam_args()
        a.abi_version, a.ctx = _lib.NIF_SNAPPARAM_ABI_VERSION, e.ctx
        a.rows, a.rows_are_latent, a.T, a.x, a.M = rows, 0, T, xp, M
        a.offsets_host = None if off is None else off.ctypes.data_as(C.POINTER(C.c_int64))
        a.y_idx, a.ny, a.p_idx, a.np = cyi, ny, cpi, nd
        a.u, a.dudp = u, dj
        return a

    ha_u, ha_j = np.empty((n, so), np.float32), np.empty((n, ny, nd), np.float32)
    hb_u, hb_j = np.empty((n, so), np.float32), np.empty((n, ny, nd), np.float32)
    a_dev = args(d_p.at(0), d_x.at(0), d_b.at(0), d_b.at(n_u))
    a_host = args(ptr(p), ptr(xm), ptr(hb_u), ptr(hb_j))

    def a_run():
        check(e.lib.nif_jacobian(e.ctx, ptr(table), n, cyi, ny, cpi, nd, ptr(ha_u), ptr(ha_j)))

    def b_host():
        check(e.lib.nif_snapshot_param_derivatives(C.byref(a_host)))

    def b_dev():
        check(e.lib.nif_snapshot_param_derivatives_dev(C.byref(a_dev)))
        e.sync()

    runs = {"A": a_run, "B": b_host, "A2": a_run, "Bd": b_dev}
    series = {k: [] for k in runs}
    for it in range(WARMUP + ITERS):
        for key, f in runs.items():
            e.sync()
            t0 = time.perf_counter(); f(); t = (time.perf_counter() - t0) * 1e3
            if it >= WARMUP:
                series[key].append(t)
    # where B's device time goes: the library's event pairs over three more calls of the device entry
    e.profile_enable(True)
    e.profile_read(reset=True)
    for _ in range(3):
        b_dev()
    split = {k: v[0] / 3 for k, v in e.profile_read(reset=True).items() if v[1]}
    e.profile_enable(False)
    parts = [(ha_u.ravel(), hb_u.ravel()), (ha_j.ravel(), hb_j.ravel())]
    rel = [float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(a.astype(np.float64)), 1e-30)) for a, b in parts]
    med = {k: float(np.median(v)) for k, v in series.items()}
    for d in (d_p, d_x, d_b):
        d.free()
    r = s.pi_hidden
    out = {"name": name, "mesh": "per-snapshot" if ragged else "shared", "T": T, "M": M, "points": n, "r": r, "ny": ny, "nd": nd,
           "A": "nif_jacobian (host entry)", "B": "nif_snapshot_param_derivatives (host entry)", "Bd": "nif_snapshot_param_derivatives_dev",
           "A_ms": med["A"], "A2_ms": med["A2"], "B_ms": med["B"], "Bd_ms": med["Bd"], "B_over_A": med["B"] / med["A"],
           "A_over_B": med["A"] / med["B"], "A_spread": abs(med["A2"] - med["A"]) / med["A"],
           "B_points_per_s": n / (med["B"] * 1e-3), "Bd_points_per_s": n / (med["Bd"] * 1e-3),
           "A_minmax_ms": [float(min(series["A"] + series["A2"])), float(max(series["A"] + series["A2"]))],
           "B_minmax_ms": [float(min(series["B"])), float(max(series["B"]))],
           "Bd_minmax_ms": [float(min(series["Bd"])), float(max(series["Bd"]))],
           "bytes_host_A": int(table.nbytes + ha_u.nbytes + ha_j.nbytes), "bytes_host_B": int(p.nbytes + xm.nbytes + hb_u.nbytes + hb_j.nbytes),
           "rel_l2_B_vs_A": rel, "B_dev_split_ms": split}
    if cls != LL:
        # plane products per point and hidden layer, counted from the shapes (not a measurement): the point-wise layers run
        # (r + 1)(1 + g) per launch group of g columns, the weight-tangent kernel 1 + 2 g
        groups = [min(3, nd - d0) for d0 in range(0, nd, 3)]
        n_units, nh = cfgs[0]["units"], cfgs[0]["nlayers"]
        flop = sum(1 + 2 * g for g in groups) * nh * 2 * n_units * n_units
        out["plane_products_counted"] = {"pointwise": sum((r + 1) * (1 + g) for g in groups), "weight_tangent": sum(1 + 2 * g for g in groups)}
        out["k_jac_wt"] = {"launches": len(groups), "flop_per_point": flop, "ms": split["snet_fwd"],
                           "TFLOPs": flop * n / (split["snet_fwd"] * 1e-3) / 1e12,
                           "frac_of_f32_mfma_peak": flop * n / (split["snet_fwd"] * 1e-3) / 157.3e12}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    res = []
    for name, cls, cfgs, T, M in CASES:
        if a.only and a.only != name:
            continue
        for ragged in (False, True):
            r = run_case(name, cls, cfgs, T, M, ragged)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"protocol": "one process, A / B / A2 / Bd alternating, %d warm-up + %d timed repetitions each, every repetition "
                                   "synchronised with the host and timed on the host's clock, medians; see "
                                   "tools/bench_snapshot_param_derivatives.py" % (WARMUP, ITERS),
                       "cases": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
