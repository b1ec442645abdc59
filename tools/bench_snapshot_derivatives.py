"""Snapshot-wise derivatives against the point-wise JacobianLayer / HessianLayer on the same rows.

    order 2   A: nif_hessian_dev on the expanded [T M, pi+si] table (resident; building it is not timed)
              B: nif_snapshot_derivatives_dev (order 2) on p [T, pi] and the mesh, operands and results resident
    order 1   A: nif_jacobian on the expanded host table (JacobianLayer has a host-pointer entry only: its copies are inside)
              B: nif_snapshot_derivatives (order 1), the host-pointer entry: its copies are inside as well
              Bd: nif_snapshot_derivatives_dev (order 1) on resident operands, for the kernel time alone

One process, A and B alternating, 3 warm-up and 10 timed repetitions each, every repetition synchronised with the host and timed on
the host's clock, medians; A2 is a second, independent series of A taken in the same alternation, whose distance from A is the
run's spread.  Coordinate columns only, every output.

    python tools/bench_snapshot_derivatives.py [--out profiles/snapshot_derivatives.json] [--only NAME]
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
    # name, class, cfgs, T, M  (T M = 2^20 points)
    ("ms_cfg2_64x4_r1", "NIFMultiScale", ms(64, 4, 32, 2, 1, 1, 1, 1), 64, 1 << 14),
    ("ms_cfg3_128x3_r1", "NIFMultiScale", ms(128, 3, 64, 2, 1, 2, 1, 1), 64, 1 << 14),
    ("ll_cfg4_128x2_r10_so3", LL, ms(128, 2, 32, 2, 10, 3, 3, 1, conn="last_layer"), 64, 1 << 14),
    # not asked for, for the scaling in r: the 64 x 4 net with three latents (four plane products per layer become one)
    ("ms_cfg2_64x4_r3", "NIFMultiScale", ms(64, 4, 32, 2, 3, 1, 1, 1), 64, 1 << 14),
]
WARMUP, ITERS = 3, 10


def _i32(idx):
    return (C.c_int32 * len(idx))(*[int(i) for i in idx])


def run_case(name, cls, cfgs, T, M, order):
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
    yi, xi = list(range(so)), list(range(si))
    ny, nx = len(yi), len(xi)
    n_u, n_j, n_h = n * so, n * ny * nx, n * ny * nx * nx if order == 2 else 0
    d_tab, d_p, d_x = e.alloc(table.size), e.alloc(p.size), e.alloc(x.size)
    d_a, d_b = e.alloc(n_u + n_j + max(n_h, 1)), e.alloc(n_u + n_j + max(n_h, 1))
    d_tab.upload(table); d_p.upload(p); d_x.upload(x)
    cyi, cxi, cxa = _i32(yi), _i32(xi), _i32([pi + j for j in xi])

    def args(rows, xm, u, dj, dh):
        a = _lib.nif_snapderiv_args()
        a.abi_version, a.order, a.ctx = _lib.NIF_SNAPDERIV_ABI_VERSION, order, e.ctx
        a.rows, a.rows_are_latent, a.T, a.x, a.M = rows, 0, T, xm, M
        a.y_idx, a.ny, a.x_idx, a.nx = cyi, ny, cxi, nx
        a.u, a.dudx, a.d2udx2 = u, dj, dh
        return a

    a_dev = args(d_p.at(0), d_x.at(0), d_b.at(0), d_b.at(n_u), d_b.at(n_u + n_j) if order == 2 else None)

    def b_dev():
        check(e.lib.nif_snapshot_derivatives_dev(C.byref(a_dev)))
        e.sync()

    runs = {}
    if order == 2:
        def a_run():
            check(e.lib.nif_hessian_dev(e.ctx, d_tab.at(0), n, cyi, ny, cxa, nx, d_a.at(0), d_a.at(n_u), d_a.at(n_u + n_j)))
            e.sync()
        runs = {"A": a_run, "B": b_dev, "A2": a_run}
    else:
        ha_u, ha_j = np.empty((n, so), np.float32), np.empty((n, ny, nx), np.float32)
        hb_u, hb_j = np.empty((n, so), np.float32), np.empty((n, ny, nx), np.float32)
        a_host = args(ptr(p), ptr(x), ptr(hb_u), ptr(hb_j), None)

        def a_run():
            check(e.lib.nif_jacobian(e.ctx, ptr(table), n, cyi, ny, cxa, nx, ptr(ha_u), ptr(ha_j)))

        def b_host():
            check(e.lib.nif_snapshot_derivatives(C.byref(a_host)))
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
    if order == 2:
        ra, rb = d_a.download(), d_b.download()
        parts = [(ra[:n_u], rb[:n_u]), (ra[n_u:n_u + n_j], rb[n_u:n_u + n_j]), (ra[n_u + n_j:n_u + n_j + n_h], rb[n_u + n_j:n_u + n_j + n_h])]
    else:
        parts = [(ha_u.ravel(), hb_u.ravel()), (ha_j.ravel(), hb_j.ravel())]
    rel = [float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(a.astype(np.float64)), 1e-30)) for a, b in parts]
    med = {k: float(np.median(v)) for k, v in series.items()}
    for d in (d_tab, d_p, d_x, d_a, d_b):
        d.free()
    out = {"name": name, "order": order, "T": T, "M": M, "points": n, "r": s.pi_hidden, "ny": ny, "nx": nx,
           "A": "nif_hessian_dev" if order == 2 else "nif_jacobian (host entry)",
           "B": "nif_snapshot_derivatives_dev" if order == 2 else "nif_snapshot_derivatives (host entry)",
           "A_ms": med["A"], "A2_ms": med["A2"], "B_ms": med["B"], "B_over_A": med["B"] / med["A"], "A_over_B": med["A"] / med["B"],
           "A_spread": abs(med["A2"] - med["A"]) / med["A"], "B_points_per_s": n / (med["B"] * 1e-3),
           "A_minmax_ms": [float(min(series["A"] + series["A2"])), float(max(series["A"] + series["A2"]))],
           "B_minmax_ms": [float(min(series["B"])), float(max(series["B"]))], "rel_l2_B_vs_A": rel}
    out["B_dev_split_ms"] = split
    if cls != LL:
        # the tangent kernel's matrix work, counted from the shapes: 2 n^2 flop per point, hidden layer and stream (primal + tangents of a
        # launch), over its event-pair time; the f32-input MFMA peak of the MI355X is 157.3 TFLOP/s
        n_units, nh = cfgs[0]["units"], cfgs[0]["nlayers"]
        launches = [(1 + min(3, nx - x0)) for x0 in range(0, nx, 3)] if order == 1 else [4] * (nx * (nx + 1) // 2)
        flop = sum(launches) * nh * 2 * n_units * n_units
        out["k_jac_snap"] = {"launches": len(launches), "flop_per_point": flop, "ms": split["snet_fwd"],
                             "TFLOPs": flop * n / (split["snet_fwd"] * 1e-3) / 1e12,
                             "frac_of_f32_mfma_peak": flop * n / (split["snet_fwd"] * 1e-3) / 157.3e12}
    if "Bd" in med:
        out["Bd_ms"] = med["Bd"]
        out["Bd_points_per_s"] = n / (med["Bd"] * 1e-3)
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
        for order in (1, 2):
            r = run_case(name, cls, cfgs, T, M, order)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"protocol": "one process, A / B / A2 alternating, %d warm-up + %d timed repetitions each, every repetition synchronised "
                                   "with the host and timed on the host's clock, medians; see tools/bench_snapshot_derivatives.py" % (WARMUP, ITERS),
                       "cases": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
