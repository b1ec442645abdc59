"""Second-order snapshot-wise parameter derivatives against the point-wise HessianLayer on the same rows and columns, every output.

    A:   nif_hessian_dev on the expanded table [T M, pi+si], resident on the device, over the pi parameter columns: the only way
         to these numbers without the snapshot call (building and uploading the table is not timed)
    B:   nif_snapshot_param_second_derivatives_dev on p [T, pi] and the mesh, the same columns (its first-order part included: u and
         dudp come from nif_snapshot_param_derivatives_dev inside it)
    L1, L3:  the same entry on latents with nd = 1 and nd = 3 drawn directions and a drawn symmetric second direction each (no
         point-wise counterpart; the ratio against A is given where nd = pi)

Each case runs on a shared mesh [M, si] and on per-snapshot meshes (the same points, handed over as T meshes with offsets).  One
process, all series alternating, 3 warm-up and 10 timed repetitions each (the warm-up carries every shape through its first launches
and the clock ramp), every repetition synchronised with the host and timed on the host's clock, medians; A2 is a second, independent
series of A taken in the same alternation, whose distance from A is the run's spread.

    python tools/bench_snapshot_param_second_derivatives.py [--out profiles/snapparam2.json] [--only NAME]
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

from tools.bench_snapshot_param_derivatives import CASES, LL, _i32      # noqa: E402  (the configs and sizes of the first-order tool)

WARMUP, ITERS = 3, 10


def run_case(name, cls, cfgs, T, M, ragged):
    import nif_amd
    from nif_amd import _lib
    from nif_amd._lib import check
    nif_amd.set_seed(0)
    m = getattr(nif_amd, cls)(*cfgs)
    m.build()
    e, s = m._engine, m._spec
    pi, si, so, r = s.pi_dim, s.si_dim, s.so_dim, s.pi_hidden
    rng = np.random.default_rng(1)
    p = rng.uniform(-1, 1, size=(T, pi)).astype(np.float32)
    x = rng.uniform(-1, 1, size=(M, si)).astype(np.float32)
    table = np.ascontiguousarray(np.hstack([np.repeat(p, M, axis=0), np.tile(x, (T, 1))]))
    n = T * M
    xm = np.ascontiguousarray(np.tile(x, (T, 1))) if ragged else x
    off = (np.arange(T + 1, dtype=np.int64) * M) if ragged else None
    lat = m.model_p_to_lr().predict(p)
    dirs = {nd: rng.uniform(-1, 1, size=(T, nd, r)).astype(np.float32) for nd in (1, 3)}
    dds = {}
    for nd in (1, 3):
        dd = rng.uniform(-1, 1, size=(T, nd, nd, r)).astype(np.float32)
        dds[nd] = np.ascontiguousarray((dd + dd.transpose(0, 2, 1, 3)).astype(np.float32))
    yi, cols = list(range(so)), list(range(pi))
    ny = len(yi)
    ndmax = max(pi, 3)
    n_u, n_j, n_h = n * so, n * ny * ndmax, n * ny * ndmax * ndmax
    d_t, d_p, d_x, d_l = e.alloc(table.size), e.alloc(p.size), e.alloc(xm.size), e.alloc(lat.size)
    d_d = {nd: e.alloc(dirs[nd].size) for nd in (1, 3)}
    d_dd = {nd: e.alloc(dds[nd].size) for nd in (1, 3)}
    d_a, d_b = e.alloc(n_u + n_j + n_h), e.alloc(n_u + n_j + n_h)
    d_t.upload(table); d_p.upload(p); d_x.upload(xm); d_l.upload(lat)
    for nd in (1, 3):
        d_d[nd].upload(dirs[nd]); d_dd[nd].upload(dds[nd])
    cyi, cpi = _i32(yi), _i32(cols)

    def args(rows, drows, ddrows, nd):
        a = _lib.nif_snapparam2_args()
        a.abi_version, a.ctx = _lib.NIF_SNAPPARAM2_ABI_VERSION, e.ctx
        a.rows, a.rows_are_latent, a.T, a.x, a.M = rows, 0 if drows is None else 1, T, d_x.at(0), M
        a.offsets_host = None if off is None else off.ctypes.data_as(C.POINTER(C.c_int64))
        a.y_idx, a.ny = cyi, ny
        if drows is None:
            a.p_idx, a.np = cpi, pi
        else:
            a.drows, a.ddrows, a.nd = drows, ddrows, nd
        a.u, a.dudp, a.d2udp2 = d_b.at(0), d_b.at(n_u), d_b.at(n_u + n_j)
        return a

    a_p = args(d_p.at(0), None, None, pi)
    a_l = {nd: args(d_l.at(0), d_d[nd].at(0), d_dd[nd].at(0), nd) for nd in (1, 3)}

    def a_run():
        e.hessian_dev(d_t.at(0), n, yi, cols, d_a.at(0), d_a.at(n_u), d_a.at(n_u + n_j))
        e.sync()

    def b_run():
        check(e.lib.nif_snapshot_param_second_derivatives_dev(C.byref(a_p)))
        e.sync()

    def l_run(nd):
        check(e.lib.nif_snapshot_param_second_derivatives_dev(C.byref(a_l[nd])))
        e.sync()

    # results first: B against A on the same columns (before the latent runs reuse B's outputs)
    a_run(); b_run()
    got_a, got_b = d_a.download(), d_b.download()
    sizes = [(0, n * so), (n_u, n * ny * pi), (n_u + n_j, n * ny * pi * pi)]
    rel = [float(np.linalg.norm(got_a[o:o + k].astype(np.float64) - got_b[o:o + k]) / max(np.linalg.norm(got_a[o:o + k].astype(np.float64)), 1e-30))
           for o, k in sizes]
    runs = {"A": a_run, "B": b_run, "L1": lambda: l_run(1), "A2": a_run, "L3": lambda: l_run(3)}
    series = {k: [] for k in runs}
    for it in range(WARMUP + ITERS):
        for key, f in runs.items():
            e.sync()
            t0 = time.perf_counter(); f(); t = (time.perf_counter() - t0) * 1e3
            if it >= WARMUP:
                series[key].append(t)
    # where B's device time goes: the library's event pairs over three more calls
    e.profile_enable(True)
    e.profile_read(reset=True)
    for _ in range(3):
        b_run()
    split = {k: v[0] / 3 for k, v in e.profile_read(reset=True).items() if v[1]}
    e.profile_enable(False)
    med = {k: float(np.median(v)) for k, v in series.items()}
    for d in [d_t, d_p, d_x, d_l, d_a, d_b] + list(d_d.values()) + list(d_dd.values()):
        d.free()
    out = {"name": name, "mesh": "per-snapshot" if ragged else "shared", "T": T, "M": M, "points": n, "r": r, "ny": ny, "pi": pi,
           "A": "nif_hessian_dev on the resident expanded table, pi parameter columns",
           "B": "nif_snapshot_param_second_derivatives_dev, p rows, the same columns",
           "L1": "the same entry, latent rows, nd = 1 with d2latent", "L3": "the same entry, latent rows, nd = 3 with d2latent",
           "A_ms": med["A"], "A2_ms": med["A2"], "B_ms": med["B"], "L1_ms": med["L1"], "L3_ms": med["L3"],
           "B_over_A": med["B"] / med["A"], "A_over_B": med["A"] / med["B"], "A_spread": abs(med["A2"] - med["A"]) / med["A"],
           "L_over_A_where_nd_is_pi": (med["L1"] / med["A"] if pi == 1 else (med["L3"] / med["A"] if pi == 3 else None)),
           "B_points_per_s": n / (med["B"] * 1e-3),
           "A_minmax_ms": [float(min(series["A"] + series["A2"])), float(max(series["A"] + series["A2"]))],
           "B_minmax_ms": [float(min(series["B"])), float(max(series["B"]))],
           "rel_l2_B_vs_A_u_dudp_d2udp2": rel, "B_dev_split_ms": split}
    if cls != LL:
        # plane products per point and hidden layer, counted from the shapes (not a measurement): the point-wise kernel runs
        # 4 (r + 1) per pair, the weight-tangent kernel 6 per diagonal and 9 per general pair (the p= route always has W'')
        npair, ndiag = pi * (pi + 1) // 2, pi
        out["plane_products_counted"] = {"pointwise": 4 * (r + 1) * npair, "weight_tangent2": 6 * ndiag + 9 * (npair - ndiag),
                                         "first_order_inside_B": sum(1 + 2 * min(3, pi - d0) for d0 in range(0, pi, 3))}
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
            json.dump({"protocol": "one process, A / B / L1 / A2 / L3 alternating, %d warm-up + %d timed repetitions each, every "
                                   "repetition synchronised with the host and timed on the host's clock, medians; see "
                                   "tools/bench_snapshot_param_second_derivatives.py" % (WARMUP, ITERS),
                       "cases": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
