"""Snapshot-wise inference against the point-wise forward on the same rows, both on device-resident operands.

    A: nif_forward_dev on the expanded [T M, pi+si] table (resident; building it is not timed)
    B: nif_forward_snapshots_dev on p [T, pi] and the mesh

One process, A and B alternating, 5 warm-up and 20 timed iterations each (HIP events on the context's stream around every call),
medians; A2 is a second, independent series of A taken in the same alternation, whose distance from A is the run's spread.

    python tools/bench_snapshots.py [--out profiles/snapshots.json] [--only NAME]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ms(n, L, nst, lst, r, si, so, pi, conn="full", p_act="sine"):
    cs = {"input_dim": si, "output_dim": so, "units": n, "nlayers": L, "use_resblock": False, "connectivity": conn,
          "omega_0": 30.0, "weight_init_factor": 0.01}
    cp = {"input_dim": pi, "latent_dim": r, "units": nst, "nlayers": lst, "activation": p_act, "use_resblock": False, "omega_0": 30.0}
    return cs, cp


CASES = [
    # name, class, cfgs, T, M, gated (the issue's expectation: B no slower than A beyond the spread)
    ("ms_cfg2_64x4_r1_T8_M131072", "NIFMultiScale", ms(64, 4, 32, 2, 1, 1, 1, 1), 8, 1 << 17, False),
    ("ms_cfg2_64x4_r1_T512_M4096", "NIFMultiScale", ms(64, 4, 32, 2, 1, 1, 1, 1), 512, 4096, False),
    ("ms_cfg2_64x4_r3_T8_M131072", "NIFMultiScale", ms(64, 4, 32, 2, 3, 1, 1, 1), 8, 1 << 17, True),
    ("ms_cfg2_64x4_r3_T512_M4096", "NIFMultiScale", ms(64, 4, 32, 2, 3, 1, 1, 1), 512, 4096, True),
    ("ll_cfg4_128x6_r10_so3_T8_M262144", "NIFMultiScaleLastLayerParameterized", ms(128, 6, 32, 2, 10, 3, 3, 1, conn="last_layer", p_act="swish"),
     8, 1 << 18, True),
]
WARMUP, ITERS = 5, 20


def run_case(name, cls, cfgs, T, M):
    import nif_amd
    nif_amd.set_seed(0)
    m = getattr(nif_amd, cls)(*cfgs)
    model = m.build()
    e, s = m._engine, m._spec
    rng = np.random.default_rng(1)
    p = rng.uniform(-1, 1, size=(T, s.pi_dim)).astype(np.float32)
    x = rng.uniform(-1, 1, size=(M, s.si_dim)).astype(np.float32)
    table = np.hstack([np.repeat(p, M, axis=0), np.tile(x, (T, 1))])
    n = T * M
    d_tab, d_p, d_x, d_ua, d_ub = e.alloc(table.size), e.alloc(p.size), e.alloc(x.size), e.alloc(n * s.so_dim), e.alloc(n * s.so_dim)
    d_tab.upload(table); d_p.upload(p); d_x.upload(x)

    def run_a():
        e.forward_dev(d_tab.at(0), n, d_ua.at(0))

    def run_b():
        nif_amd._lib.check(e.lib.nif_forward_snapshots_dev(e.ctx, d_p.at(0), 0, T, d_x.at(0), None, M, d_ub.at(0)))

    def timed(f):
        e.timer_start(); f(); return e.timer_stop()

    series = {"A": [], "B": [], "A2": []}
    for it in range(WARMUP + ITERS):
        for key, f in (("A", run_a), ("B", run_b), ("A2", run_a)):
            t = timed(f)
            if it >= WARMUP:
                series[key].append(t)
    ua, ub = d_ua.download(), d_ub.download()
    rel = float(np.linalg.norm(ua.astype(np.float64) - ub) / max(np.linalg.norm(ua.astype(np.float64)), 1e-30))
    med = {k: float(np.median(v)) for k, v in series.items()}
    for d in (d_tab, d_p, d_x, d_ua, d_ub):
        d.free()
    spread = abs(med["A2"] - med["A"]) / med["A"]
    return {"name": name, "T": T, "M": M, "points": n, "A_ms": med["A"], "A2_ms": med["A2"], "B_ms": med["B"],
            "A_points_per_s": n / (med["A"] * 1e-3), "B_points_per_s": n / (med["B"] * 1e-3), "B_over_A": med["B"] / med["A"],
            "A_spread": spread, "A_minmax_ms": [float(min(series["A"] + series["A2"])), float(max(series["A"] + series["A2"]))],
            "B_minmax_ms": [float(min(series["B"])), float(max(series["B"]))], "rel_l2_B_vs_A": rel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    res = []
    for name, cls, cfgs, T, M, gated in CASES:
        if a.only and a.only != name:
            continue
        r = run_case(name, cls, cfgs, T, M)
        r["gated"] = gated
        r["gate_ok"] = (r["B_over_A"] <= 1.0 + r["A_spread"]) if gated else None
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"protocol": "one process, A / B / A2 alternating, %d warm-up + %d timed calls each, HIP events per call, medians; "
                                   "A = nif_forward_dev on the resident expanded table, B = nif_forward_snapshots_dev" % (WARMUP, ITERS),
                       "cases": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
