"""Milliseconds per nif_select_sensors_dev call (csrc/k_sensors.hip) at M = 2^20 mesh points on configs[3]'s 128 x 6
ShapeNet of the last-layer class, in one process on one GPU:
  * so = 1, r = 10, K = 10;   * configs[3]'s head, so = 3, r = 10, K = 10;   * so = 1, r = 64, K = 64.
The clock is ramped with untimed calls, then the median of `--steps` host-synchronised calls is taken.  A second run under the
library's profiler splits the call from its event pairs: the phi pass (snet_fwd) and the 2 K selection launches (reduce).  The bytes
the selection must move -- k_sens_init reads PHI and writes the residual and the scores, each of the K - 1 update passes reads and
writes both -- over the selection's time are set against the read and the store-stream rates the project measured.

The baseline is what a user of the parent commit does: model_x_to_phi(x) to the host, then scipy.linalg.qr(Phi^T, pivoting=True)
there (LAPACK geqp3); where SciPy is absent, the NumPy float64 recurrence of tests/sensors_ref.py.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_READ_TBS, HBM_STORE_TBS = 6.29, 5.77      # measured read bandwidth, pure 16-byte store stream
M = 1 << 20
CASES = [("so1_r10_k10", 1, 10, 10), ("configs3_head_so3_r10_k10", 3, 10, 10), ("so1_r64_k64", 1, 64, 64)]
SI, PI = 3, 1


def _cfgs(so, r):
    cs = {"input_dim": SI, "output_dim": so, "units": 128, "nlayers": 6, "use_resblock": False, "connectivity": "last_layer",
          "omega_0": 30.0, "weight_init_factor": 0.01}
    cp = {"input_dim": PI, "latent_dim": r, "units": 32, "nlayers": 2, "activation": "swish", "use_resblock": False, "omega_0": 30.0}
    return cs, cp


def _median_ms(f, sync, ramp, steps):
    for _ in range(ramp):
        f()
    sync()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        f()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 4) for t in ts]


def _host_qr(phi, K):
    """the first K pivots of the pivoted QR of Phi^T on the host, and which routine ran"""
    rows = phi.reshape(-1, phi.shape[2])
    try:
        import scipy.linalg as sl
    except ImportError:
        from tests import sensors_ref
        return sensors_ref.select(phi, K).pivots, "numpy float64 recurrence"
    return sl.qr(rows.T, mode="r", pivoting=True)[1][:K].astype(np.int64), "scipy.linalg.qr(pivoting=True)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ramp", type=int, default=3)
    ap.add_argument("--baseline-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import nif_amd
    res = {"tool": "bench_sensors", "M": M, "steps": args.steps, "ramp": args.ramp, "hbm_read_tbs": HBM_READ_TBS,
           "hbm_store_tbs": HBM_STORE_TBS, "cases": []}
    x = np.random.default_rng(0).uniform(-1.0, 1.0, size=(M, SI)).astype(np.float32)
    for name, so, r, K in CASES:
        nif_amd.set_seed(0)
        m = nif_amd.NIFMultiScaleLastLayerParameterized(*_cfgs(so, r))
        m.build()
        e = m._engine
        d_x, d_p, d_d = e.alloc(x.size), e.alloc(2 * K), e.alloc(K)
        d_x.upload(x)
        call = lambda: e.select_sensors_dev(d_x.at(0), M, None, K, d_p.at(0), d_d.at(0))
        ms, ts = _median_ms(call, e.sync, args.ramp, args.steps)
        piv = d_p.download().view(np.int64)
        e.profile_enable(True)
        e.profile_read(reset=True)
        for _ in range(args.steps):
            call()
        e.sync()
        prof = e.profile_read(reset=True)
        e.profile_enable(False)
        per = {k: v[0] / args.steps for k, v in prof.items() if v[1]}
        phi_ms, sel_ms = per.get("snet_fwd", 0.0), per.get("reduce", 0.0)
        N = M * so
        nbytes = (8.0 * N * r + 4.0 * N) + (K - 1) * (8.0 * N * r + 8.0 * N)
        out = {"name": name, "so": so, "r": r, "K": K, "launches": 2 * K,
               "device": {"ms_median": round(ms, 4), "ms": ts, "phi_pass_ms": round(phi_ms, 4), "selection_ms": round(sel_ms, 4),
                          "phi_share_of_call": round(phi_ms / (phi_ms + sel_ms), 4) if phi_ms + sel_ms > 0 else None,
                          "selection_gb": round(nbytes / 1e9, 4),
                          "selection_tbs": round(nbytes / (sel_ms * 1e-3) / 1e12, 3) if sel_ms > 0 else None,
                          "us_per_selection_launch": round(sel_ms * 1e3 / (2 * K), 2)}}
        if sel_ms > 0:
            out["device"]["fraction_of_store_stream"] = round(out["device"]["selection_tbs"] / HBM_STORE_TBS, 4)
        bt, how, bp = [], None, None
        for _ in range(args.baseline_repeats):
            t0 = time.perf_counter()
            phi = e.x_to_phi(x)
            t1 = time.perf_counter()
            bp, how = _host_qr(phi, K)
            bt.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
            if how.startswith("numpy"):
                break
        tot = [a + b for a, b in bt]
        i = int(np.argsort(tot)[len(tot) // 2])
        out["baseline"] = {"how": how, "ms_median": round(tot[i], 2), "x_to_phi_to_host_ms": round(bt[i][0], 2), "host_qr_ms": round(bt[i][1], 2),
                           "repeats": len(bt)}
        out["baseline_over_device"] = round(tot[i] / ms, 1)
        out["pivots_equal_to_baseline"] = int(np.sum(piv == bp))      # (a dense mesh has near-ties: information, not a check)
        res["cases"].append(out)
        print("%s: device %.3f ms, baseline %.1f ms (%s)" % (name, ms, tot[i], how), file=sys.stderr, flush=True)
        for d in (d_x, d_p, d_d):
            d.free()
        e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
