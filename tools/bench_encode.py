"""The normal-equation pass of Model.encode_snapshots (nif_snapshot_normal_eq_dev) on device-resident samples: report only,
there is no predecessor to hold it against.

    T = 512 snapshots x 4096 points of a shared mesh, on the ms_cfg2_64x4 net (latent_dim 1) and on the same net at latent_dim 3.
    call_ms        median of 10 calls, host clock around the call and a stream synchronise (3 warm-up calls)
    jac_ms etc.    the same calls split by the library's event pairs (nif_profile_*): the k_jac launches (ceil(r / 3) of them),
                   the Gram reducer, the expand kernel
    reducer_bytes  the reducer's algorithmic traffic, 4 so (r + 1) bytes per point (J and u; y and w come on top), over its time,
                   against the 6.29 TB/s measured HBM peak
    jacobian_*     for context: nif_jacobian (host entry: staging copies included) on 2^17 points of the same net, one parameter
                   column, per point

    python tools/bench_encode.py [--out profiles/encode.json]
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

HBM_PEAK = 6.29e12
T, M, WARMUP, ITERS = 512, 4096, 3, 10


def net(r):
    cs = {"input_dim": 1, "output_dim": 1, "units": 64, "nlayers": 4, "use_resblock": False, "connectivity": "full",
          "omega_0": 30.0, "weight_init_factor": 0.01}
    cp = {"input_dim": 1, "latent_dim": r, "units": 32, "nlayers": 2, "activation": "sine", "use_resblock": False, "omega_0": 30.0}
    return cs, cp


def run_case(name, r):
    import nif_amd
    from nif_amd import _lib
    nif_amd.set_seed(0)
    m = nif_amd.NIFMultiScale(*net(r))
    m.build()
    e, s = m._engine, m._spec
    so = s.so_dim
    rng = np.random.default_rng(1)
    p = rng.uniform(-1, 1, size=(T, s.pi_dim)).astype(np.float32)
    lat = e.p_to_lr(p)
    x = rng.uniform(-1, 1, size=(M, s.si_dim)).astype(np.float32)
    y = rng.uniform(-1, 1, size=(T, M, so)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=(T, M)).astype(np.float32)
    samples = e.snapshot_samples(x, y, w)
    d_l, d_s = e.alloc(lat.size), e.alloc(2 * T * (r + 1) ** 2)
    d_l.upload(lat)
    a = samples.args(d_l, d_s)

    def call():
        _lib.check(e.lib.nif_snapshot_normal_eq_dev(C.byref(a)))
        e.sync()

    for _ in range(WARMUP):
        call()
    e.profile_enable(True)
    e.profile_read(reset=True)
    times = []
    for _ in range(ITERS):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    prof = e.profile_read(reset=True)
    e.profile_enable(False)
    per = {k: prof[k][0] / ITERS for k in ("snet_fwd", "reduce", "pack")}
    n = T * M
    red_bytes = 4.0 * so * (r + 1) * n
    bw = red_bytes / (per["reduce"] * 1e-3)
    # context: JacobianLayer w.r.t. one parameter column on the same net
    B = 1 << 17
    inp = rng.uniform(-1, 1, size=(B, s.pi_dim + s.si_dim)).astype(np.float32)
    e.jacobian(inp, [0], [0])
    jt = []
    for _ in range(5):
        t0 = time.perf_counter()
        e.jacobian(inp, [0], [0])
        jt.append((time.perf_counter() - t0) * 1e3)
    samples.free(); d_l.free(); d_s.free()
    return {"name": name, "latent_dim": r, "T": T, "M": M, "points": n, "call_ms": float(np.median(times)),
            "call_minmax_ms": [float(min(times)), float(max(times))], "ns_per_point": float(np.median(times)) * 1e6 / n,
            "jac_ms": per["snet_fwd"], "jac_launches": (r + 2) // 3, "reducer_ms": per["reduce"], "expand_ms": per["pack"],
            "reducer_bytes": red_bytes, "reducer_bytes_per_s": bw, "reducer_share_of_hbm_peak": bw / HBM_PEAK,
            "jacobian_host_call_ms": float(np.median(jt)), "jacobian_points": B, "jacobian_ns_per_point": float(np.median(jt)) * 1e6 / B}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = []
    for name, r in (("ms_cfg2_64x4_r1", 1), ("ms_cfg2_64x4_r3", 3)):
        res.append(run_case(name, r))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"protocol": "%d warm-up + %d timed calls of nif_snapshot_normal_eq_dev, host clock around call + stream synchronise, "
                                   "medians; the split from the library's event pairs over the same calls" % (WARMUP, ITERS),
                       "cases": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
