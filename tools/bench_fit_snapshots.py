"""Milliseconds per loss-and-gradient call of the snapshot-wise training step (nif_snapshot_loss_grad_dev, csrc/k_snapfit.hip) against the
point-wise step (nif_loss_grad_dev) on the expanded table [repeat(p, M) | tile(x, T)] at the same T M, in one process on one GPU:
  * nets: configs[3]'s 128 x 6 (r = 10, si = so = 3, pi = 1) and 256 x 6 of the last-layer class;
  * sizes: T = 512, M = 4096 and T = 64, M = 32768 (2^21 samples each).
The clock is ramped with untimed calls, then the median of `--steps` host-synchronised calls is taken.  A second, untimed-by-the-host
run under the library's profiler gives the split of the snapshot call from its event pairs: phi forward (snet_fwd), head (snet; on
the wide route the adjoint sweep's launches land in this group too), ShapeNet adjoint + reductions (gw), ParameterNet (pnet_fwd +
pnet_bwd) and the row reduction.  The head's bytes per sample are what it must move -- y once, this mesh tile's share of dL/da -- set
against the read bandwidth the project measured.

The two sides run separately, so that the point-wise side can come from another build (the parent commit's, whose step this one does
not change): run `--side pointwise --out pw.json` in that checkout, then `--side snapshots --pointwise pw.json --out
profiles/fit_snapshots.json` here.  Without --pointwise the point-wise side is measured on this build.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS_MEASURED = 6.29             # DESIGN: the read bandwidth measured on this machine
NETS = [("ll_128x6_configs3", 128, 6), ("ll_256x6", 256, 6)]
SIZES = [(512, 4096), (64, 32768)]
R, SI, SO, PI = 10, 3, 3, 1


def _cfgs(n, L):
    cs = {"input_dim": SI, "output_dim": SO, "units": n, "nlayers": L, "use_resblock": False, "connectivity": "last_layer",
          "omega_0": 30.0, "weight_init_factor": 0.01}
    cp = {"input_dim": PI, "latent_dim": R, "units": 32, "nlayers": 2, "activation": "swish", "use_resblock": False, "omega_0": 30.0}
    return cs, cp


def _problem(T, M):
    rng = np.random.default_rng(0)
    p = rng.uniform(-1.0, 1.0, size=(T, PI)).astype(np.float32)
    x = rng.uniform(-1.0, 1.0, size=(M, SI)).astype(np.float32)
    u = np.sin(4.0 * x[None, :, :SO] - p[:, None, :1]).astype(np.float32)
    return p, x, u


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=["snapshots", "pointwise"], default="snapshots")
    ap.add_argument("--pointwise", default=None, help="JSON of a --side pointwise run (another build's)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ramp", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import nif_amd
    res = {"tool": "bench_fit_snapshots", "side": args.side, "steps": args.steps, "ramp": args.ramp, "hbm_tbs": HBM_TBS_MEASURED, "cases": []}
    other = None
    if args.pointwise:
        other = {(c["name"], c["T"], c["M"]): c for c in json.load(open(args.pointwise))["cases"]}
        res["pointwise_from"] = os.path.basename(args.pointwise)
    for name, n, L in NETS:
        for T, M in SIZES:
            nif_amd.set_seed(0)
            cs, cp = _cfgs(n, L)
            m = nif_amd.NIFMultiScaleLastLayerParameterized(cs, cp)
            m.build()
            e = m._engine
            p, x, u = _problem(T, M)
            B = T * M
            out = {"name": name, "units": n, "layers": L, "T": T, "M": M, "samples": B}
            bufs = []

            def dev(a):
                d = e.alloc(a.size); d.upload(a); bufs.append(d)
                return d

            def pointwise():
                table = np.hstack([np.repeat(p, M, axis=0), np.tile(x, (T, 1))]).astype(np.float32)
                d_t, d_y = dev(table), dev(u.reshape(B, SO))
                e.reserve(B)
                ms, ts = _median_ms(lambda: e.loss_grad_dev(d_t.at(0), d_y.at(0), None, B, B), e.sync, args.ramp, args.steps)
                return {"ms_median": round(ms, 4), "ms": ts, "loss": e.grad_read_loss()}

            if args.side == "pointwise":
                out["pointwise"] = pointwise()
            else:
                d_p, d_x, d_u = dev(p), dev(x), dev(u)
                call = lambda: e.snapshot_loss_grad_dev(d_p.at(0), T, d_x.at(0), M, d_u.at(0), None, 0)
                ms, ts = _median_ms(call, e.sync, args.ramp, args.steps)
                out["snapshots"] = {"ms_median": round(ms, 4), "ms": ts, "loss": e.grad_read_loss()}
                e.profile_enable(True)
                e.profile_read(reset=True)
                for _ in range(args.steps):
                    call()
                e.sync()
                prof = e.profile_read(reset=True)
                e.profile_enable(False)
                per = {k: v[0] / args.steps for k, v in prof.items() if v[1]}
                split = {"phi_forward_ms": per.get("snet_fwd", 0.0), "head_ms": per.get("snet", 0.0),
                         "shapenet_adjoint_and_reductions_ms": per.get("gw", 0.0),
                         "parameternet_ms": per.get("pnet_fwd", 0.0) + per.get("pnet_bwd", 0.0), "row_reduction_ms": per.get("reduce", 0.0)}
                out["split"] = {k: round(v, 4) for k, v in split.items()}
                out["split_groups_ms"] = {k: round(v, 4) for k, v in per.items()}
                head_bytes = 4.0 * SO + 4.0 * R / 32.0
                out["head"] = {"bytes_per_sample": head_bytes, "ms_at_measured_bw": round(head_bytes * B / (HBM_TBS_MEASURED * 1e12) * 1e3, 4)}
                if split["head_ms"] > 0 and n <= 128:      # (wide route: the group also holds the adjoint sweep)
                    out["head"]["tbs"] = round(head_bytes * B / (split["head_ms"] * 1e-3) / 1e12, 3)
                    out["head"]["fraction_of_measured_bw"] = round(out["head"]["tbs"] / HBM_TBS_MEASURED, 4)
                pw = other[(name, T, M)]["pointwise"] if other else pointwise()
                out["pointwise"] = pw
                out["pointwise_over_snapshots"] = round(pw["ms_median"] / ms, 2)
            res["cases"].append(out)
            print("%s T=%d M=%d: %s" % (name, T, M, {k: out[k]["ms_median"] for k in ("snapshots", "pointwise") if k in out}),
                  file=sys.stderr, flush=True)
            for d in bufs:
                d.free()
            e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
