"""Milliseconds per L-BFGS closure evaluation, float32 against float64, in one process on one GPU:
  * configs[1]: NIFMultiScale ShapeNet 4 x 64 SIREN, 2^20 points (bench.py's model);
  * configs[0]: class NIF 2 x 32 + 2 x 32, 10 000 points.
An evaluation is what TFPLBFGS._f does: parameters up, loss + gradient on the resident table, P + 1 numbers back.  The clock is ramped
with untimed evaluations first (bench.py's clock_ramp_steps), then the median of `--evals` timed ones is taken, host wall time around
the synchronising read-out.  Prints one JSON line and, with --out, writes it to a file.

    python tools/bench_lbfgs_f64.py --out profiles/lbfgs_f64.json
    python tools/bench_lbfgs_f64.py --only cfg1 --dtype float64 --evals 3        # (the form a kernel trace is taken of)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLOP_PER_POINT_CFG1 = 198144       # DESIGN's algorithmic count for configs[1] (forward + adjoint + weight gradients)


def _models():
    import bench
    cs0 = {"input_dim": 1, "output_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    cp0 = {"input_dim": 1, "latent_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    return {"cfg1": ("NIFMultiScale", bench.CFG_SHAPE, bench.CFG_PARAM, 1 << 20), "cfg0": ("NIF", cs0, cp0, 10000)}


def _time(f, theta, ramp, evals):
    for _ in range(ramp):
        f(theta)
    ts = []
    for _ in range(evals):
        t0 = time.perf_counter()
        f(theta)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 4) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=10)
    ap.add_argument("--ramp32", type=int, default=40, help="untimed float32 evaluations in front (clock ramp)")
    ap.add_argument("--ramp64", type=int, default=3, help="untimed float64 evaluations in front")
    ap.add_argument("--only", choices=["cfg0", "cfg1"], default=None)
    ap.add_argument("--dtype", choices=["float32", "float64"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import nif_amd
    from nif_amd.optimizers import TFPLBFGS
    res = {"tool": "bench_lbfgs_f64", "evals": args.evals, "configs": {}}
    for name, (kind, cs, cp, B) in _models().items():
        if args.only and name != args.only:
            continue
        nif_amd.set_seed(0)
        model = getattr(nif_amd, kind)(cs, cp).build()
        rng = np.random.default_rng(0)
        x = rng.uniform(-1.0, 1.0, size=(B, 2))
        y = np.sin(4.0 * x[:, 1:2] - x[:, 0:1])
        out = {"points": B}
        for dtype, ramp in (("float32", args.ramp32), ("float64", args.ramp64)):
            if args.dtype and dtype != args.dtype:
                continue
            t = TFPLBFGS(model, "mse", x, y, display_epoch=1 << 62, dtype=dtype)
            med, ts = _time(t._f, t._start(), ramp, args.evals)
            out[dtype] = {"ms_per_eval_median": round(med, 4), "ms": ts, "ramp_evals": ramp}
        if "float32" in out and "float64" in out:
            out["ratio_f64_over_f32"] = round(out["float64"]["ms_per_eval_median"] / out["float32"]["ms_per_eval_median"], 2)
        if name == "cfg1" and "float64" in out:
            out["f64_algorithmic_tflops"] = round(FLOP_PER_POINT_CFG1 * B / (out["float64"]["ms_per_eval_median"] * 1e-3) / 1e12, 3)
        res["configs"][name] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
