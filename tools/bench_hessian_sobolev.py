"""ms per step and points/s of the second-order Sobolev step (SobolevModel over a HessianLayer: nif_sobolev2_loss_grad_dev) next to the
first-order one (JacobianLayer: nif_sobolev_loss_grad_dev_y) at configs[4]'s shape: NIFMultiScale, ShapeNet 4 x 64 SIREN, two
coordinates, 2^20 points, fp32.  Both in the same run, each timed on the host around `--steps` steps after `--warmup` (the engine's
stream drained before and after); one JSON line.
    python tools/bench_hessian_sobolev.py [--points 1048576] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import time
    import nif_amd
    from nif_amd.engine import DeviceArray
    cs = {"input_dim": 2, "output_dim": 1, "units": 64, "nlayers": 4, "use_resblock": False, "connectivity": "full",
          "omega_0": 30.0, "weight_init_factor": 0.01}
    cp = {"input_dim": 1, "latent_dim": 1, "units": 32, "nlayers": 2, "activation": "swish", "use_resblock": False,
          "omega_0": 30.0}
    nif_amd.set_seed(0)
    m = nif_amd.NIFMultiScale(cs, cp)
    m.build()
    e = m._engine
    B, xi = a.points, [1, 2]
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (B, 3)).astype(np.float32)
    y = rng.standard_normal((B, 1)).astype(np.float32)
    g = rng.standard_normal((B, 1, 2)).astype(np.float32)
    t = rng.standard_normal((B, 1, 2, 2)).astype(np.float32)
    d = [DeviceArray(e, v.size) for v in (x, y, g, t)]
    for dv, v in zip(d, (x, y, g, t)):
        dv.upload(v)
    e.reserve(B, 3)
    steps = {
        "hessian_sobolev": lambda: e.sobolev2_loss_grad_dev(d[0].at(0), d[1].at(0), d[2].at(0), d[3].at(0), None, B, B, xi, 0.1, 0.01),
        "jacobian_sobolev": lambda: e.sobolev_loss_grad_dev(d[0].at(0), d[1].at(0), d[2].at(0), None, B, B, xi, 0.1),
    }
    out = {"shape": "NIFMultiScale 4x64 SIREN, x_index [1, 2], fp32", "points": B, "steps": a.steps}
    for name, step in steps.items():
        for _ in range(a.warmup):
            step()
        e.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        e.sync()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        out[name] = {"ms_per_step": round(ms, 4), "points_per_s": round(B / (ms * 1e-3), 1)}
    out["ratio"] = round(out["hessian_sobolev"]["ms_per_step"] / out["jacobian_sobolev"]["ms_per_step"], 3)
    for dv in d:
        dv.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
