"""Per-step cost of the gradient transform (k_gradtf.hip): Adam with global_clipnorm on against Adam without a transform.

    python tools/bench_gradtf.py [--steps K] [--warmup W] [--ramp-steps R] [--rounds N] [--epochs0 E] [--only configs1|configs0]

* configs[1] (bench.py's workload: NIFMultiScale, ShapeNet 4x64 SIREN, 2^20 points): nif_loss_grad_dev + nif_adam_step_dev; off = the
  fused reduce-and-update launch, on = k_reduce + k_gt_reduce + k_gt_apply + k_opt.  The two take turns, `--rounds` rotations, medians.
* configs[0] (tutorial NIF 2x32 / 2x32, 10 000 points, batch 512 = 20 steps per epoch): eager Model.fit, a 2-epoch fit first, then
  `--epochs0` timed epochs.

One JSON line on stdout.  The launch list of a step comes from a kernel trace of a run of its own:
rocprofv3 --kernel-trace --stats -- python tools/bench_gradtf.py --only configs1 --rounds 1"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MODES = ("off", "global_clipnorm")


def configs1(nif_amd, args):
    import bench
    from nif_amd.engine import DeviceArray
    B = args.points
    nif_amd.set_seed(1)
    m = nif_amd.NIFMultiScale(bench.CFG_SHAPE, bench.CFG_PARAM)
    m.build()
    e = m._engine
    x, y = nif_amd.data.synthetic_wave_batch(B, seed=100)
    d_x, d_y = DeviceArray(e, x.size), DeviceArray(e, y.size)
    d_x.upload(x); d_y.upload(y)
    e.reserve(B, 0)
    w0 = e.get_flat()
    z = np.zeros_like(w0)
    adam = nif_amd.Adam(1e-3).as_struct()
    times = {k: [] for k in MODES}

    def run(n):
        for _ in range(n):
            e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
            e.adam_step_dev(adam)

    for _ in range(args.rounds):
        for mode in MODES:
            e.set_flat(w0); e.set_opt_state(z, z, 0)
            e.set_grad_transform(None if mode == "off" else {"global_clipnorm": 1e-3})
            run(args.ramp_steps)
            run(args.warmup)
            e.sync()
            t0 = time.perf_counter()
            run(args.steps)
            e.sync()
            times[mode].append((time.perf_counter() - t0) / args.steps * 1e3)
    e.set_grad_transform(None)
    return {k: float(np.median(v)) for k, v in times.items()}, times, e.n_params


def configs0(nif_amd, args):
    from oracle import nif_oracle as O
    cs = {"input_dim": 1, "output_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    cp = {"input_dim": 1, "latent_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    x, y = O.synthetic_wave_batch(10000, seed=0)
    runs = {k: [] for k in MODES}
    for _ in range(args.rounds):
        for mode in MODES:
            nif_amd.set_seed(4)
            m = nif_amd.NIF(cs, cp)
            model = m.build()
            model.compile(nif_amd.Adam(1e-3) if mode == "off" else nif_amd.Adam(1e-3, global_clipnorm=1e-2), "mse")
            model.fit(x, y, epochs=2, batch_size=512, shuffle=False, verbose=0)
            t0 = time.perf_counter()
            model.fit(x, y, epochs=args.epochs0, batch_size=512, shuffle=False, verbose=0)
            runs[mode].append((time.perf_counter() - t0) / (args.epochs0 * 20) * 1e3)
    return {k: float(np.median(v)) for k, v in runs.items()}, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ramp-steps", type=int, default=40)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs0", type=int, default=20)
    ap.add_argument("--only", choices=["configs1", "configs0"], default=None)
    args = ap.parse_args()
    import nif_amd
    res = {"metric": "ms_per_step", "modes": list(MODES)}
    if args.only in (None, "configs1"):
        c1, r1, P = configs1(nif_amd, args)
        res.update(configs1_ms_per_step=c1, configs1_rounds=r1, configs1_params=P,
                   configs1_added_ms=c1["global_clipnorm"] - c1["off"])
    if args.only in (None, "configs0"):
        c0, r0 = configs0(nif_amd, args)
        res.update(configs0_eager_ms_per_step=c0, configs0_rounds=r0, configs0_added_ms=c0["global_clipnorm"] - c0["off"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
