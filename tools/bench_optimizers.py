"""Per-step time of the training step with each optimizer of the hot path: Adam, Lion, AdaBelief, AdaBelief with amsgrad.

    python tools/bench_optimizers.py [--steps K] [--warmup W] [--ramp-steps R] [--rounds N] [--epochs0 E]

* configs[1] (bench.py's workload: NIFMultiScale, ShapeNet 4x64 SIREN, 2^20 points): nif_loss_grad_dev + the update, the row reduction
  fused with the update (fuse_tail, the default), bench.py's clock ramp / warm-up / timed steps; the optimizers take turns, `--rounds`
  rotations, the median per optimizer.
* configs[0] (tutorial NIF 2x32 / 2x32, 10 000 points, batch 512 = 20 steps per epoch): Model.fit with the epochs replayed as captured
  graphs (model._graph_epochs), a 2-epoch fit first (capture + warm clocks), then `--epochs0` timed epochs.

One JSON line on stdout.  Launch counts per step come from a kernel trace of a run of its own:
rocprofv3 --kernel-trace --stats -- python tools/bench_optimizers.py ..."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KINDS = ("adam", "lion", "adabelief", "adabelief_amsgrad")


def _opt(nif_amd, kind):
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    return {"adam": lambda: nif_amd.Adam(1e-3), "lion": lambda: Lion(1e-4), "adabelief": lambda: AdaBeliefOptimizer(1e-3),
            "adabelief_amsgrad": lambda: AdaBeliefOptimizer(1e-3, amsgrad=True)}[kind]()


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
    times = {k: [] for k in KINDS}

    def run(kind, n):
        o = _opt(nif_amd, kind)
        if kind == "adam":
            s = o.as_struct()
            for _ in range(n):
                e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
                e.adam_step_dev(s)
        else:
            s = o.as_opt()
            for _ in range(n):
                e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
                e.opt_step_dev(s)

    for _ in range(args.rounds):
        for kind in KINDS:
            e.set_flat(w0); e.set_opt_state(z, z, 0); e.set_opt_slot(2, z)
            run(kind, args.ramp_steps)
            run(kind, args.warmup)
            e.sync()
            t0 = time.perf_counter()
            run(kind, args.steps)
            e.sync()
            times[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
    return {k: float(np.median(v)) for k, v in times.items()}, times


def configs0(nif_amd, args):
    from oracle import nif_oracle as O
    cs = {"input_dim": 1, "output_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    cp = {"input_dim": 1, "latent_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    x, y = O.synthetic_wave_batch(10000, seed=0)
    out, runs = {}, {k: [] for k in KINDS}
    for _ in range(args.rounds):
        for kind in KINDS:
            nif_amd.set_seed(4)
            m = nif_amd.NIF(cs, cp)
            model = m.build()
            model._graph_epochs = True
            model.compile(_opt(nif_amd, kind), "mse")
            model.fit(x, y, epochs=2, batch_size=512, shuffle=False, verbose=0)
            t0 = time.perf_counter()
            model.fit(x, y, epochs=args.epochs0, batch_size=512, shuffle=False, verbose=0)
            runs[kind].append((time.perf_counter() - t0) / (args.epochs0 * 20) * 1e3)
    for k, v in runs.items():
        out[k] = float(np.median(v))
    return out, runs


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
    res = {"metric": "ms_per_step", "kinds": list(KINDS)}
    if args.only in (None, "configs1"):
        c1, r1 = configs1(nif_amd, args)
        res["configs1_ms_per_step"] = c1
        res["configs1_rounds"] = r1
        res["configs1_rel_to_adam"] = {k: c1[k] / c1["adam"] - 1.0 for k in KINDS}
    if args.only in (None, "configs0"):
        c0, r0 = configs0(nif_amd, args)
        res["configs0_graph_ms_per_step"] = c0
        res["configs0_rounds"] = r0
        res["configs0_rel_to_adam"] = {k: c0[k] / c0["adam"] - 1.0 for k in KINDS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
