"""Cost of low-magnitude pruning (nif_amd.sparsity, k_prune.hip) on the training step.

    python tools/bench_pruning.py [--steps K] [--warmup W] [--ramp-steps R] [--rounds N] [--epochs0 E] [--turns T]

* configs[1] (bench.py's workload, 2^20 points): nif_loss_grad_dev + nif_adam_step_dev, against the same step behind nif_prune_apply
  (a non-turn step of a pruned fit); the two alternate, `--rounds` times, medians reported.  A pruning turn: nif_prune_update +
  nif_prune_apply between two synchronisations, by stream events, median of `--turns`.
* configs[0] (tutorial NIF 2x32 / 2x32, 10 000 points, batch 512 = 20 steps per epoch): Model.fit eager (the default), unpruned against
  pruned with ConstantSparsity(0.5, 0, frequency=100) -- a turn every 100 steps -- alternating, `--epochs0` timed epochs each.
* select: one synthetic segment of 16 M floats (N(0, 0.1)): nif_prune_update (three histogram + pick passes and the mask build) and
  nif_prune_apply by stream events; bytes/s count 4 B per entry per digit pass, 4 B read + 1 B written by the mask build, 4 + 1 + 4 B by
  the apply.

One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def _events(e, fn, n):
    out = []
    for _ in range(n):
        e.sync()
        e.timer_start()
        fn()
        out.append(e.timer_stop())
    return float(np.median(out)), out


def configs1(nif_amd, args):
    import bench
    from nif_amd import sparsity as S
    B = args.points
    nif_amd.set_seed(1)
    m = nif_amd.NIFMultiScale(bench.CFG_SHAPE, bench.CFG_PARAM)
    base = m.build()
    e = m._engine
    segs = S._segments(m._spec)
    x, y = nif_amd.data.synthetic_wave_batch(B, seed=100)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    e.reserve(B, 0)
    e.prune_config([o for _, o, _ in segs], [n for _, _, n in segs])
    w0 = e.get_flat()
    z = np.zeros_like(w0)
    adam = nif_amd.Adam(1e-3).as_struct()

    def run(pruned, n):
        for _ in range(n):
            if pruned:
                e.prune_apply()
            e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
            e.adam_step_dev(adam)

    times = {"unpruned": [], "pruned": []}
    for _ in range(args.rounds):
        for kind in ("unpruned", "pruned"):
            e.set_flat(w0); e.set_opt_state(z, z, 0)
            run(kind == "pruned", args.ramp_steps)
            run(kind == "pruned", args.warmup)
            e.sync()
            t0 = time.perf_counter()
            run(kind == "pruned", args.steps)
            e.sync()
            times[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
    ks = [S.keep_count(n, 0.5) for _, _, n in segs]
    turn, turns = _events(e, lambda: (e.prune_update(ks), e.prune_apply()), args.turns)
    med = {k: float(np.median(v)) for k, v in times.items()}
    del base
    return {"ms_per_step": med, "rounds": times, "rel_pruned": med["pruned"] / med["unpruned"] - 1.0,
            "turn_ms": turn, "turn_ms_all": turns, "turn_amortised_per_100_steps_rel": turn / 100.0 / med["unpruned"],
            "prunable_entries": int(sum(n for _, _, n in segs)), "segments": len(segs)}


def configs0(nif_amd, args):
    from nif_amd import sparsity as S
    from oracle import nif_oracle as O
    cs = {"input_dim": 1, "output_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    cp = {"input_dim": 1, "latent_dim": 1, "units": 32, "nlayers": 2, "activation": "swish"}
    x, y = O.synthetic_wave_batch(10000, seed=0)
    runs = {"unpruned": [], "pruned": []}
    for _ in range(args.rounds):
        for kind in ("unpruned", "pruned"):
            nif_amd.set_seed(4)
            m = nif_amd.NIF(cs, cp)
            model = m.build()
            cbs = []
            if kind == "pruned":
                model = S.prune_low_magnitude(model, pruning_schedule=S.ConstantSparsity(0.5, 0, frequency=100))
                cbs = [S.UpdatePruningStep()]
            model.compile(nif_amd.Adam(1e-3), "mse")
            model.fit(x, y, epochs=2, batch_size=512, shuffle=False, verbose=0, callbacks=cbs)
            t0 = time.perf_counter()
            model.fit(x, y, epochs=args.epochs0, batch_size=512, shuffle=False, verbose=0, callbacks=cbs)
            runs[kind].append((time.perf_counter() - t0) / (args.epochs0 * 20) * 1e3)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    return {"ms_per_step": med, "rounds": runs, "rel_pruned": med["pruned"] / med["unpruned"] - 1.0}


def select(nif_amd, args):
    cs = {"input_dim": 1, "output_dim": 1, "units": 128, "nlayers": 16, "use_resblock": False, "connectivity": "full",
          "omega_0": 30.0, "weight_init_factor": 0.01}
    cp = {"input_dim": 1, "latent_dim": 64, "units": 16, "nlayers": 1, "activation": "swish", "use_resblock": False, "omega_0": 30.0}
    nif_amd.set_seed(0)
    m = nif_amd.NIFMultiScale(cs, cp)
    e = m._engine
    n = 16 * (1 << 20)
    assert e.n_params > n + 64
    th = (0.1 * np.random.default_rng(0).standard_normal(e.n_params)).astype(np.float32)
    e.set_flat(th)
    e.prune_config([33], [n])
    k = n // 2
    e.prune_update([k])                  # (first use)
    upd, upd_all = _events(e, lambda: e.prune_update([k]), args.turns)
    app, app_all = _events(e, e.prune_apply, args.turns)
    e.prune_config([], [])
    return {"entries": n, "update_ms": upd, "update_ms_all": upd_all, "update_GBps": (3 * 4 + 5) * n / (upd * 1e-3) / 1e9,
            "apply_ms": app, "apply_ms_all": app_all, "apply_GBps": 9 * n / (app * 1e-3) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ramp-steps", type=int, default=40)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs0", type=int, default=20)
    ap.add_argument("--turns", type=int, default=20)
    ap.add_argument("--only", choices=["configs1", "configs0", "select"], default=None)
    args = ap.parse_args()
    import nif_amd
    res = {"metric": "ms"}
    if args.only in (None, "select"):
        res["select_16M"] = select(nif_amd, args)
    if args.only in (None, "configs1"):
        res["configs1"] = configs1(nif_amd, args)
    if args.only in (None, "configs0"):
        res["configs0"] = configs0(nif_amd, args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
