"""Milliseconds per training step and per forward pass of the last-layer class with a ShapeNet wider than 128 units (csrc/k_wide.hip),
in one process on one GPU, with the roofline figures beside them:
  * 256 x 6, r = 10, si = so = 3 (configs[3]'s shape at twice its width) at 2^19 and 2^21 points; 512 x 4 at 2^19;
  * configs[3]'s own 128 x 6 on the unchanged k_snet4<.., LL> path at 2^19 points, the yardstick.
A step is nif_loss_grad_dev + nif_adam_step_dev on a resident batch, a forward nif_forward_dev; the clock is ramped with untimed
repetitions first, then the median of `--steps` host-synchronised repetitions is taken.  FLOP / point is the algorithmic count of the
ShapeNet, 2 (si n + L n^2 + n r so) forward and three times that for the step; HBM bytes / point is what the layer-at-a-time
formulation moves if every activation, cosine and adjoint row crosses HBM once per launch that reads or writes it (fp32).  Prints one
JSON line and, with --out, writes it to a file.

    python tools/bench_wide_ll.py --out profiles/wide_ll.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MATRIX_TFLOPS = 157.0      # MI355X, f32-input MFMA
HBM_TBS_MEASURED = 6.29             # DESIGN: the read bandwidth measured on this machine

CASES = [      # name, units, layers, points
    ("ll_128x6_yardstick", 128, 6, 1 << 19),
    ("ll_256x6", 256, 6, 1 << 19),
    ("ll_256x6", 256, 6, 1 << 21),
    ("ll_512x4", 512, 4, 1 << 19),
]
R, SI, SO, PI = 10, 3, 3, 1


def _cfgs(n, L):
    cs = {"input_dim": SI, "output_dim": SO, "units": n, "nlayers": L, "use_resblock": False, "connectivity": "last_layer",
          "omega_0": 30.0, "weight_init_factor": 0.01}
    cp = {"input_dim": PI, "latent_dim": R, "units": 32, "nlayers": 2, "activation": "swish", "use_resblock": False, "omega_0": 30.0}
    return cs, cp


def flop_per_point(n, L):
    return 2 * (SI * n + L * n * n + n * R * SO)


def hbm_bytes_per_point(n, L):
    """(forward, step) of the layer-at-a-time formulation: rows read + rows written per launch, 4 bytes each"""
    sop = R * SO
    fwd = (SI + n) + L * 2 * n + (n + sop)
    fwd_train = (SI + 2 * n) + L * 3 * n + (n + sop)                 # + the cosine of every sine layer
    adj = (sop + 2 * n) + L * 3 * n                                  # dL/da in, cosine in, dL/da out, per matrix with a layer below
    gw = (SI + n) + L * 2 * n + (n + sop)                            # layer input + dL/da, once per layer
    return 4 * fwd, 4 * (fwd_train + adj + gw)


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
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ramp", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import nif_amd
    adam = nif_amd.Adam(1e-4).as_struct()
    res = {"tool": "bench_wide_ll", "steps": args.steps, "ramp": args.ramp, "peak_f32_matrix_tflops": PEAK_F32_MATRIX_TFLOPS,
           "hbm_tbs": HBM_TBS_MEASURED, "cases": []}
    yard = None
    for name, n, L, B in CASES:
        nif_amd.set_seed(0)
        cs, cp = _cfgs(n, L)
        m = nif_amd.NIFMultiScaleLastLayerParameterized(cs, cp)
        m.build()
        e = m._engine
        rng = np.random.default_rng(0)
        x = rng.uniform(-1.0, 1.0, size=(B, PI + SI)).astype(np.float32)
        y = np.sin(4.0 * x[:, 1:1 + SO] - x[:, 0:1]).astype(np.float32)
        d_x, d_y, d_u = e.alloc(x.size), e.alloc(y.size), e.alloc(B * SO)
        d_x.upload(x); d_y.upload(y)
        e.reserve(B)

        def step():
            e.loss_grad_dev(d_x.at(0), d_y.at(0), None, B, B)
            e.adam_step_dev(adam)

        def fwd():
            e.forward_dev(d_x.at(0), B, d_u.at(0))

        ramp = args.ramp * (10 if n <= 128 else 1)
        ms_step, ts_step = _median_ms(step, e.sync, ramp, args.steps)
        ms_fwd, ts_fwd = _median_ms(fwd, e.sync, ramp, args.steps)
        f = flop_per_point(n, L)
        hb_f, hb_s = hbm_bytes_per_point(n, L)
        out = {"name": name, "units": n, "layers": L, "points": B, "loss_after": e.last_loss(),
               "step": {"ms_median": round(ms_step, 3), "ms": ts_step, "points_per_s": round(B / (ms_step * 1e-3)),
                        "flop_per_point": 3 * f, "tflops": round(3 * f * B / (ms_step * 1e-3) / 1e12, 2),
                        "fraction_of_f32_matrix_peak": round(3 * f * B / (ms_step * 1e-3) / 1e12 / PEAK_F32_MATRIX_TFLOPS, 4)},
               "forward": {"ms_median": round(ms_fwd, 3), "ms": ts_fwd, "points_per_s": round(B / (ms_fwd * 1e-3)),
                           "flop_per_point": f, "tflops": round(f * B / (ms_fwd * 1e-3) / 1e12, 2),
                           "fraction_of_f32_matrix_peak": round(f * B / (ms_fwd * 1e-3) / 1e12 / PEAK_F32_MATRIX_TFLOPS, 4)}}
        if n > 128:      # (the fused 128-wide kernel keeps its layers on chip: the count does not describe it)
            out["step"]["hbm_bytes_per_point"] = hb_s
            out["step"]["hbm_ms_at_measured_bw"] = round(hb_s * B / (HBM_TBS_MEASURED * 1e12) * 1e3, 3)
            out["forward"]["hbm_bytes_per_point"] = hb_f
            out["forward"]["hbm_ms_at_measured_bw"] = round(hb_f * B / (HBM_TBS_MEASURED * 1e12) * 1e3, 3)
        if yard is None:
            yard = out
        else:
            out["step_ms_over_yardstick_per_point"] = round((ms_step / B) / (yard["step"]["ms_median"] / yard["points"]), 2)
            out["forward_ms_over_yardstick_per_point"] = round((ms_fwd / B) / (yard["forward"]["ms_median"] / yard["points"]), 2)
        res["cases"].append(out)
        print("%s n=%d L=%d B=%d: step %.3f ms, forward %.3f ms" % (name, n, L, B, ms_step, ms_fwd), file=sys.stderr, flush=True)
        for d in (d_x, d_y, d_u):
            d.free()
        e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
