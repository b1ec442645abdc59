"""A/B of the alternative kernel paths on identical inputs, each in its own process (the switches are read once):
bf16-split products (k_snet4, default) vs f32-input MFMAs (NIF_FP32_MFMA=1 -> k_snet3), and the stash-free
ParameterNet adjoint (k_pnet_bwg, default) vs the stash path (NIF_PNET_STASH=1), LDS-DMA vs register-load
weight-gradient kernels (NIF_GW_LDS=0).  All must agree with the fp64
oracle to the parity bar AND with each other far inside it -- the split products are an fp32-exact reformulation,
not a lower-precision mode."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import nif_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import bench, nif_amd
from oracle import nif_oracle as O
out = sys.argv[1]
spec = O.Spec("NIFMultiScale", bench.CFG_SHAPE, bench.CFG_PARAM)
rng = np.random.default_rng(5)
ws = O.init_weights(spec, rng, dtype=np.float32)
names = [nm for nm, _ in spec.param_shapes()]
ws[names.index("pnet_last_w")] = (ws[names.index("pnet_last_w")] * 2.0).astype(np.float32)
m = nif_amd.NIFMultiScale(bench.CFG_SHAPE, bench.CFG_PARAM)
model = m.build(); model.set_weights(ws)
x, y = nif_amd.data.synthetic_wave_batch(20000, seed=3)
u = model.predict(x)
loss, grad = m._engine.loss_and_grad(x, y, None)
np.savez(out, u=u, loss=np.float64(loss), grad=grad, x=x, y=y, **{"w%%d" %% i: w for i, w in enumerate(ws)})
''' % ROOT


def _run(tmp_path, tag, env_extra):
    out = str(tmp_path / (tag + ".npz"))
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", SCRIPT, out], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    return np.load(out)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def test_bf16_split_and_fp32_mfma_paths_agree(tmp_path):
    a = _run(tmp_path, "split", {"NIF_FP32_MFMA": "0", "NIF_PNET_STASH": "0"})
    b = _run(tmp_path, "fp32", {"NIF_FP32_MFMA": "1", "NIF_PNET_STASH": "1"})
    # weight-gradient kernels with register loads (k_gw_mfma / k_gw_first_mfma / k_gw_out) instead of the LDS-DMA forms
    d = _run(tmp_path, "gwreg", {"NIF_GW_LDS": "0"})
    assert _rel(d["u"], a["u"]) == 0.0 and _rel(d["grad"], a["grad"]) < 2e-5, _rel(d["grad"], a["grad"])
    # the two GPU formulations against each other
    assert _rel(a["u"], b["u"]) < 2e-6, _rel(a["u"], b["u"])
    assert abs(float(a["loss"]) - float(b["loss"])) <= 2e-6 * abs(float(b["loss"]))
    assert _rel(a["grad"], b["grad"]) < 5e-5, _rel(a["grad"], b["grad"])
    # and each against the fp64 oracle (same weights, same inputs)
    import bench
    spec = O.Spec("NIFMultiScale", bench.CFG_SHAPE, bench.CFG_PARAM)
    ws = [a["w%d" % i].astype(np.float64) for i in range(len(spec.param_shapes()))]
    ref = O.forward(spec, ws, a["x"].astype(np.float64))
    rl, rg = O.loss_and_grad(spec, ws, a["x"].astype(np.float64), a["y"].astype(np.float64))
    for d in (a, b):
        assert _rel(d["u"], ref) < 1e-5, _rel(d["u"], ref)
        assert abs(float(d["loss"]) - rl) <= 1e-5 * abs(rl)
        assert _rel(d["grad"], O.flatten(rg)) < 2e-4, _rel(d["grad"], O.flatten(rg))


# ---- every runtime knob of the library, flipped, against the oracle ------------------------------------------
# The switches are read once per process, so each case runs in a child.  The child computes (loss, flat gradient) of one config with
# the knob set; the parent compares with the fp64 oracle at the parity bars of tests/test_gpu_parity.py.
KNOB_CHILD = r'''
import sys, json, numpy as np
sys.path.insert(0, %r)
import nif_amd
from oracle import nif_oracle as O
from tests.test_gpu_parity import CONFIGS
name, mode, policy, out = sys.argv[1:5]
(kind, cs, cp), B = CONFIGS[name]
spec = O.Spec(kind, cs, cp)
rng = np.random.default_rng(0)
ws = O.init_weights(spec, rng, dtype=np.float32)
names = [nm for nm, _ in spec.param_shapes()]
if kind == "NIFMultiScale":
    ws[names.index("pnet_last_w")] = (ws[names.index("pnet_last_w")] * (1.0 if policy != "float32" else 2.0)).astype(np.float32)
if kind == "NIFMultiScaleLastLayerParameterized":
    ws[names.index("pnet_last_w")] = (ws[names.index("pnet_last_w")] * 30.0).astype(np.float32)
m = getattr(nif_amd, kind)(cs, cp, mixed_policy=policy)
model = m.build(); model.set_weights(ws)
x = rng.uniform(-1, 1, size=(B, spec.pi + spec.si)).astype(np.float32)
y = rng.uniform(-1, 1, size=(B, spec.so)).astype(np.float32)
sw = rng.uniform(0.5, 1.5, size=(B,)).astype(np.float32)
xi = list(range(spec.pi, spec.pi + spec.si))
g = np.random.default_rng(11).uniform(-1, 1, size=(B, spec.so, len(xi))).astype(np.float32)
if mode == "sobolev":
    loss, grad = m._engine.sobolev_loss_and_grad(x, y, g, xi, 0.05, sw)
else:
    loss, grad = m._engine.loss_and_grad(x, y, sw)
np.savez(out, loss=np.float64(loss), grad=grad, x=x, y=y, sw=sw, g=g, **{"w%%d" %% i: w for i, w in enumerate(ws)})
''' % ROOT

KNOBS = [
    # (environment, config, mode, policy)
    ({"NIF_FUSE_GW": "0"}, "ms_cfg2_64x4", "plain", "float32"),            # k_snet4 + k_gw_* instead of the fused-gradient kernel
    ({"NIF_FUSE_GW": "1"}, "ms_cfg2_64x4", "plain", "float32"),
    ({"NIF_SIDE_PNET": "0", "NIF_FUSE_GW": "0"}, "ms_cfg2_64x4", "plain", "float32"),
    ({"NIF_SIDE_PNET": "1", "NIF_FUSE_GW": "0"}, "ms_cfg2_64x4", "plain", "float32"),
    ({"NIF_PBW_TOUCH": "0", "NIF_FUSE_GW": "0"}, "ms_cfg2_64x4", "plain", "float32"),
    ({"NIF_PNET_STASH": "1"}, "ms_cfg3_128x3", "plain", "float32"),        # ParameterNet adjoint through its HBM stash
    ({"NIF_PNET_STASH": "1"}, "ll_plain_32x2_r3", "plain", "float32"),     # ... from the last-layer class's step (gw_pnet_stack's second caller)
    ({"NIF_PNET_STASH": "1"}, "ms_cfg5_64x4_si2", "sobolev", "float32"),   # ... and behind the Sobolev kernel
    ({"NIF_PNET_BF2": "0"}, "ms_cfg3_128x3", "plain", "float32"),          # 64-unit ParameterNet on the f32-input MFMAs
    ({"NIF_GW8": "0"}, "ms_cfg3_128x3", "plain", "float32"),               # 128-wide weight gradients on k_gw_lds<4, 2, 1>
    ({"NIF_GW8": "0", "NIF_GW_LDS": "0"}, "ms_cfg3_128x3", "plain", "float32"),   # ... on the register-load form
    ({"NIF_GW_LDS": "0", "NIF_FUSE_GW": "0"}, "ms_64x2_r1_so5", "plain", "float32"),
    ({"NIF_SOBW": "0"}, "ms_cfg5_64x4_si2", "sobolev", "float32"),         # k_sob instead of the streams-on-waves kernel
    ({"NIF_SOBW": "1"}, "ms_cfg5_64x4_si2", "sobolev", "float32"),
    # r4: k_sobw took over resblock nets, class NIF and the 65..128-unit nets -- k_sob's forms for them stay the fallback (LDS) and A/B path
    ({"NIF_SOBW": "0"}, "ms_res_64x2", "sobolev", "float32"),
    ({"NIF_SOBW": "0"}, "nif_cfg1_32x2", "sobolev", "float32"),
    ({"NIF_SOBW": "0"}, "ms_cfg3_128x3", "sobolev", "float32"),
    ({"NIF_SOBW": "0"}, "ms_res_64x2", "sobolev", "mixed_bfloat16"),
    ({"NIF_LL_MLP": "1"}, "ll_plain_32x2_r3", "plain", "float32"),         # last-layer class on the r1 MLP kernels
    ({"NIF_FP32_MFMA": "1"}, "ms_res_64x2", "plain", "float32"),
    ({"NIF_PIPE_CHUNK": "64", "NIF_FP32_MFMA": "1"}, "ms_cfg2_64x4", "plain", "float32"),   # two-stream chunk pipeline of the k_snet3 path
    ({"NIF_DA_BF16": "0", "NIF_S6_POLICY": "0"}, "ms_cfg2_64x4", "plain", "mixed_bfloat16"),     # fp32 dL/da stash rows under the policy
    ({"NIF_DA_BF16": "1", "NIF_S6_POLICY": "0"}, "ms_cfg2_64x4", "plain", "mixed_bfloat16"),
    ({"NIF_S6_POLICY": "1"}, "ms_cfg2_64x4", "plain", "mixed_bfloat16"),   # late r4: the fused-gradient kernel's policy forms (default)
    ({"NIF_S6_POLICY": "1"}, "ms_cfg2_64x4", "plain", "mixed_float16"),
    ({"NIF_S6_POLICY": "0"}, "ms_cfg2_64x4", "plain", "mixed_float16"),    # k_snet4<.., PR = 2> + the fp32-row reductions
    ({"NIF_DA_BF16": "0"}, "ms_cfg5_64x4_si2", "sobolev", "mixed_bfloat16"),
    ({"NIF_H_PH16": "0"}, "ms_cfg3_128x3", "plain", "mixed_bfloat16"),     # r5: fp32 layer-input stash rows on the 128-wide policy step (default: 16-bit phases)
    ({"NIF_H_PH16": "1"}, "ms_cfg3_128x3", "plain", "mixed_bfloat16"),
    ({"NIF_H_PH16": "0"}, "ll_cfg4_128x2_r10_so3", "plain", "mixed_bfloat16"),
    ({"NIF_SMALL_STEP": "0"}, "nif_cfg1_32x2", "plain", "float32"),        # r6: a small batch on the tile kernels (default: k_small, one launch)
    ({"NIF_SMALL_STEP": "1"}, "nif_cfg1_32x2", "plain", "float32"),
    ({"NIF_SMALL_STEP": "0"}, "nif_pad_n30_tanh_r2_so2", "plain", "float32"),
    ({"NIF_FUSE_TAIL": "0"}, "ms_cfg2_64x4", "plain", "float32"),          # r6: the row reduction inside nif_loss_grad_dev (default: deferred to its consumer)
    ({"NIF_FUSE_TAIL": "0"}, "nif_cfg1_32x2", "plain", "float32"),
]


@pytest.mark.parametrize("case", range(len(KNOBS)), ids=["+".join("%s=%s" % kv for kv in sorted(k[0].items())) + ":" + k[1] for k in KNOBS])
def test_every_runtime_knob_against_the_oracle(case, tmp_path):
    env_extra, name, mode, policy = KNOBS[case]
    from tests.test_gpu_parity import CONFIGS
    out = str(tmp_path / "knob.npz")
    env = dict(os.environ)
    for k in ("NIF_FUSE_GW", "NIF_SIDE_PNET", "NIF_PBW_TOUCH", "NIF_PNET_STASH", "NIF_PNET_BF2", "NIF_GW8", "NIF_GW_LDS", "NIF_SOBW", "NIF_LL_MLP",
              "NIF_FP32_MFMA", "NIF_PIPE_CHUNK", "NIF_DA_BF16", "NIF_S6_POLICY", "NIF_H_PH16", "NIF_SMALL_STEP", "NIF_FUSE_TAIL"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", KNOB_CHILD, name, mode, policy, out], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    d = np.load(out)
    (kind, cs, cp), B = CONFIGS[name]
    spec = O.Spec(kind, cs, cp)
    ws = [d["w%d" % i].astype(np.float64) for i in range(len(spec.param_shapes()))]
    x, y, sw, g = (d[k].astype(np.float64) for k in ("x", "y", "sw", "g"))
    xi = list(range(spec.pi, spec.pi + spec.si))
    if mode == "sobolev":
        rl, rg, _, _ = O.sobolev_loss_and_grad(spec, ws, x, y, g, xi, 0.05, sw)
    else:
        rl, rg = O.loss_and_grad(spec, ws, x, y, sw)
    rg = O.flatten(rg)
    # fp32: the parity bars of test_gpu_parity; mixed_bfloat16: the distance of the policy from exact arithmetic (the cast-for-cast
    # pin of the default path lives in test_gpu_parity; here the knob must not change what is computed)
    lbar, gbar = (2e-5, 3e-4) if policy == "float32" else (2e-2, 0.1)
    assert abs(float(d["loss"]) - rl) <= lbar * abs(rl), (float(d["loss"]), rl)
    off = 0
    for nm, shp in spec.param_shapes():
        k = int(np.prod(shp))
        a, b = d["grad"][off:off + k], rg[off:off + k]
        off += k
        # (the metric of test_loss_and_grad_match_oracle: relative to the tensor, plus 2e-6 of the whole gradient's norm for the
        # tensors that are small against it -- pnet_bottleneck_b of the 128-wide net is 1e-3 of the gradient)
        err = float(np.linalg.norm(a.astype(np.float64) - b))
        assert err <= gbar * np.linalg.norm(b) + 2e-6 * np.linalg.norm(rg), (nm, err, float(np.linalg.norm(b)))
