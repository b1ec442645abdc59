"""Cases of tests/test_gpu_wide_ll.py: NIFMultiScaleLastLayerParameterized with a ShapeNet of 129..512 units, the domain of the
workgroup-tiled layer kernels (csrc/k_wide.hip; tile 128 rows x 64 columns x 32 reduction steps).  The shapes are the smallest that
reach each guard of the tile program; every one of them was refused by nif_create before these kernels existed."""
import numpy as np

from oracle import nif_oracle as O
from tests.test_gpu_parity import _cfg, _make


def _case(n, L, r, si, so, pi, B, nst=32, lst=2, p_act="sine"):
    return _cfg("LL", n, L, nst, lst, r, si, so, pi, p_act=p_act), B


# name: ((kind, cfg_shape_net, cfg_parameter_net), batch)
CASES = {
    "w129x1": _case(129, 1, 3, 2, 2, 1, 33),                         # one feature past the cap: row and reduction tails of 1
    "w144x2": _case(144, 2, 5, 3, 3, 1, 257, p_act="swish"),         # width no multiple of 32; partial point tile
    "w256x3": _case(256, 3, 10, 3, 3, 1, 1000),                      # exact tiles; several workgroups in the sums over the batch
    "w256x6": _case(256, 6, 10, 3, 3, 1, 160, p_act="swish"),        # configs[3]'s depth at twice its width
    "w320x0": _case(320, 0, 4, 1, 1, 2, 31, nst=20, lst=1),          # no hidden matrix: first layer -> bottleneck; less than one tile
    "w512x1": _case(512, 1, 16, 2, 4, 1, 65),                        # the admission edge; r so = 64
    "w192x2_b1": _case(192, 2, 1, 1, 1, 1, 1, p_act="tanh"),         # a single point, r so = 1
    # 1251 point tiles = 626 point blocks x 2 row blocks of a 144-wide layer: more work items than the 1024 workgroups of a launch
    "w144x2_b40k": _case(144, 2, 5, 3, 3, 1, 40001, p_act="swish"),
}
SMALL = [k for k in sorted(CASES) if k != "w144x2_b40k"]

_cache = {}


def make(name):
    """(m, model, spec, ws64, x, y, sw) of a case, built once: nothing in the tests writes into the arrays; a test that changes the
    model's weights or optimizer state builds its own with fresh()"""
    if name not in _cache:
        _cache[name] = _make(CASES[name])
    return _cache[name]


def fresh(name):
    return _make(CASES[name])


_refs = {}


def ref_loss_grad(name, weighted):
    """the oracle's (loss, [gradient tensors]) of a case in float64, computed once"""
    key = (name, weighted)
    if key not in _refs:
        m, model, spec, ws, x, y, sw = make(name)
        s = sw.astype(np.float64) if weighted else None
        _refs[key] = O.loss_and_grad(spec, ws, x.astype(np.float64), y.astype(np.float64), s)
    return _refs[key]
