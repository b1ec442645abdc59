"""A workspace allocation that fails leaves the context consistent: no field claims memory that is not there, so the steps after the
failure allocate again and compute what a context that never saw a failure computes (device memory)."""
import numpy as np
import pytest

from tests.test_gpu_parity import CONFIGS, _cfg, _make

pytestmark = pytest.mark.gpu

B_TILE = 2080        # one 32-point tile above NIF_SMALL_MAX_B = 2048: the tile kernels and their point workspaces
B_GROW = 4128        # a second growth of every workspace
B_SMALL = 512        # the one-launch small-batch step (partial rows and loss partials only)

NETS = [
    _cfg("NIFMultiScale", 32, 2, 32, 2, 1, 1, 1, 1),       # ParameterNet without a stash
    CONFIGS["ms_res_48x2_pres"][0],                        # ParameterNet through the HBM stash
]


def _step(m, x, y, B):
    loss, g = m._engine.loss_and_grad(x[:B], y[:B])
    return np.float32(loss), g


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_failed_reserve_leaves_the_context_consistent():
    import nif_amd
    for cfg in NETS:
        a, _, _, _, x, y, _ = _make((cfg, B_GROW), seed=5)
        first = _step(a, x, y, B_TILE)
        assert np.isfinite(first[0]) and np.isfinite(first[1]).all()
        # 2^38 points: the first workspace request alone is >= 1 TiB, beyond any HBM -- the allocation fails before anything sizeable is held
        with pytest.raises(nif_amd.NifError, match=r"libnif_hip error -2\b"):      # NIF_ERR_HIP
            a._engine.reserve(2 ** 38)
        assert _same(_step(a, x, y, B_TILE), first)
        b = _make((cfg, B_GROW), seed=5)[0]      # the same net and data on a context that never saw a failure
        for B in (B_GROW, B_SMALL):
            assert _same(_step(a, x, y, B), _step(b, x, y, B)), B
