"""k_snet6 (csrc/k_snet6.hip) where its first layer sits next to the adjoint layer loop, at shapes tests/snet6_domain.py does not have.

The kernel evaluates the first layer's plane rows three times per tile: forward, again at adjoint layer j == 0 (h_0 is recomputed, not
stored) and in the first-layer adjoint's dL/dz row; the operands of the splits, the cosine tags and the per-point sums are built in the
order the instructions want them.  With ONE hidden matrix the adjoint loop runs j == 0 only, directly in front of the first-layer
adjoint; one, two and three coordinates take different trips through the first layer's row loop; 49 units leave 15 padded features in
the last block.  Four hidden matrices with si 2, so 3 and sample weights is the long form of the same code.  Batches of 1, 17 and
129 points: seven inactive waves, a partial second tile, a second workgroup with one active wave.

Every case: loss and gradient per Keras tensor and per slot group against the fp64 oracle, with the k_snet4 + k_gw_* route as the
yardstick of the group bars and the witness that k_snet6 ran -- the checks and bars of tests/snet6_domain.py as
tests/test_gpu_snet6_domain.py uses them: loss 2e-6 and flat gradient 3e-5 at 129 points (its test 1 has 127- and 129-point cases),
loss 1e-5 and no flat bar at 1 and 17 points (its ragged-batch test: the loss of a handful of points, (u - y)^2, has no more)."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import snet6_domain as D
from tests.test_gpu_parity import _cfg, _make, _snet6_shape

pytestmark = pytest.mark.gpu

BMAX = 129
# name: (units, hidden matrices, si, so)
NETS = {"fl_%dx1_si%d" % (n, si): (n, 1, si, si) for n in (49, 64) for si in (1, 2, 3)}
NETS["fl_64x4_si2_so3"] = (64, 4, 2, 3)


@pytest.fixture(scope="module")
def nets():
    """one engine and one 129-point batch per net; the smaller batches are its first rows"""
    made = {}

    def get(name):
        if name not in made:
            n, L, si, so = NETS[name]
            out = _make((_cfg("NIFMultiScale", n, L, 32, 2, 1, si, so, 1), BMAX))
            spec = out[2]
            assert _snet6_shape(spec) and spec.n_hidden_mats == L and not spec.s_res and (spec.si, spec.so) == (si, so), name
            made[name] = out
        return made[name]

    yield get
    for out in made.values():
        out[0]._engine.close()


@pytest.mark.parametrize("B", [1, 17, BMAX])
@pytest.mark.parametrize("name", sorted(NETS))
def test_first_layer_shapes_against_the_oracle(nets, name, B):
    m, model, spec, ws, x, y, sw = nets(name)
    x, y, sw = x[:B], y[:B], sw[:B]
    what = "%s B %d" % (name, B)
    (l1, g1), (l0, g0) = D.both_routes(m._engine, x, y, sw)
    lref, gref = O.loss_and_grad(spec, ws, x.astype(np.float64), y.astype(np.float64), sw.astype(np.float64))
    loss_bar, flat_bar = (2e-6, 3e-5) if B == BMAX else (1e-5, None)
    D.check_tensor_bars(spec, l1, g1, lref, gref, what + " fused", loss_bar, flat_bar)
    D.check_tensor_bars(spec, l0, g0, lref, gref, what + " unfused", loss_bar, flat_bar)
    D.check_group_bars(spec, g1, g0, gref, what)
    if B > 1:      # (one point: a sum of one term per entry may well come out the same on both routes)
        D.check_route_witness(spec, g1, g0, 5e-5, what)
