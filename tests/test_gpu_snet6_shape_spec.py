"""k_snet6<4, PR, 1, 1> (csrc/k_snet6.hip): the form of the fused-gradient training kernel that knows one coordinate and one output at
compile time, against the run-time-shape form k_snet6<4, PR, 0, 0> of the same launch (nif_set_option "s6_shape_generic" = 1) and
against the fp64 oracle.

The two forms run the same sums in the same order, so loss and gradient agree under numpy.array_equal -- not to a tolerance.  Nets:
49 (padded) and 64 units, one and four hidden matrices (both ends of nh), ParameterNet 2 x 32, latent_dim 1.  Batches of 1, 17, 129
and 2049 points: a lone point, a ragged tile, a ragged round (a second workgroup with one active wave), more than one round's worth
of tiles; with and without sample weights.  Float32 also meets the oracle at the bars tests/test_gpu_snet6_first_layer.py uses for
these nets (tests/snet6_domain.py: loss 2e-6 and flat gradient 3e-5 from 129 points on, loss 1e-5 and no flat bar at 1 and 17 points,
every tensor 5e-5 of its norm + 2.5e-7 of the gradient's).  The two policy forms are compared with their generic forms; their
accuracy is what tests/test_gpu_snet6_domain.py pins (its si = so = 1 nets run the <1, 1> forms).  A net with two coordinates and a
net with three outputs run the generic form whatever the option says: the option changes nothing there."""
import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import snet6_domain as D
from tests.test_gpu_parity import _cfg, _make, _make_policy, _snet6_shape

pytestmark = pytest.mark.gpu

BMAX = 2049
BATCHES = [1, 17, 129, BMAX]
POLICIES = ["float32", "mixed_bfloat16", "mixed_float16"]
# name: (units, hidden matrices, si, so)
NETS = {"ss_%dx%d" % (n, L): (n, L, 1, 1) for n in (49, 64) for L in (1, 4)}
OTHER = {"ss_64x1_si2_so1": (64, 1, 2, 1), "ss_49x4_si1_so3": (49, 4, 1, 3)}


@pytest.fixture(scope="module")
def nets():
    """one engine and one 2049-point batch per (net, policy); the smaller batches are its first rows"""
    made = {}

    def get(name, policy="float32"):
        if (name, policy) not in made:
            n, L, si, so = {**NETS, **OTHER}[name]
            key = (_cfg("NIFMultiScale", n, L, 32, 2, 1, si, so, 1), BMAX)
            out = _make(key) if policy == "float32" else _make_policy(key, policy)
            spec = out[2]
            assert _snet6_shape(spec) and spec.n_hidden_mats == L and not spec.s_res and (spec.si, spec.so) == (si, so), name
            made[(name, policy)] = out
        return made[(name, policy)]

    yield get
    for out in made.values():
        out[0]._engine.close()


def _both_forms(engine, x, y, sw):
    """the same batch through the default form and through the run-time-shape form on one engine: ((loss, g), (loss, g))"""
    engine.set_option("s6_shape_generic", 0)
    default = engine.loss_and_grad(x, y, sw)
    engine.set_option("s6_shape_generic", 1)
    try:
        generic = engine.loss_and_grad(x, y, sw)
    finally:
        engine.set_option("s6_shape_generic", 0)
    return default, generic


def _assert_same_bits(default, generic, what):
    (l1, g1), (l0, g0) = default, generic
    ndiff = int((np.asarray(g1) != np.asarray(g0)).sum())
    print("%s: loss %.9e / %.9e, %d of %d gradient entries differ between the forms" % (what, l1, l0, ndiff, np.asarray(g1).size))
    assert np.all(np.isfinite(g1)) and np.isfinite(l1), what
    assert np.array_equal(np.asarray([l1]), np.asarray([l0])), (what, l1, l0)
    assert np.array_equal(g1, g0), (what, ndiff)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", sorted(NETS))
def test_float32_forms_agree_in_bits_and_meet_the_oracle(nets, name, B, weighted):
    m, model, spec, ws, x, y, sw = nets(name)
    x, y, sw = x[:B], y[:B], (sw[:B] if weighted else None)
    what = "%s B %d%s" % (name, B, " weighted" if weighted else "")
    default, generic = _both_forms(m._engine, x, y, sw)
    _assert_same_bits(default, generic, what)
    lref, gref = O.loss_and_grad(spec, ws, x.astype(np.float64), y.astype(np.float64), None if sw is None else sw.astype(np.float64))
    loss_bar, flat_bar = (2e-6, 3e-5) if B >= 129 else (1e-5, None)
    D.check_tensor_bars(spec, default[0], default[1], lref, gref, what, loss_bar, flat_bar)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("policy", POLICIES[1:])
@pytest.mark.parametrize("name", sorted(NETS))
def test_policy_forms_agree_in_bits(nets, name, policy, B, weighted):
    m, model, spec, ws, x, y, sw = nets(name, policy)
    assert m.mixed_policy_name == policy
    default, generic = _both_forms(m._engine, x[:B], y[:B], sw[:B] if weighted else None)
    _assert_same_bits(default, generic, "%s %s B %d%s" % (name, policy, B, " weighted" if weighted else ""))


@pytest.mark.parametrize("name", sorted(OTHER))
def test_the_option_changes_nothing_on_other_shapes(nets, name):
    """si = 2 (so = 1) and so = 3 (si = 1): one of the two counts is 1, the launch must still take the run-time-shape form"""
    m, model, spec, ws, x, y, sw = nets(name)
    B = 129
    x, y, sw = x[:B], y[:B], sw[:B]
    default, generic = _both_forms(m._engine, x, y, sw)
    _assert_same_bits(default, generic, name)
    lref, gref = O.loss_and_grad(spec, ws, x.astype(np.float64), y.astype(np.float64), sw.astype(np.float64))
    D.check_tensor_bars(spec, default[0], default[1], lref, gref, name, 2e-6, 3e-5)
