"""The order sweep's own machinery, without a GPU (tests/api_order.py): every export of include/nif_hip.h is reached by an op of the alphabet
or exempt for a stated reason, the pair sweep is the cartesian product, walks are a function of their seed, and the shrinker finds the
two-op core of a planted order bug."""
import itertools
import os
import re
from collections import OrderedDict

import numpy as np

from tests import api_order as AO
from tests.doubles import DeferredMetricEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NO_STATE = "no context state"
PRIMITIVE = "memory, copy or timer primitive: touches none of the deferred fields"
MULTI = "needs more than one GPU"
HOST = "host-pointer wrapper whose _dev form is in the alphabet"
# (no export is exempt as PRIMITIVE: the allocation, copy and stopwatch calls all run the deferred reduction first, so an op reaches them)
EXEMPT = {
    "nif_last_error": NO_STATE, "nif_abi_version": NO_STATE, "nif_device_count": NO_STATE, "nif_device_pci_bus_id": NO_STATE,
    "nif_opt_scalars": NO_STATE,      # (nif_comm_unique_id has no context state either; comm_attach calls it)
    "nif_comm_init_all": MULTI, "nif_allreduce_grad_multi": MULTI, "nif_train_step_multi": MULTI,
    "nif_forward": HOST,                 # nif_forward_dev
    "nif_loss_and_grad": HOST,           # nif_loss_grad_dev + nif_grad_read
    "nif_train_step": HOST,              # nif_loss_grad_dev + nif_adam_step_dev
    "nif_latent_to_w": HOST,             # nif_latent_to_w_dev
    "nif_shapenet_given_w": HOST,        # nif_shapenet_given_w_dev
    "nif_hessian": HOST,                 # nif_hessian_dev
}


def _exports():
    text = open(os.path.join(ROOT, "include", "nif_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nif_[a-z0-9_]+)\s*\(", text)))


def _engine_methods():
    """{C symbol: [Engine / DeviceArray methods whose body calls it]} from nif_amd/engine.py"""
    src = open(os.path.join(ROOT, "nif_amd", "engine.py")).read()
    out = {}
    for m in re.finditer(r"^    def (\w+)\(.*?(?=^    def |^class |\Z)", src, flags=re.S | re.M):
        for sym in re.findall(r"\blib\.(nif_\w+)", m.group(0)):
            out.setdefault(sym, []).append(m.group(1))
    return out


def test_every_export_is_reached_by_an_op_or_exempt():
    exports = _exports()
    assert len(exports) > 90, exports
    bound = open(os.path.join(ROOT, "nif_amd", "_lib.py")).read()
    ops_src = open(os.path.join(ROOT, "tests", "api_order.py")).read()
    methods = _engine_methods()
    missing = []
    for sym in exports:
        assert '"%s"' % sym in bound, "%s is not bound in nif_amd/_lib.py" % sym
        reached = ("lib.%s(" % sym) in ops_src or any(re.search(r"\be\.%s\(" % m, ops_src) for m in methods.get(sym, []))
        if reached == (sym in EXEMPT):
            missing.append("%s: %s" % (sym, "reached by an op AND exempt" if reached else "neither reached by an op of tests/api_order.py nor in EXEMPT"))
    assert not missing, "\n".join(missing)
    assert set(EXEMPT) <= set(exports), sorted(set(EXEMPT) - set(exports))
    assert set(EXEMPT.values()) <= {NO_STATE, PRIMITIVE, MULTI, HOST}


def test_alphabet_holds_what_the_prefixes_and_the_anchor_name():
    names = list(AO.full_alphabet())
    assert len(names) == len(set(names)) >= 55
    for pre in AO.PREFIXES.values():
        assert set(pre) <= set(names)
    assert set(AO.THETA_OPS) <= set(names) and set(AO.NEEDS) <= set(names)
    assert len(AO.NOT_BITWISE) <= 2
    assert not set(AO.NOT_BITWISE) & {"loss_grad_a", "loss_grad_a_weighted", "loss_grad_b", "loss_grad_tile", "adam_step", "lion_step",
                                      "adabelief_step", "metric_accumulate", "metric_read", "metric_read_reset"}


def test_pair_sweep_is_the_cartesian_product():
    full = list(AO.full_alphabet())
    assert set(AO.SWEEP_EXCLUDED) == {"comm_attach"}      # one op, for its measured cost; it has sequences of its own
    names = [n for n in full if n not in AO.SWEEP_EXCLUDED]
    got = [(p, x, y) for p, x, y, _ in AO.pair_sequences(full)]
    assert len(got) == len(set(got)) == len(AO.PREFIXES) * len(names) ** 2
    assert set(got) == set(itertools.product(AO.PREFIXES, names, names))
    comm = [(p, x, y) for p, x, y, _ in AO.comm_attach_sequences()]
    assert set(comm) == set(itertools.product(AO.PREFIXES, ["comm_attach"], AO.COMM_PARTNERS))
    for p, x, y, seq in itertools.islice(AO.pair_sequences(names), 0, None, 997):
        assert seq == AO.PREFIXES[p] + [x, y]


def test_walks_are_a_function_of_the_seed():
    names = list(AO.full_alphabet())
    a, b = AO.walk(names, 11), AO.walk(names, 11)
    assert a == b and len(a) == 16 and set(a) <= set(names)
    assert AO.walk(names, 12) != a
    k = AO.walk_midpoints(11)
    assert k == AO.walk_midpoints(11) and len(set(k)) == 2 and all(1 <= i < 16 for i in k)


def _fake_ops():
    ops = OrderedDict()
    ops["step_a"] = lambda c: c.e.step(1.0)
    ops["step_b"] = lambda c: c.e.step(2.0)
    ops["metric_accumulate"] = lambda c: c.e.metric_accumulate(0.75)
    ops["replay"] = lambda c: c.e.replay()
    ops["update"] = lambda c: c.e.update()
    ops["metric_read"] = lambda c: c.e.metric_read(reset=False)
    return ops


class _FakeCtx(object):
    def __init__(self, bug):
        self.e, self.reads = DeferredMetricEngine(bug), []


def _fake_outcome(bug):
    ops = _fake_ops()

    def observe(c):
        return OrderedDict([("metric", np.array(c.e.metric_read(reset=False))), ("loss", np.array([c.e.loss])), ("theta", np.array([c.e.theta]))])

    def outcome(seq):      # fresh contexts for every candidate
        cl, ce = _FakeCtx(bug), _FakeCtx(bug)
        return AO.compare(cl, ce, ops, seq, reset_fn=lambda c: None, observe_fn=observe, full_fn=observe, check_metric=False)
    return outcome


def test_shrinker_returns_the_two_op_core_of_a_planted_order_bug():
    seq = ["update", "step_b", "metric_read", "step_a", "update", "metric_accumulate", "update", "metric_read", "step_a", "metric_accumulate",
           "update", "replay", "step_b", "update", "metric_read", "step_a"]
    core, what = AO.shrink(seq, _fake_outcome(True))
    assert core == ["metric_accumulate", "replay"] and "metric" in what
    assert AO.shrink(seq, _fake_outcome(False)) == (seq, None)


def test_shrinker_stops_at_the_first_gpu_error():
    calls = []

    def outcome(seq):
        calls.append(list(seq))
        if len(seq) == 3:
            raise AO.GpuError("x", "libnif_hip error -2: fault")
        return "mismatch"
    core, what = AO.shrink(["a", "b", "c", "d"], outcome)
    assert len(core) == 3 and what.startswith("GPU error") and len(calls) == 2
