"""Call orders of the C-ABI (tests/api_order.py): every ordered pair of ops behind every pending prefix, seeded random walks, and the
named regressions of the holes the sweep was written for.  The lazy run of a sequence and the eager run (everything deferred forced
behind every op) must agree bit for bit; theta-changing ops are anchored against the oracle."""
import itertools

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import api_order as AO
from tests.test_gpu_parity import CONFIGS, _make, _make_policy
from tests.test_gpu_tail import CASES

pytestmark = pytest.mark.gpu

NETS = {k: v[0] for k, v in CASES.items()}
NETS["ll_plain_32x2_r3"] = CONFIGS["ll_plain_32x2_r3"][0]
NETS["ms_res_48x2_pres"] = CONFIGS["ms_res_48x2_pres"][0]
POLICY_NET = "ms_cfg2_64x4:mixed_bfloat16"          # the `small` prefix set only
PARAMS = sorted(NETS) + [POLICY_NET]
WALK_SEEDS = (11, 23)
COMM_NET = "small_nif_32x2"                         # the net whose sweep also holds the comm_attach sequences (api_order.SWEEP_EXCLUDED)

# (prefix, X, Y) triples that need a redesign rather than a flush, with the cause (none)
XFAIL = {}


def _context(name):
    if ":" in name:
        base, policy = name.split(":")
        made = _make_policy((CONFIGS[base][0], AO.B_SMALL), policy)
    else:
        made = _make((NETS[name], AO.B_SMALL))
    m, spec = made[0], made[2]
    c = AO.Ctx(m._engine, AO.Fixture(m._engine, spec))
    c.keep = made[:2]
    AO.probe_caps(c)
    return c


def _pair(name):
    cl, ce = _context(name), _context(name)
    assert cl.fix.caps == ce.fix.caps
    return cl, ce, AO.alphabet(cl.fix.caps)


@pytest.mark.parametrize("name", PARAMS)
def test_every_pair_behind_every_pending_prefix(name):
    cl, ce, ops = _pair(name)
    prefixes = AO.PREFIXES if ":" not in name else {k: AO.PREFIXES[k] for k in AO.SMALL_PREFIXES}
    failures, unexpected_pass, n = [], [], 0
    sequences = AO.pair_sequences(list(ops), prefixes)
    if name == COMM_NET:
        sequences = itertools.chain(sequences, AO.comm_attach_sequences(prefixes))
    for pname, x, y, seq in sequences:
        n += 1
        try:
            what = AO.compare(cl, ce, ops, seq)
        except AO.GpuError as ex:
            pytest.fail("GPU error in (%s, %s, %s), not run again: %s" % (pname, x, y, ex))
        if (pname, x, y) in XFAIL:
            if what is None:
                unexpected_pass.append((pname, x, y))
        elif what is not None:
            failures.append("(%s, %s, %s): %s" % (pname, x, y, what))
    print("%s: %d ops, %d sequences, %d fail" % (name, len(ops), n, len(failures)), flush=True)
    for f in failures[:200]:
        print("FAIL " + f, flush=True)
    if ":" not in name:
        for pname, t, seq in AO.anchor_sequences(list(ops)):
            AO.reset(cl)
            try:
                AO.run_ops(cl, ops, seq, False)
                what = AO.anchor(cl, O)
            except AO.GpuError as ex:
                pytest.fail("GPU error behind (%s, %s), not run again: %s" % (pname, t, ex))
            if what is not None:
                failures.append("oracle anchor behind (%s, %s): %s" % (pname, t, what))
    assert not failures, "%d of %d sequences fail:\n%s" % (len(failures), n, "\n".join(failures[:60]))
    assert not unexpected_pass, "expected to fail (XFAIL), pass: %r" % unexpected_pass


@pytest.mark.parametrize("name", sorted(NETS))
def test_seeded_random_walks(name):
    cl, ce, ops = _pair(name)
    names = list(ops)
    for seed in WALK_SEEDS:
        seq = AO.walk(names, seed)
        try:
            what = AO.compare(cl, ce, ops, seq, midpoints=AO.walk_midpoints(seed))
            if what is None:      # a third run, with the oracle anchor behind every theta-changing op
                found = []

                def hook(c, i, op):
                    if op in AO.THETA_OPS:
                        w = AO.anchor(c, O)
                        if w is not None:
                            found.append("oracle anchor behind op %d (%s): %s" % (i, op, w))
                AO.reset(cl)
                AO.run_ops(cl, ops, seq, False, after=hook)
                what = "; ".join(found) or None
        except AO.GpuError as ex:
            pytest.fail("GPU error in walk %d %r, not run again: %s" % (seed, seq, ex))
        if what is not None:
            def outcome(cand):      # each candidate on fresh contexts
                a, b, o = _pair(name)
                return AO.compare(a, b, o, cand)
            core, why = AO.shrink(seq, outcome)
            pytest.fail("walk %d fails: %s\nshortest failing subsequence %r: %s" % (seed, what, core, why or "passes alone (the anchor run)"))


def _metric_after(c, ops, seq):
    AO.reset(c)
    errs, _ = AO.run_ops(c, ops, seq, False)
    assert not errs, errs
    return c.e.metric_read(reset=False)


@pytest.mark.parametrize("name", sorted(NETS))
def test_named_regressions(name):
    """the mechanisms: a deferred metric accumulation belongs to the step it was called for, whatever rewrites grad[P] next"""
    cl, ce, ops = _pair(name)
    w = float(np.float32(AO.METRIC_W))

    def loss_of(step):
        AO.reset(ce)
        ops[step](ce)
        return float(np.float32(ce.e.last_loss()))
    la, lt = loss_of("loss_grad_a"), loss_of("loss_grad_tile")
    s_rep, n_rep = _metric_after(ce, ops, ["capture", "replay"])          # what the replay itself accumulates: l1 + l2, weight 1 each
    assert n_rep == 2.0
    l1 = la                                                               # the graph's first step: batch a at theta0, the same kernel
    l2 = s_rep - l1                                                       # (two float32 values summed in double: exact)
    # small step -> metric_accumulate (deferred) -> replay -> metric_read
    s, n = _metric_after(cl, ops, ["capture", "loss_grad_a", "metric_accumulate", "replay"])
    assert (s, n) == ((w * la + l1) + l2, w + 2.0), (s, n, la, l1, l2)
    # capture (its recorded steps are small steps; none ran) -> metric_accumulate -> replay -> metric_read
    s, n = _metric_after(cl, ops, ["loss_grad_tile", "capture", "metric_accumulate", "replay"])
    assert (s, n) == ((w * lt + l1) + l2, w + 2.0), (s, n, lt, l1, l2)
    # small step -> metric_accumulate -> comm_attach -> metric_read; and with the self-test's fill of [grad | loss] behind it
    s, n = _metric_after(cl, ops, ["loss_grad_a", "metric_accumulate", "comm_attach"])
    assert (s, n) == (w * la, w), (s, n, la)
    s, n = _metric_after(cl, ops, ["loss_grad_a", "metric_accumulate", "comm_attach", "comm_selftest"])
    assert (s, n) == (w * la, w), (s, n, la)
    s, n = _metric_after(cl, ops, ["loss_grad_a", "metric_accumulate", "comm_selftest"])
    assert (s, n) == (w * la, w), (s, n, la)
    # found by the sweep: the regulariser term lands in grad[P]; a deferred accumulation takes the loss as it stood at its call
    s, n = _metric_after(cl, ops, ["loss_grad_a", "metric_accumulate", "set_regularizer_on", "grad_read"])
    assert (s, n) == (w * la, w), (s, n, la)
    s, n = _metric_after(cl, ops, ["loss_grad_a", "metric_accumulate", "set_regularizer_on", "adam_step"])
    assert (s, n) == (w * la, w), (s, n, la)
    # found by the sweep: a gradient read with no regulariser set must not keep one that is set afterwards out of the update
    AO.reset(cl); AO.run_ops(cl, ops, ["loss_grad_a", "grad_read", "set_regularizer_on", "adam_step"], False)
    AO.reset(ce); AO.run_ops(ce, ops, ["loss_grad_a", "set_regularizer_on", "adam_step"], False)
    assert np.array_equal(cl.e.get_flat(), ce.e.get_flat())
    assert not np.array_equal(cl.e.get_flat(), cl.fix.theta0)
    # found by the sweep: the profiler's events must stay out of a capture (read back, they are graph nodes without a time)
    AO.reset(cl)
    errs, _ = AO.run_ops(cl, ops, ["profile_on", "capture", "profile_off", "profile_on", "replay", "profile_off"], False)
    assert not errs, errs
