"""CPU tests of the Lion / AdaBelief surface (reference nif/optimizers/external_optimizers.py:322-735): the constructors, the host
function that forms the per-step scalars (nif_opt_scalars, the code every eager step runs and every captured block compiles), the
nif_opt ctypes layout against include/nif_hip.h, and Model.fit / save_weights / load_weights dispatching to the new engine calls --
on one process and on two gloo processes with uneven shards, with an engine double whose update is the NumPy restatement."""
import os
import re
import types
import warnings

import numpy as np
import pytest

from oracle import nif_oracle as O
from tests import opt_ref as R
from tests.cfgs import ALL_SMALL
from tests.doubles import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- constructors -------------------------------------------------------------------------------------------------------------
def test_constructor_defaults_and_config_keys():
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    lion = Lion()
    assert (lion.learning_rate, lion.beta_1, lion.beta_2, lion.wd, lion.decay, lion.name) == (1e-4, 0.9, 0.99, 0.0, 0.0, "lion")
    assert sorted(lion.get_config()) == sorted(["name", "learning_rate", "decay", "beta_1", "beta_2", "wd"])
    ab = AdaBeliefOptimizer()
    assert (ab.learning_rate, ab.beta_1, ab.beta_2, ab.epsilon, ab.weight_decay) == (1e-3, 0.9, 0.999, 1e-14, 0.0)
    assert (ab.rectify, ab.amsgrad, ab.sma_threshold, ab.total_steps, ab.warmup_proportion, ab.min_lr) == (True, False, 5.0, 0, 0.1, 0.0)
    assert ab.name == "AdaBeliefOptimizer"
    assert sorted(ab.get_config()) == sorted(["name", "learning_rate", "beta_1", "beta_2", "decay", "weight_decay", "sma_threshold",
                                              "epsilon", "amsgrad", "rectify", "total_steps", "warmup_proportion", "min_lr"])
    assert AdaBeliefOptimizer(epsilon=0).epsilon == 1e-7          # `epsilon or K.epsilon()`
    assert AdaBeliefOptimizer.from_config(ab.get_config()).get_config() == ab.get_config()
    assert Lion.from_config(lion.get_config()).get_config() == lion.get_config()


def test_lr_and_decay_aliases_and_learning_rate_property():
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    for cls in (Lion, AdaBeliefOptimizer):
        o = cls(learning_rate=0.5, lr=0.25, decay=1e-3, name="x", print_change_log=False)
        assert o.learning_rate == 0.25 and o.lr == 0.25 and o.decay == 1e-3 and o.name == "x"
        o.lr = 0.125
        assert o.learning_rate == 0.125 and o.as_opt().lr == 0.125
        o.learning_rate = 2.0
        assert o.lr == 2.0
        with pytest.raises(ValueError):
            cls(decay=-1.0)


@pytest.mark.parametrize("kw", ["clipnorm", "clipvalue", "global_clipnorm", "momentum"])
def test_rejected_keyword_arguments_are_named(kw):
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    for cls in (Lion, AdaBeliefOptimizer):
        with pytest.raises(NotImplementedError, match=kw):
            cls(**{kw: 1.0})


def test_schedule_objects_are_rejected():
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    sched = lambda step: 1e-3      # noqa: E731  (anything that is not a number)
    with pytest.raises(NotImplementedError, match="learning_rate"):
        Lion(learning_rate=sched)
    with pytest.raises(NotImplementedError, match="learning_rate"):
        AdaBeliefOptimizer(learning_rate=sched)
    with pytest.raises(NotImplementedError, match="weight_decay"):
        AdaBeliefOptimizer(weight_decay=sched)


def test_l4adam_is_refused_and_get_keeps_the_new_instances():
    from nif_amd import optimizers
    with pytest.raises(NotImplementedError, match="L4Adam"):
        optimizers.L4Adam()
    lion, ab = optimizers.Lion(), optimizers.AdaBeliefOptimizer()
    assert optimizers.get(lion) is lion and optimizers.get(ab) is ab       # (AdaBelief has learning_rate / beta_1 / beta_2 / epsilon:
    adam = optimizers.get(types.SimpleNamespace(learning_rate=1e-2, beta_1=0.8, beta_2=0.9, epsilon=1e-6))   # not duck-typed to Adam)
    assert isinstance(adam, optimizers.Adam) and adam.learning_rate == 1e-2
    with pytest.raises(NotImplementedError):
        optimizers.get("lion")


# ---- the host scalar function -----------------------------------------------------------------------------------------------------
def _lib_scalars(opt, ts):
    import ctypes
    from nif_amd import _lib
    lib = _lib.load()
    o = opt.as_opt()
    out = (ctypes.c_double * 5)()
    rows = []
    for t in ts:
        _lib.check(lib.nif_opt_scalars(ctypes.byref(o), int(t), out))
        rows.append(list(out))
    return np.array(rows)


def _configs():
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    return {
        "adabelief_default": AdaBeliefOptimizer(),
        "adabelief_warmup_decay": AdaBeliefOptimizer(learning_rate=1e-3, total_steps=10000, warmup_proportion=0.1, min_lr=1e-5),
        "adabelief_decay_norect": AdaBeliefOptimizer(learning_rate=2e-3, decay=1e-3, rectify=False, beta_2=0.99),
        "adabelief_short_horizon": AdaBeliefOptimizer(total_steps=10, warmup_proportion=0.3, min_lr=1e-5, decay=1e-4),
        "lion_decay": Lion(learning_rate=3e-4, decay=1e-3),
    }


@pytest.mark.parametrize("name", sorted(_configs()))
def test_host_scalars_over_20000_steps_match_the_restatement(name):
    """nif_opt_scalars against opt_ref.scalars for t = 1 ... 20 000, all five configurations: measured max rel. difference 0 for the
    learning rate, both bias corrections and r_t (the same fp64 expressions); bar 1e-12, the branch exact"""
    opt = _configs()[name]
    ts = np.arange(1, 20001)
    got = _lib_scalars(opt, ts)
    want = np.array([R.scalars(opt, t) for t in ts], dtype=np.float64)
    rel = lambda a, b: np.abs(a - b) / np.maximum(np.abs(b), 1e-300)     # noqa: E731
    assert rel(got[:, 0], want[:, 0]).max() < 1e-12
    if opt.kind == 2:
        assert rel(got[:, 1], want[:, 1]).max() < 1e-12 and rel(got[:, 2], want[:, 2]).max() < 1e-12
        assert np.array_equal(got[:, 4] != 0, want[:, 4].astype(bool))
        div = want[:, 4].astype(bool)
        assert rel(got[div, 3], want[div, 3]).max() < 1e-12


def test_branch_switch_warmup_ramp_and_decay_floor():
    from nif_amd.optimizers import AdaBeliefOptimizer
    got = _lib_scalars(AdaBeliefOptimizer(), range(1, 9))
    # b2 = 0.999: sma_t = 1.0, 2.0, 3.0, 4.0, 4.996 (momentum steps), 5.994 at t = 6 (rectified from there on)
    assert list(got[:, 4]) == [0, 0, 0, 0, 0, 1, 1, 1]
    assert np.allclose([R.sma(0.999, t) for t in range(1, 7)], [1.0, 2.0, 3.0, 4.0, 4.996, 5.994], atol=3e-3)
    ab = AdaBeliefOptimizer(learning_rate=1e-3, total_steps=1000, warmup_proportion=0.1, min_lr=1e-5)
    lr = _lib_scalars(ab, range(1, 1501))[:, 0]
    assert np.allclose(lr[:100], 1e-3 * np.arange(1, 101) / 100.0, rtol=1e-6)          # linear warm-up to lr at t = w = 100
    assert np.all(np.diff(lr[100:1000]) < 0)                                          # then a linear decay ...
    assert abs(lr[999] - 1e-5) < 1e-10 and np.allclose(lr[1000:], lr[999], rtol=0, atol=1e-12)   # ... to min_lr at total_steps, held
    lion = _lib_scalars(types.SimpleNamespace(as_opt=_lion_opt(1e-3, 0.5)), [1, 2, 11])[:, 0]
    assert np.allclose(lion, [1e-3, 1e-3 / 1.5, 1e-3 / 6.0], rtol=1e-7)


def _lion_opt(lr, decay):
    def make():
        from nif_amd.optimizers import Lion
        return Lion(learning_rate=lr, decay=decay).as_opt()
    return make


# ---- the struct against the header ----------------------------------------------------------------------------------------------
def test_nif_opt_layout_matches_the_header():
    import ctypes
    from nif_amd import _lib
    txt = open(os.path.join(ROOT, "include", "nif_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*nif_opt;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        for nm in names.split(","):
            nm = nm.strip()
            mm = re.match(r"(\w+)\[(\d+)\]", nm)
            fields.append((mm.group(1), typ, int(mm.group(2))) if mm else (nm, typ, 1))
    ct = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    got = [(nm, t) for nm, t in _lib.nif_opt._fields_]
    assert [nm for nm, _ in got] == [f[0] for f in fields]
    for (nm, t), (_, typ, n) in zip(got, fields):
        assert t == (ct[typ] if n == 1 else ct[typ] * n), nm
    assert ctypes.sizeof(_lib.nif_opt) == 72
    assert _lib.nif_opt.total_steps.offset == 48
    m = re.search(r"NIF_OPT_ADAM = (\d+), NIF_OPT_LION = (\d+), NIF_OPT_ADABELIEF = (\d+)", txt)
    assert tuple(int(v) for v in m.groups()) == (_lib.OPT_ADAM, _lib.OPT_LION, _lib.OPT_ADABELIEF)
    assert int(re.search(r"#define NIF_OPT_RECTIFY (\d+)", txt).group(1)) == _lib.OPT_RECTIFY
    assert int(re.search(r"#define NIF_OPT_AMSGRAD (\d+)", txt).group(1)) == _lib.OPT_AMSGRAD


# ---- Model.fit on an engine double ----------------------------------------------------------------------------------------------
def _hyper(o):
    """the nif_opt a step receives, as the attribute set opt_ref reads"""
    return types.SimpleNamespace(kind=o.kind, learning_rate=o.lr, beta_1=o.beta1, beta_2=o.beta2, epsilon=o.eps, wd=o.weight_decay,
                                 weight_decay=o.weight_decay, decay=o.decay, rectify=bool(o.flags & 1), amsgrad=bool(o.flags & 2),
                                 sma_threshold=o.sma_threshold, total_steps=int(o.total_steps), warmup_proportion=o.warmup_proportion,
                                 min_lr=o.min_lr)


def opt_apply(theta, g, m, v, vhat, hyper, t):
    th = np.asarray(theta, np.float32)
    if hyper.kind == 1:
        th, m = R.lion(th, g, m, hyper, t)
    else:
        th, m, v, vhat = R.adabelief(th, g, m, v, vhat if vhat is not None else np.zeros_like(th), hyper, t)
    return th.astype(np.float64), m, v, vhat


class OptEngine(OracleEngine):
    """OracleEngine + the Lion / AdaBelief calls: the update is the NumPy restatement (float32), the regulariser term added first"""

    def __init__(self, spec_oracle, weights, reg=(0.0, 0.0, 0, 0)):
        OracleEngine.__init__(self, spec_oracle, weights, reg)
        self.vhat = np.zeros_like(self.theta)
        self.shapes = spec_oracle.param_shapes()

    def opt_step_dev(self, opt):
        l1, l2, lo, hi = self.reg
        if (l1 or l2) and not self.reg_applied:
            w = self.theta[lo:hi]
            self.grad_buf[lo:hi] += 2.0 * l2 * w + l1 * np.sign(w)
            self.grad_buf[-1] += l2 * np.sum(w * w) + l1 * np.sum(np.abs(w))
        self.t += 1
        self.theta, self.m, self.v, vh = opt_apply(self.theta, self.grad_buf[:-1].astype(np.float32), self.m.astype(np.float32),
                                                   self.v.astype(np.float32), self.vhat.astype(np.float32), _hyper(opt), self.t)
        if vh is not None:
            self.vhat = vh
        self.reg_applied = False
        self.calls.append(("opt_step", int(opt.kind)))

    def adam_step_dev(self, adam):
        self.calls.append(("adam_step",))
        OracleEngine.adam_step_dev(self, adam)

    def get_opt_slot(self, slot):
        return np.asarray((self.m, self.v, self.vhat)[slot], np.float32).copy()

    def set_opt_slot(self, slot, values):
        a = np.asarray(values, np.float64).copy()
        if slot == 0:
            self.m = a
        elif slot == 1:
            self.v = a
        else:
            self.vhat = a

    def get_weights(self):
        return [w.astype(np.float32) for w in O.unflatten(self.o, self.theta)]

    def set_weights(self, weights):
        self.theta = O.flatten([np.asarray(w, np.float64) for w in weights])


def _problem(name="ms_plain", n=72):
    kind, cs, cp = ALL_SMALL[name]
    spec = O.Spec(kind, cs, cp)
    rng = np.random.default_rng(0)
    ws = O.init_weights(spec, rng)
    x = rng.uniform(-1, 1, size=(n, spec.pi + spec.si)).astype(np.float32)
    y = rng.uniform(-1, 1, size=(n, spec.so)).astype(np.float32)
    return kind, cs, cp, spec, ws, x, y


def _model(eng, kind, cs, cp):
    from nif_amd.model import Model
    from nif_amd.spec import Spec
    return Model(types.SimpleNamespace(_spec=Spec(kind, cs, cp), _engine=eng), "full")


def _make_opt(which):
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    return {"lion": lambda: Lion(learning_rate=1e-3, wd=1e-2, decay=1e-3),
            "adabelief": lambda: AdaBeliefOptimizer(learning_rate=1e-2, weight_decay=1e-3),
            "adabelief_ams": lambda: AdaBeliefOptimizer(learning_rate=1e-2, amsgrad=True, total_steps=9, warmup_proportion=0.3)}[which]()


def _serial(spec, ws, x, y, opt, bs, epochs):
    """the manual sequence: one restated update per batch of the global batch order"""
    hyper = _hyper(opt.as_opt())
    th = O.flatten(ws); m = np.zeros_like(th, dtype=np.float32); v = m.copy(); vh = m.copy(); t = 0
    losses = []
    for _ in range(epochs):
        tot = 0.0
        for b0 in range(0, x.shape[0], bs):
            xb, yb = x[b0:b0 + bs].astype(np.float64), y[b0:b0 + bs].astype(np.float64)
            loss, g = O.loss_and_grad(spec, O.unflatten(spec, th), xb, yb)
            t += 1
            th, m, v, vh2 = opt_apply(th, O.flatten(g).astype(np.float32), m, v, vh, hyper, t)
            vh = vh2 if vh2 is not None else vh
            tot += loss * xb.shape[0]
        losses.append(tot / x.shape[0])
    return th, losses


@pytest.mark.parametrize("which", ["lion", "adabelief", "adabelief_ams"])
def test_fit_dispatches_to_opt_step_dev(which):
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = OptEngine(spec, ws)
    model = _model(eng, kind, cs, cp)
    model.compile(_make_opt(which), "mse")
    h = model.fit(x, y, batch_size=16, epochs=3, shuffle=False, verbose=0)
    steps = [c for c in eng.calls if c[0] in ("opt_step", "adam_step")]
    assert len(steps) == 3 * 5 and all(c[0] == "opt_step" for c in steps)
    assert eng.t == 15
    th, losses = _serial(spec, ws, x, y, _make_opt(which), 16, 3)
    assert np.array_equal(eng.theta, th)
    assert np.allclose(h.history["loss"], losses, rtol=1e-12)
    assert not np.array_equal(th, O.flatten(ws))


def test_compile_restarts_the_new_optimizer_and_adam_still_uses_adam_step():
    from nif_amd.optimizers import Adam, AdaBeliefOptimizer
    kind, cs, cp, spec, ws, x, y = _problem()
    eng = OptEngine(spec, ws)
    model = _model(eng, kind, cs, cp)
    model.compile(Adam(1e-3), "mse")
    model.fit(x, y, batch_size=32, epochs=1, shuffle=False, verbose=0)
    assert [c[0] for c in eng.calls if c[0].endswith("_step")] == ["adam_step"] * 3
    eng.calls.clear()
    eng.vhat[:] = 7.0
    model.compile(AdaBeliefOptimizer(amsgrad=True), "mse")
    model.fit(x, y, batch_size=32, epochs=1, shuffle=False, verbose=0)
    assert [c[0] for c in eng.calls if c[0].endswith("_step")] == ["opt_step"] * 3
    assert eng.t == 3                                    # a new optimizer: step 0, zeroed slots (vhat included) before its first step
    assert np.all(eng.vhat < 7.0)


def test_save_load_round_trip_of_the_slots(tmp_path):
    from nif_amd.optimizers import Adam, AdaBeliefOptimizer, Lion
    kind, cs, cp, spec, ws, x, y = _problem()
    for which, nslot in (("lion", 1), ("adabelief", 2), ("adabelief_ams", 3)):
        eng = OptEngine(spec, ws)
        model = _model(eng, kind, cs, cp)
        model.compile(_make_opt(which), "mse")
        model.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
        f = str(tmp_path / which)
        model.save_weights(f)
        d = np.load(f + ".npz")
        assert int(d["opt_step"]) == 5 and "adam_m" not in d
        assert [k in d for k in ("opt_m", "opt_v", "opt_vhat")] == [True, nslot >= 2, nslot >= 3]
        # a fresh model with the same optimizer continues exactly where the first one is
        eng2 = OptEngine(spec, O.init_weights(spec, np.random.default_rng(5)))
        model2 = _model(eng2, kind, cs, cp)
        model2.compile(_make_opt(which), "mse")
        model2.load_weights(f)
        assert eng2.t == 5 and np.array_equal(eng2.theta, eng.theta.astype(np.float32))
        for s in range(nslot):
            assert np.array_equal(eng2.get_opt_slot(s), eng.get_opt_slot(s))
        model.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
        model2.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
        assert np.array_equal(eng2.theta, eng.theta)
        # another optimizer: weights only, with a warning
        eng3 = OptEngine(spec, O.init_weights(spec, np.random.default_rng(6)))
        model3 = _model(eng3, kind, cs, cp)
        model3.compile(Lion() if which != "lion" else AdaBeliefOptimizer(), "mse")
        with pytest.warns(UserWarning, match="not restored"):
            model3.load_weights(f)
        assert eng3.t == 0 and np.array_equal(eng3.theta, eng.theta.astype(np.float32) * 0 + eng3.theta)
    # amsgrad must match too; and an Adam file into a Lion model: weights only
    eng4 = OptEngine(spec, ws)
    model4 = _model(eng4, kind, cs, cp)
    model4.compile(AdaBeliefOptimizer(), "mse")
    with pytest.warns(UserWarning):
        model4.load_weights(str(tmp_path / "adabelief_ams"))
    assert eng4.t == 0
    eng5 = OptEngine(spec, ws)
    model5 = _model(eng5, kind, cs, cp)
    model5.compile(Adam(1e-3), "mse")
    model5.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
    model5.save_weights(str(tmp_path / "adam"))
    assert "adam_m" in np.load(str(tmp_path / "adam.npz")) and "opt_kind" not in np.load(str(tmp_path / "adam.npz"))
    model5.compile(Lion(), "mse")
    with pytest.warns(UserWarning):
        model5.load_weights(str(tmp_path / "adam"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model5.compile(Adam(1e-3), "mse")
        model5.load_weights(str(tmp_path / "adam"))
    assert eng5.t == 5


# ---- two gloo processes, uneven shards -----------------------------------------------------------------------------------------
N_LOCAL = (40, 25)
BS = 16
L2 = 1e-3


def _worker(rank, world, port, which, outdir):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank)})
    import torch.distributed as td
    td.init_process_group("gloo")
    from nif_amd import distributed as dist
    from tests.doubles import GlooComm
    comm = dist.install(GlooComm())
    kind, cs, cp, spec, ws, x, y = _problem(n=sum(N_LOCAL))
    n_pnet = sum(int(np.prod(s)) for nm, s in spec.param_shapes() if nm.startswith("pnet_"))
    eng = OptEngine(spec, ws, (0.0, L2, 0, n_pnet))
    model = _model(eng, kind, cs, cp)
    model.compile(_make_opt(which), "mse")
    lo = sum(N_LOCAL[:rank]); hi = lo + N_LOCAL[rank]
    h = model.fit(x[lo:hi], y[lo:hi], batch_size=BS, epochs=2, shuffle=False, verbose=0)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), theta=eng.theta, loss=np.array(h.history["loss"]), nred=comm.n_grad_reduces,
             nopt=len([c for c in eng.calls if c[0] == "opt_step"]))
    dist.shutdown()
    if td.is_initialized():
        td.destroy_process_group()


@pytest.mark.parametrize("which", ["lion", "adabelief_ams"])
def test_two_rank_fit_updates_after_the_all_reduce_with_replicated_state(which, tmp_path):
    pytest.importorskip("torch")
    import torch.multiprocessing as mp
    from tests.test_distributed import _free_port
    mp.spawn(_worker, args=(2, _free_port(), which, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert int(r0["nred"]) == int(r1["nred"]) == 6 and int(r0["nopt"]) == int(r1["nopt"]) == 6
    assert np.array_equal(r0["theta"], r1["theta"]) and np.array_equal(r0["loss"], r1["loss"])
    # serial emulation: every step is the union of the ranks' rows of that step (+ L2 on the ParameterNet) and one restated update
    kind, cs, cp, spec, ws, x, y = _problem(n=sum(N_LOCAL))
    n_pnet = sum(int(np.prod(s)) for nm, s in spec.param_shapes() if nm.startswith("pnet_"))
    hyper = _hyper(_make_opt(which).as_opt())
    th = O.flatten(ws); m = np.zeros_like(th, dtype=np.float32); v = m.copy(); vh = m.copy(); t = 0
    for _ in range(2):
        for ib in range(3):
            rows = []
            for r in range(2):
                lo = sum(N_LOCAL[:r]) + ib * BS
                rows += list(range(lo, min(lo + BS, sum(N_LOCAL[:r + 1]))))
            rows = np.array(rows)
            _, grads = O.loss_and_grad(spec, O.unflatten(spec, th), x[rows].astype(np.float64), y[rows].astype(np.float64))
            g = O.flatten(grads)
            g[:n_pnet] += 2 * L2 * th[:n_pnet]
            t += 1
            th, m, v, vh2 = opt_apply(th, g.astype(np.float32), m, v, vh, hyper, t)
            vh = vh2 if vh2 is not None else vh
    # (the ranks' all-reduce sums fp64 shard gradients in another order than the serial batch; measured max |diff| 0 for both
    # optimizers, the bar leaves room for a rounding-level difference that the fp32 update carries one ulp further)
    assert np.abs(r0["theta"] - th).max() < 1e-6
