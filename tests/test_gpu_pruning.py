"""GPU tests of low-magnitude pruning (k_prune.hip, nif_prune_*, nif_amd.sparsity): the device select against NumPy's sort, bit for
bit; mask and apply; a pruned fit against the manual sequence of engine calls with the masks checked against NumPy's masks of the same
weights at every pruning turn (teacher forcing); the mixed policies; save / load / continue."""
import numpy as np
import pytest

from tests import prune_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def big_engine():
    """an engine whose flat parameter vector (8.5 M floats) holds every synthetic segment"""
    import nif_amd
    from tests.test_gpu_parity import _cfg
    kind, cs, cp = _cfg("NIFMultiScale", 128, 8, 16, 1, 64, 1, 1, 1, p_act="swish")
    nif_amd.set_seed(0)
    m = nif_amd.NIFMultiScale(cs, cp)
    e = m._engine
    assert e.n_params > 8_000_000
    yield e
    e.prune_config([], [])


def _synthetic(P, rng):
    th = (0.1 * rng.standard_normal(P)).astype(f32)
    segs = []

    def put(off, vals):
        th[off:off + len(vals)] = vals
        segs.append((off, len(vals)))

    put(0, [f32(-0.3)])                                                            # size 1
    put(1, rng.standard_normal(7).astype(f32))                                     # unaligned, tiny
    put(9, rng.choice(np.array([0.5, -0.5, 0.25, 0.0, -0.0], f32), 1000))           # heavy ties
    put(1013, np.where(rng.random(4096) < 0.5, f32(0.0), f32(-0.0)).astype(f32))   # all zero, both signs
    den = (rng.integers(1, 1 << 23, 3001).astype(np.uint32)).view(f32) * np.where(rng.random(3001) < 0.5, f32(1), f32(-1))
    den[::7] = f32(-0.0)
    put(5203, den.astype(f32))                                                     # denormals and negative zeros
    put(8301, rng.standard_normal(4099).astype(f32))
    put(12503, (rng.standard_normal(65537) * 1e-3).astype(f32))
    put(80005, (0.1 * rng.standard_normal(4_000_003)).astype(f32))                  # ~4 M
    put(4_100_001, (1.0 + rng.random(1_000_000)).astype(f32))                      # one exponent: the later digits decide
    return th, segs


def _check_round(e, th, segs, ks):
    e.set_flat(th)
    e.prune_update(ks)
    masks, thr = e.get_prune_state()
    for (off, n), k, mk, t in zip(segs, ks, masks, thr):
        w = th[off:off + n]
        want = R.threshold(w, k)
        assert _bits(t) == _bits(want), (off, n, k, t, want)
        assert np.array_equal(mk, R.mask(w, want)), (off, n, k)
        assert int(mk.sum()) >= k
    e.prune_apply()
    got = e.get_flat()
    want = th.copy()
    for (off, n), mk in zip(segs, masks):
        want[off:off + n] = th[off:off + n] * mk
    assert np.array_equal(_bits(got), _bits(want))      # signed zeros included; outside the segments nothing changed


def test_select_mask_and_apply_are_bit_exact(big_engine):
    e = big_engine
    rng = np.random.default_rng(11)
    th, segs = _synthetic(e.n_params, rng)
    e.prune_config([o for o, _ in segs], [n for _, n in segs])
    ks1 = [1, 7, 500, 4096, 1, 2000, 65537, 1_234_567, 999_999]
    ks2 = [1, 1, 1000, 1, 3001, 4099, 1, 1, 1]
    ks3 = [1] + [max(1, int(rng.integers(1, n + 1))) for _, n in segs[1:]]
    for ks in (ks1, ks2, ks3):            # (the histograms must be empty again after every update)
        _check_round(e, th, segs, ks)
    # a state round trip and the refusals
    masks, thr = e.get_prune_state()
    e.set_prune_state(masks, thr)
    m2, t2 = e.get_prune_state()
    assert all(np.array_equal(a, b) for a, b in zip(masks, m2)) and np.array_equal(thr, t2)
    from nif_amd import NifError
    with pytest.raises(NifError):
        e.prune_update([0] + ks1[1:])
    with pytest.raises(NifError):
        e.prune_config([5, 4], [2, 2])         # overlapping
    e.prune_config([], [])
    with pytest.raises(NifError, match="not configured"):
        e.prune_apply()


def _opt(name):
    import nif_amd
    from nif_amd.optimizers import AdaBeliefOptimizer, Lion
    return {"adam": lambda: nif_amd.Adam(1e-3), "lion": lambda: Lion(learning_rate=1e-3, wd=1e-2),
            "adabelief": lambda: AdaBeliefOptimizer(learning_rate=1e-3)}[name]()


def _setup(kind_name, policy, seed):
    import nif_amd
    from tests.test_gpu_parity import _cfg
    kind, cs, cp = _cfg(kind_name, 64, 2, 32, 2, 1 if kind_name != "LL" else 4, 1, 1, 1, p_act="swish")
    cls = {"NIFMultiScale": nif_amd.NIFMultiScale, "LL": nif_amd.NIFMultiScaleLastLayerParameterized}[kind_name]
    nif_amd.set_seed(seed)
    return cls, cs, cp, policy


SCHED = dict(initial_sparsity=0.1, final_sparsity=0.7, begin_step=1, end_step=7, frequency=2)


@pytest.mark.parametrize("variant", ["adam", "lion", "adabelief", "adam_bf16", "adam_f16", "adam_ll"])
def test_pruned_fit_equals_the_manual_sequence(variant):
    """fit() with UpdatePruningStep for 3 epochs of 3 batches (pruning turns at steps 1, 3, 5, 7; epoch ends after steps 2, 5, 8)
    against the engine calls by hand, bit for bit; at every turn the device masks equal NumPy's masks of the weights read just
    before it; after fit every pruned tensor holds exactly size - k zeros"""
    import nif_amd
    from nif_amd import sparsity as S
    opt_name = variant.split("_")[0]
    policy = {"adam_bf16": "mixed_bfloat16", "adam_f16": "mixed_float16"}.get(variant, "float32")
    cls, cs, cp, _ = _setup("LL" if variant == "adam_ll" else "NIFMultiScale", policy, 4)
    x, y = nif_amd.data.synthetic_wave_batch(1500, seed=3)
    m1 = cls(cs, cp, mixed_policy=policy)
    base = m1.build()
    w0 = base.get_weights()
    pruned = S.prune_low_magnitude(base, pruning_schedule=S.PolynomialDecay(**SCHED))
    pruned.compile(_opt(opt_name), "mse")
    pruned.fit(x, y, epochs=3, batch_size=512, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    assert pruned.pruning_step == 8

    m2 = cls(cs, cp, mixed_policy=policy)
    model2 = m2.build()
    model2.set_weights(w0)
    e = m2._engine
    spec = m2._spec
    names = S.prunable_weights(model2)
    segs = R.segments(spec, names)
    e.prune_config([o for o, _ in segs], [n for _, n in segs])
    z = np.zeros((e.n_params,), f32)
    e.set_opt_state(z, z, 0)
    d_x, d_y = e.alloc(x.size), e.alloc(y.size)
    d_x.upload(x); d_y.upload(y)
    opt = _opt(opt_name)
    is_adam = opt_name == "adam"
    o = opt.as_struct() if is_adam else opt.as_opt()
    step, turns, last_k = 0, 0, None
    for _ in range(3):
        for b0 in range(0, 1500, 512):
            b = min(512, 1500 - b0)
            if R.should_prune(step, SCHED["begin_step"], SCHED["end_step"], SCHED["frequency"]):
                sp = R.poly_sparsity(step, SCHED["initial_sparsity"], SCHED["final_sparsity"], SCHED["begin_step"], SCHED["end_step"], 3)
                ks = [R.keep(n, sp) for _, n in segs]
                w = e.get_flat()
                e.prune_update(ks)
                masks, thr = e.get_prune_state()
                for (off, n), k, mk, t in zip(segs, ks, masks, thr):
                    want = R.threshold(w[off:off + n], k)
                    assert _bits(t) == _bits(want)
                    assert np.array_equal(mk, R.mask(w[off:off + n], want))
                turns += 1
                last_k = ks
            e.prune_apply()
            e.loss_grad_dev(d_x.at(b0 * 2), d_y.at(b0), None, b, b)
            (e.adam_step_dev if is_adam else e.opt_step_dev)(o)
            step += 1
        e.prune_apply()                     # UpdatePruningStep.on_epoch_end
    assert turns == 4
    got = m1._engine.get_flat()
    assert np.array_equal(_bits(got), _bits(e.get_flat()))
    m_a, _, t_a = m1._engine.get_opt_state()
    m_b, _, t_b = e.get_opt_state()
    assert t_a == t_b == 9 and np.array_equal(m_a, m_b)
    for (off, n), k in zip(segs, last_k):
        assert int(np.count_nonzero(got[off:off + n] == 0)) == n - k, (off, n, k)
    # predict applies the masks first (no change now: the epoch end applied them)
    u = pruned.predict(x[:64])
    assert np.array_equal(_bits(m1._engine.get_flat()), _bits(got)) and np.isfinite(u).all()


def test_save_load_continue_equals_an_uninterrupted_run(tmp_path):
    """two fit calls on one model against fit, save_weights, a new model, load_weights, fit (the step number of the second call
    repeats the first call's last one, as TF-MOT's callback does)"""
    import nif_amd
    from nif_amd import sparsity as S
    cls, cs, cp, _ = _setup("NIFMultiScale", "float32", 6)
    x, y = nif_amd.data.synthetic_wave_batch(1200, seed=5)
    sched = lambda: S.ConstantSparsity(0.6, begin_step=0, frequency=3)

    def fresh(w0=None):
        m = cls(cs, cp)
        b = m.build()
        if w0 is not None:
            b.set_weights(w0)
        p = S.prune_low_magnitude(b, pruning_schedule=sched())
        p.compile(nif_amd.Adam(1e-3), "mse")
        return m, p

    ma, a = fresh()
    w0 = a.get_weights()
    for _ in range(2):
        a.fit(x, y, epochs=2, batch_size=256, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    mb, b = fresh(w0)
    b.fit(x, y, epochs=2, batch_size=256, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    path = str(tmp_path / "pruned")
    b.save_weights(path)
    d = np.load(path + ".npz")
    assert int(d["pruning_step"]) == b.pruning_step == 9
    assert all("prune_mask_%s" % nm in d for nm in S.prunable_weights(b))
    mc, c = fresh()
    c.load_weights(path)
    assert c.pruning_step == 9
    c.fit(x, y, epochs=2, batch_size=256, shuffle=False, verbose=0, callbacks=[S.UpdatePruningStep()])
    assert np.array_equal(_bits(ma._engine.get_flat()), _bits(mc._engine.get_flat()))
    ms_a, ms_c = ma._engine.get_prune_state(), mc._engine.get_prune_state()
    assert all(np.array_equal(p, q) for p, q in zip(ms_a[0], ms_c[0])) and np.array_equal(ms_a[1], ms_c[1])
    # strip_pruning: the masked weights, pruning off on the engine
    plain = S.strip_pruning(c)
    assert not isinstance(plain, S.PrunedModel)
    flat = mc._engine.get_flat()
    for nm, off, n in S._segments(mc._spec):
        assert np.count_nonzero(flat[off:off + n] == 0) >= n - S.keep_count(n, 0.6)
