"""NumPy restatement of the reference's Lion and AdaBelief updates (nif/optimizers/external_optimizers.py: Lion's dense apply
:682-703, AdaBelief's :456-530), written from the formulas, for the tests of the k_opt.hip kernels.

* `scalars(opt, t)`: the per-step scalars in fp64 -- lr_d = lr / (1 + decay (t-1)), AdaBelief's warm-up / decay, 1 - b^t, r_t and the
  branch -- from the optimizer object's attributes.
* `lion(...)` / `adabelief(...)`: one update in float32 arithmetic, one rounding per operation in the order the formulas are written
  (the kernels run the same order with contraction off)."""
import numpy as np

f32 = np.float32


def scalars(opt, t):
    """(lr_t, 1 - b1^t, 1 - b2^t, r_t, divides) for iteration t >= 1"""
    t = float(t)
    lr = float(f32(opt.learning_rate))
    decay = float(f32(opt.decay))
    if decay != 0.0:
        lr = lr / (1.0 + decay * (t - 1.0))
    b1, b2 = float(f32(opt.beta_1)), float(f32(opt.beta_2))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    r, div = 1.0, True
    if getattr(opt, "kind", 1) == 2:
        if opt.total_steps > 0:
            w = float(opt.total_steps) * float(f32(opt.warmup_proportion))
            ds = max(float(opt.total_steps) - w, 1.0)
            rate = (float(f32(opt.min_lr)) - lr) / ds
            lr = lr * (t / w) if t <= w else lr + rate * min(t - w, ds)
        if opt.rectify:
            sma_inf = 2.0 / (1.0 - b2) - 1.0
            sma_t = sma_inf - 2.0 * t * b2 ** t / (1.0 - b2 ** t)
            if sma_t >= float(f32(opt.sma_threshold)):
                r = np.sqrt((sma_t - 4.0) / (sma_inf - 4.0) * (sma_t - 2.0) / (sma_inf - 2.0) * sma_inf / sma_t)
            else:
                div = False
    return lr, bc1, bc2, r, div


def sma(beta_2, t):
    b2 = float(f32(beta_2))
    sma_inf = 2.0 / (1.0 - b2) - 1.0
    return sma_inf - 2.0 * t * b2 ** t / (1.0 - b2 ** t)


def lion(th, g, m, opt, t):
    """(theta, m) after one Lion step; float32 in, float32 out"""
    th, g, m = (np.asarray(a, dtype=f32) for a in (th, g, m))
    lr = f32(scalars(opt, t)[0])
    b1, b2, wd = f32(opt.beta_1), f32(opt.beta_2), f32(opt.wd)
    with np.errstate(all="ignore"):
        c = m * b1 + g * (f32(1) - b1)
        s = np.sign(c).astype(f32)
        th_new = th - lr * (s + th * wd)
        m_new = m * b2 + g * (f32(1) - b2)
    return th_new.astype(f32), m_new.astype(f32)


def lion_c(g, m, opt):
    """Lion's c = b1 m + (1-b1) g in fp64 and the size of its larger term (where fp32 may round the sign either way)"""
    b1 = float(f32(opt.beta_1)); ob1 = float(f32(1) - f32(opt.beta_1))
    a, b = np.asarray(m, np.float64) * b1, np.asarray(g, np.float64) * ob1
    return a + b, np.maximum(np.abs(a), np.abs(b))


def adabelief(th, g, m, v, vhat, opt, t):
    """(theta, m, v, vhat) after one AdaBelief step (vhat None without amsgrad); float32"""
    th, g, m, v = (np.asarray(a, dtype=f32) for a in (th, g, m, v))
    lr, bc1, bc2, r, div = scalars(opt, t)
    lr, bc1, bc2, r = f32(lr), f32(bc1), f32(bc2), f32(r)
    b1, b2, eps, wd = f32(opt.beta_1), f32(opt.beta_2), f32(opt.epsilon), f32(opt.weight_decay)
    with np.errstate(all="ignore"):
        m_new = b1 * m + (f32(1) - b1) * g
        d = g - m_new
        v_new = (b2 * v + (f32(1) - b2) * (d * d)) + eps
        vv = v_new
        vh_new = None
        if opt.amsgrad:
            vh_new = np.maximum(np.asarray(vhat, dtype=f32), v_new)
            vv = vh_new
        mh = m_new / bc1
        u = (r * mh) / (np.sqrt(vv / bc2) + eps) if div else mh
        if wd != 0:
            u = u + wd * th
        th_new = th - lr * u
    return th_new.astype(f32), m_new.astype(f32), v_new.astype(f32), None if vh_new is None else vh_new.astype(f32)


def ulps(a, b):
    """|a - b| in units of the float32 spacing at max(|a|, |b|) (0 where both are equal, including both zero)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(f32)).astype(np.float64)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return np.where(d == 0, 0.0, d / sp)
