"""NumPy restatement of Keras 2.11's SGD, RMSprop, Adagrad, Adamax, Adam (with amsgrad) and AdamW updates and of its ExponentialDecay,
InverseTimeDecay, CosineDecay and PolynomialDecay schedules, written from the formulas, for the tests of the k_opt.hip kernels.  The
formulas are restated from Keras 2.11; no TensorFlow run pins them.

* `schedule_lr(o, step)`: the learning rate of a nif_opt (its float32 constants, as the kernels receive them) at Keras' step, fp64.
* `step_lr(o, t)`: the learning rate of iteration t = step + 1 of a nif_opt with or without a schedule, fp64.
* `update(o, t, th, g, s0, s1, s2)`: one update in float32 arithmetic, one rounding per operation in the order the kernels run them
  (contraction off); s0, s1, s2 are the optimizer slots by index (Adam m, v, vhat; SGD m; RMSprop v, mom, a; Adagrad acc; Adamax m, u)."""
import numpy as np

f32 = np.float32

ADAM, SGD, RMSPROP, ADAGRAD, ADAMAX = 0, 3, 4, 5, 6
AMSGRAD, NESTEROV, CENTERED, DECOUPLED_WD = 2, 4, 8, 16
EXPONENTIAL, INVERSE_TIME, COSINE, POLYNOMIAL = 1, 2, 3, 4
STAIRCASE, CYCLE = 0x100, 0x200


def schedule_lr(o, step):
    step = float(step)
    lr, ds, a, b = float(f32(o.lr)), float(o.decay_steps), float(f32(o.sched_a)), float(f32(o.sched_b))
    k = o.sched & 0xff
    if k in (EXPONENTIAL, INVERSE_TIME):
        p = step / ds
        if o.sched & STAIRCASE:
            p = np.floor(p)
        return lr * a ** p if k == EXPONENTIAL else lr / (1.0 + a * p)
    if k == COSINE:
        q = min(step, ds) / ds
        return lr * ((1.0 - a) * 0.5 * (1.0 + np.cos(np.pi * q)) + a)
    if k == POLYNOMIAL:
        if o.sched & CYCLE:
            ds = ds * max(1.0, np.ceil(step / ds))
        q = min(step, ds) / ds
        return (lr - a) * (1.0 - q) ** b + a
    return lr


def step_lr(o, t):
    return schedule_lr(o, t - 1) if o.sched else float(f32(o.lr))


def update(o, t, th, g, s0, s1, s2):
    """(theta, s0, s1, s2) after iteration t >= 1 of the nif_opt `o`; float32 arrays in and out, unused slots returned as given"""
    th, g, s0, s1, s2 = (np.asarray(a, dtype=f32) for a in (th, g, s0, s1, s2))
    lr64 = step_lr(o, t)
    lr = f32(lr64)
    b1, b2, eps = f32(o.beta1), f32(o.beta2), f32(o.eps)
    one = f32(1)
    with np.errstate(all="ignore"):
        if o.kind == SGD:
            s = lr * g
            if b1 == 0:
                return (th - s).astype(f32), s0, s1, s2
            m = b1 * s0 - s
            th = th + (b1 * m - s) if o.flags & NESTEROV else th + m
            return th.astype(f32), m.astype(f32), s1, s2
        if o.kind == RMSPROP:            # b1 = momentum, b2 = rho
            v = b2 * s0 + (one - b2) * (g * g)
            d = v
            if o.flags & CENTERED:
                s2 = b2 * s2 + (one - b2) * g
                d = v - s2 * s2
            d = d + eps
            inc = lr * g / np.sqrt(d)
            if b1 > 0:
                s1 = b1 * s1 + inc
                th = th - s1
            else:
                th = th - inc
            return th.astype(f32), v.astype(f32), s1.astype(f32), s2.astype(f32)
        if o.kind == ADAGRAD:
            acc = s0 + g * g
            return (th - lr * g / np.sqrt(acc + eps)).astype(f32), acc.astype(f32), s1, s2
        if o.kind == ADAMAX:
            lr_t = f32(lr64 / (1.0 - float(b1) ** t))
            m = s0 + (g - s0) * (one - b1)
            u = np.maximum(b2 * s1, np.abs(g))
            return (th - lr_t * m / (u + eps)).astype(f32), m.astype(f32), u.astype(f32), s2
        assert o.kind == ADAM
        if o.flags & DECOUPLED_WD:
            th = th - lr * f32(o.weight_decay) * th
        lr_t = f32(lr64 * np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t))
        m = s0 + (g - s0) * (one - b1)
        # v + (g^2 - v)(1 - b2) rounded once (the kernel's fmaf): the product g g is a float32, the rest exact in float64
        gg = (g * g).astype(f32)
        v = ((gg.astype(np.float64) - s1.astype(np.float64)).astype(f32).astype(np.float64) * float(one - b2) + s1.astype(np.float64)).astype(f32)
        den = v
        if o.flags & AMSGRAD:
            s2 = np.maximum(s2, v)
            den = s2
        th = th - lr_t * m / (np.sqrt(den) + eps)
        return th.astype(f32), m.astype(f32), v.astype(f32), s2.astype(f32)


def rel_l2(a, b):
    """|a - b|_2 / |b|_2 in float64 (0 where both are all zero)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.linalg.norm(b)
    d = np.linalg.norm(a - b)
    return 0.0 if d == 0.0 else d / max(n, 1e-300)
