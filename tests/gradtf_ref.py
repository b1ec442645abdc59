"""NumPy restatement of the gradient transform (k_gradtf.hip; include/nif_hip.h nif_set_grad_transform), written from the formulas of
the reference's centralized_gradients_for_optimizer (nif/optimizers/gtcf.py:7-67) and the published behaviour of tf.clip_by_value,
tf.clip_by_norm and tf.clip_by_global_norm, for the tests of the kernels.

A layout is a list of (name, offset, rows, cols) as Engine.layout() returns it (cols == 0: a vector); a spec is the dict
Engine.set_grad_transform takes: centralize, gtcf (bool), clipnorm, clipvalue, global_clipnorm (0 / None = off).  Stages, in order:
1 centralise the matrices over their rows; Keras route (gtcf false), one of: 2 clamp, 3 per-tensor norm, 4a global norm; gtcf route:
4b global norm (legacy clip_norm), 5 clamp.

* `transform64`: the meaning, in float64 -> (g, per-tensor norms, global norm); the norms are those of the gradient in front of the
  norm stage (behind stage 1 and stage 2).
* `transform32`: the float sequence of the kernels, one rounding per operation in their summation order:
    - a work block is 64 columns of a matrix over all rows, or a chunk of 4096 floats of a vector laid out [rows][64];
    - per column four partial sums over the rows rg, rg + 4, ... (rg = 0..3) in order, added as (s0 + s1) + (s2 + s3);
      mean = sum / rows; x = g - mean; the squares x x add the same way, then the 64 columns of the block by the halving tree
      v[l] += v[l + 32], 16, 8, 4, 2, 1: one partial per block;
    - a sum over partials (a tensor's, or all of them in block order): 256 accumulators a[t] += p[t], p[t + 256], ... in order, then
      the halving tree a[t] += a[t + 128], 64, ..., 1; norm = sqrt(sum);
    - per element: (x c) / max(n_t, c);  x (c min(1 / n, 1 / c));  (x c) / n where n >= c;  min(max(x, -c), c)."""
import numpy as np

f32 = np.float32
VEC_CHUNK = 4096


def _on(spec, key):
    v = spec.get(key)
    return float(v) if v else 0.0


def plan(spec):
    """(centralise, stage, clamp in front of / without a norm stage, clamp behind it); stage 0 none, 3 per tensor, 4 Keras global, 5 gtcf"""
    gtcf = bool(spec.get("gtcf"))
    cn, cv, gc = _on(spec, "clipnorm"), _on(spec, "clipvalue"), _on(spec, "global_clipnorm")
    if not gtcf:
        assert (cn > 0) + (cv > 0) + (gc > 0) <= 1, "Keras route: one of clipnorm, clipvalue, global_clipnorm"
    else:
        assert gc == 0
    stage = (5 if cn > 0 else 0) if gtcf else (3 if cn > 0 else (4 if gc > 0 else 0))
    return bool(spec.get("centralize")), stage, (stage == 0 and cv > 0), (stage != 0 and gtcf and cv > 0)


def _tensor(g, d):
    name, off, rows, cols = d
    n = rows * (cols if cols else 1)
    return g[off:off + n].reshape((rows, cols) if cols else (rows,))


# ---- float64: the meaning -------------------------------------------------------------------------------------------------------
def transform64(g, layout, spec):
    g = np.array(g, dtype=np.float64)
    cen, stage, clamp_a, clamp_b = plan(spec)
    cn, cv, gc = _on(spec, "clipnorm"), _on(spec, "clipvalue"), _on(spec, "global_clipnorm")
    with np.errstate(all="ignore"):
        for d in layout:
            t = _tensor(g, d)
            if cen and d[3] > 0:
                t -= t.mean(axis=0, keepdims=True)
            if clamp_a:
                t[...] = np.minimum(np.maximum(t, -cv), cv)
        per = np.array([np.sqrt(np.sum(_tensor(g, d) ** 2)) for d in layout])
        glob = np.sqrt(np.sum(per ** 2))
        for d, n in zip(layout, per):
            t = _tensor(g, d)
            if stage == 3:
                t[...] = (t * cn) / max(n, cn)
            elif stage == 4:
                t[...] = t * (gc * min(1.0 / glob, 1.0 / gc)) if np.isfinite(glob) else np.nan
            elif stage == 5 and glob >= cn:
                t[...] = (t * cn) / glob
            if clamp_b:
                t[...] = np.minimum(np.maximum(t, -cv), cv)
    return g, per, glob


# ---- float32: the kernels' float sequence -----------------------------------------------------------------------------------------
def _rows4(a, square=False):
    """per column: four in-order sums over the rows rg, rg + 4, ..., added as (s0 + s1) + (s2 + s3); a is [rows, cols] float32"""
    s = []
    for rg in range(4):
        acc = np.zeros((a.shape[1],), f32)
        for i in range(rg, a.shape[0], 4):
            acc = acc + (a[i] * a[i] if square else a[i])
        s.append(acc)
    return (s[0] + s[1]) + (s[2] + s[3])


def _tree(v):
    """halving tree along the last axis (a power of two long)"""
    v = v.copy()
    h = v.shape[-1] // 2
    while h > 0:
        v = v[..., :h] + v[..., h:2 * h]
        h //= 2
    return v[..., 0]


def _partials(colq):
    """[ncols] column sums of squares -> one partial per block of 64 columns"""
    nb = (colq.size + 63) // 64
    p = np.zeros((nb * 64,), f32)
    p[:colq.size] = colq
    return _tree(p.reshape(nb, 64))


def block_sum(p):
    p = np.asarray(p, f32)
    k = (p.size + 255) // 256
    a = np.zeros((k * 256,), f32)
    a[:p.size] = p
    acc = np.zeros((256,), f32)
    for row in a.reshape(k, 256):
        acc = acc + row
    return f32(_tree(acc))


def transform32(g, layout, spec):
    """-> (g float32, per-tensor norms float32, global norm float32)"""
    g = np.array(g, dtype=f32)
    cen, stage, clamp_a, clamp_b = plan(spec)
    cn, cv, gc = f32(_on(spec, "clipnorm")), f32(_on(spec, "clipvalue")), f32(_on(spec, "global_clipnorm"))
    parts = []
    with np.errstate(all="ignore"):
        for d in layout:
            name, off, rows, cols = d
            if cols > 0:
                t = _tensor(g, d)
                if cen:
                    t -= _rows4(t) / f32(rows)
                if clamp_a:
                    t[...] = np.minimum(np.maximum(t, -cv), cv)
                parts.append(_partials(_rows4(t, square=True)))
            else:
                t = _tensor(g, d)
                if clamp_a:
                    t[...] = np.minimum(np.maximum(t, -cv), cv)
                pt = []
                for e0 in range(0, rows, VEC_CHUNK):
                    ch = t[e0:e0 + VEC_CHUNK]
                    r = (ch.size + 63) // 64
                    a = np.zeros((r * 64,), f32)
                    a[:ch.size] = ch
                    pt.append(_partials(_rows4(a.reshape(r, 64), square=True))[0])
                parts.append(np.array(pt, f32))
        per = np.array([np.sqrt(block_sum(p)) for p in parts], f32)
        glob = f32(np.sqrt(block_sum(np.concatenate(parts))))
        for d, n in zip(layout, per):
            t = _tensor(g, d)
            if stage == 3:
                t[...] = (t * cn) / (n if (np.isnan(n) or n > cn) else cn)
            elif stage == 4:
                if np.isfinite(glob):
                    a, b = f32(1) / glob, f32(1) / gc
                    t[...] = t * (gc * (a if a < b else b))
                else:
                    t[...] = np.nan
            elif stage == 5 and glob >= cn:
                t[...] = (t * cn) / glob
            if clamp_b:
                t[...] = np.minimum(np.maximum(t, -cv), cv)
    return g, per, glob


def ulps(a, b):
    """|a - b| in units of the float32 spacing at max(|a|, |b|) (0 where both are equal, both NaN included)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(f32)).astype(np.float64)
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        same = (d == 0) | (np.isnan(a) & np.isnan(b))
        return np.where(same, 0.0, d / sp)
