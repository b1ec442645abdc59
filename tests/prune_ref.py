"""NumPy restatement of low-magnitude pruning (tfmot.sparsity.keras 0.7.3, as nif_amd/sparsity.py states it) for the tests."""
import numpy as np


def keep(size, sparsity):
    """pruning_impl.py: k = max(round_half_even(float32(size) * (1 - float32(sparsity))), 1)"""
    return max(int(np.rint(np.float32(size) * (np.float32(1.0) - np.float32(sparsity)))), 1)


def threshold(w, k):
    """the k-th largest |w| (float32)"""
    return np.sort(np.abs(np.asarray(w, np.float32)).ravel())[::-1][k - 1]


def mask(w, thr):
    return (np.abs(np.asarray(w, np.float32)) >= thr).astype(np.float32)


def should_prune(step, begin, end, frequency):
    return step >= begin and (end < 0 or step <= end) and (step - begin) % frequency == 0


def poly_sparsity(step, initial, final, begin, end, power):
    f = np.float32
    p = min(f(1.0), max(f(0.0), f(step - begin) / f(end - begin)))
    return f(f(initial - final) * np.power(f(1.0) - f(p), f(power)) + f(final))


def segments(spec, names):
    """(offset, size) of the named tensors in the flat parameter vector"""
    out, off = [], 0
    for nm, s in spec.param_shapes():
        n = int(np.prod(s))
        if nm in names:
            out.append((off, n))
        off += n
    return out
