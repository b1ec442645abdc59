"""The host half of Model.encode_snapshots: Levenberg-Marquardt in the latent, one problem per snapshot, all snapshots
advanced together.  NumPy only, float64.  The device's part is one call per iteration: `normal_eq(latents [T, r] float32)` returns the
float64 Gram matrices S [T, r + 1, r + 1] of the augmented rows [du/dz, u - y] at those latents -- A = S[:r, :r] = J^T W J,
g = S[:r, r] = J^T W e, c = S[r, r] = sum w |e|^2 (Engine.snapshot_normal_eq; the tests pass a float64 reference instead)."""
import collections

import numpy as np

EncodeResult = collections.namedtuple("EncodeResult", ["latent", "loss", "iterations", "converged"])

LAMBDA0, LAMBDA_DOWN, LAMBDA_UP = 1e-3, 3.0, 2.0
EPS_REL = 1e-12      # the absolute floor of the damping, relative to the largest diagonal entry of A


def lm_step(A, g, lam):
    """(A + lam diag(A) + eps I) delta = -g for one snapshot.  A singular A (fewer samples than latent dimensions, or a latent
    direction the samples do not see) leaves g in A's range: the eps I floor makes the system solvable and the step has no component
    along the unseen directions beyond eps's"""
    d = np.diag(A)
    eps = EPS_REL * max(float(d.max()) if d.size else 0.0, 0.0) + 1e-300
    return np.linalg.solve(A + lam * np.diag(d) + eps * np.eye(A.shape[0]), -g)


def lm_encode(normal_eq, latent0, counts, so, max_iter=20, tol=1e-8):
    """Minimise c_t(z) = sum_m w_m |u(z; x_m) - y_m|^2 per snapshot from latent0 [T, r].  counts [T]: points per snapshot (an empty
    snapshot keeps its latent).  Each snapshot has its own damping lam_t: a trial z + delta is accepted when c fell (lam /= 3, the
    trial's S is reused), else rejected (lam *= 2).  A snapshot is converged when the relative decrease of c of an accepted step, or
    |delta| / |z| of a solved step, is below tol, when the step no longer changes the float32 latent, or when c is 0; converged
    snapshots keep their latent through the remaining calls.  One normal_eq call per iteration: at most max_iter + 1 in all.
    Returns EncodeResult(latent float32 [T, r], loss [T] = c / (so M_t), Keras' mse of the snapshot (0 for an empty one),
    iterations [T], converged [T])."""
    z = np.array(latent0, dtype=np.float32, ndmin=2)
    T, r = z.shape
    counts = np.asarray(counts, dtype=np.int64).reshape(T)
    iters = np.zeros(T, dtype=np.int64)
    done = counts == 0
    lam = np.full(T, LAMBDA0)
    c = np.zeros(T)
    if T and not done.all():
        S = np.array(normal_eq(z), dtype=np.float64)
        c = S[:, r, r].copy()
        done |= ~(c > 0.0)
        for _ in range(int(max_iter)):
            trial = z.copy()
            live = []
            for t in np.flatnonzero(~done):
                delta = lm_step(S[t, :r, :r], S[t, :r, r], lam[t])
                zt = (z[t].astype(np.float64) + delta).astype(np.float32)
                if np.linalg.norm(delta) <= tol * np.linalg.norm(z[t].astype(np.float64)) or np.array_equal(zt, z[t]):
                    done[t] = True
                    continue
                trial[t] = zt
                live.append(t)
            if not live:
                break
            St = np.array(normal_eq(trial), dtype=np.float64)
            for t in live:
                iters[t] += 1
                ct = St[t, r, r]
                if ct < c[t]:
                    rel = (c[t] - ct) / c[t]
                    z[t], S[t], c[t] = trial[t], St[t], ct
                    lam[t] /= LAMBDA_DOWN
                    if rel < tol or not ct > 0.0:
                        done[t] = True
                else:
                    lam[t] *= LAMBDA_UP
    loss = np.where(counts > 0, c / np.maximum(counts * int(so), 1), 0.0)
    return EncodeResult(z, loss, iters, done.copy())
