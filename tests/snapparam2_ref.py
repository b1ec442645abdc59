"""float64 reference of the latent route of Model.predict_snapshot_parameter_derivatives(order=2) (imported, not collected;
tests/test_snapshot_param_second_derivatives.py, tests/test_gpu_snapshot_param_second_derivatives.py): second directional derivatives
of the field in the latent z, and mixed in (z, x), by torch autograd in float64 through tests/encode_ref.py's restatement of the field
-- its approach one order higher.  Also the oracle's dz/dp and d2z/dp2 as the directions that make the latent route the p= route."""
import numpy as np

from oracle import nif_oracle as O
from tests.encode_ref import _torch_field


def latent_second(spec, ws, z, dirs, d2dirs, x, x_index=()):
    """One snapshot: latent z [r], directions dirs [nd, r], second directions d2dirs [nd, nd, r] (or None: zeros), points x [M, si] ->
    (u [M, so], dudp [M, so, nd], d2udp2 [M, so, nd, nd], dudx [M, so, nx], d2udpdx [M, so, nd, nx]) in float64:
        dudp[m, i, a]       = du_i/dz . dirs[a]
        d2udp2[m, i, a, b]  = dirs[a] . d2u_i/dz2 . dirs[b] + du_i/dz . d2dirs[a, b]
        d2udpdx[m, i, a, j] = d/dx_j (du_i/dz . dirs[a])
    The rows of the tiled latent are independent, so one backward pass through a sum over the points serves them all."""
    import torch
    x = np.asarray(x, dtype=np.float64)
    dirs = np.asarray(dirs, dtype=np.float64)
    M, so, nd, xi = x.shape[0], spec.so, dirs.shape[0], list(x_index)
    dd = np.zeros((nd, nd, spec.r)) if d2dirs is None else np.asarray(d2dirs, dtype=np.float64)
    if M == 0:
        return (np.zeros((0, so)), np.zeros((0, so, nd)), np.zeros((0, so, nd, nd)), np.zeros((0, so, len(xi))), np.zeros((0, so, nd, len(xi))))
    tw = [torch.tensor(np.asarray(w, dtype=np.float64)) for w in ws]
    lat = torch.tensor(np.tile(np.asarray(z, dtype=np.float64), (M, 1)), requires_grad=True)
    xt = torch.tensor(x, requires_grad=True)
    td, tdd = torch.tensor(dirs), torch.tensor(dd)
    u = _torch_field(spec, tw, lat, xt)
    J = np.zeros((M, so, nd)); H = np.zeros((M, so, nd, nd)); Jx = np.zeros((M, so, len(xi))); Hx = np.zeros((M, so, nd, len(xi)))
    for i in range(so):
        g, gx = torch.autograd.grad(u[:, i].sum(), (lat, xt), create_graph=True)
        J[:, i] = (g @ td.T).detach().numpy()
        Jx[:, i] = gx.detach().numpy()[:, xi]
        first = torch.einsum("mk,abk->mab", g, tdd).detach().numpy()
        for a in range(nd):
            ga = (g * td[a]).sum()
            if ga.requires_grad:
                hz, hx = torch.autograd.grad(ga, (lat, xt), retain_graph=True, allow_unused=True)
            else:      # (a field that is linear in z and does not couple it with x: nothing left to differentiate)
                hz, hx = None, None
            if hz is not None:
                H[:, i, a] = (hz @ td.T).numpy()
            if hx is not None:
                Hx[:, i, a] = hx.numpy()[:, xi]
        H[:, i] += first
    return u.detach().numpy(), J, H, Jx, Hx


def pnet_directions(spec, ws, p, cols):
    """The directions that turn the latent route into the p= route: for the rows p [T, pi] and the parameter columns `cols`
    -> (z [T, r], dz/dp [T, nd, r], d2z/dp2 [T, nd, nd, r]) in float64 from oracle.nif_oracle.pnet_tangents2 (last-layer class: of the
    coefficient vector a = z last_w + last_b)"""
    p = np.asarray(p, dtype=np.float64)
    ws = [np.asarray(w, dtype=np.float64) for w in ws]
    nd = len(cols)
    z = None
    dz = np.zeros((p.shape[0], nd, spec.r)); ddz = np.zeros((p.shape[0], nd, nd, spec.r))
    for a in range(nd):
        for b in range(a, nd):
            z, za, zb, zab = O.pnet_tangents2(spec, ws, p, cols[a], cols[b])
            dz[:, a], dz[:, b] = za, zb
            ddz[:, a, b] = zab
            ddz[:, b, a] = zab
    if spec.kind == O.KIND_LL:
        lw, lb = O._pnet_split(spec, ws)[3]
        z, dz, ddz = z @ lw + lb, dz @ lw, ddz @ lw
    return z, dz, ddz
