"""fp64 reference of the second-order Sobolev step: what Keras computes for
    Model(x, HessianLayer(model, y_index, x_index)(x)).compile(opt, loss, loss_weights=[w0, w1, w2])
(reference nif/layers/gradient.py:130-180, :234-261).  torch_ref.forward and autograd three levels deep: the Jacobian and the
Hessian with create_graph=True, then the gradient of the loss with respect to the weights."""
import numpy as np
import torch

from tests import torch_ref


def sobolev2_loss_and_grad(kind, cs, cp, ws_np, inputs_np, y_np, dydx_np, d2_np, y_index, x_index, loss_weights=(1.0, 1.0, 1.0),
                           sw_np=None, loss="mse", want_grad=True):
    """loss = 1/B sum_a sw_a (w0 mean_i l(u - y) + w1 mean_{i in Y, j} l(J - G) + w2 mean_{i in Y, j, k} l(H - T)).
    dydx_np [B, ny, nx], d2_np [B, ny, nx, nx] in y_index / x_index order.  Returns (loss, grads per weight, u, J, H)."""
    w0, w1, w2 = [float(v) for v in loss_weights]
    ws = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws_np]
    inputs = torch.tensor(inputs_np, dtype=torch.float64, requires_grad=True)
    y = torch.tensor(y_np, dtype=torch.float64)
    G = torch.tensor(np.asarray(dydx_np), dtype=torch.float64)
    T = torch.tensor(np.asarray(d2_np), dtype=torch.float64)
    xi, yi = list(x_index), list(y_index)
    u = torch_ref.forward(kind, cs, cp, ws, inputs)
    jrows, hrows = [], []
    for i in yi:
        g, = torch.autograd.grad(u[:, i].sum(), inputs, create_graph=True)
        jrows.append(g[:, xi])
        hcols = []
        for j in xi:
            h, = torch.autograd.grad(g[:, j].sum(), inputs, create_graph=True)
            hcols.append(h[:, xi])
        hrows.append(torch.stack(hcols, 1))
    J = torch.stack(jrows, 1)
    H = torch.stack(hrows, 1)
    le = lambda e: torch_ref._loss_elem(loss, e)
    per = w0 * le(u - y).mean(dim=1) + w1 * le(J - G).mean(dim=(1, 2)) + w2 * le(H - T).mean(dim=(1, 2, 3))
    if sw_np is not None:
        per = per * torch.tensor(np.asarray(sw_np), dtype=torch.float64)
    L = per.sum() / u.shape[0]
    grads = None
    if want_grad:
        grads = [g.numpy() if g is not None else np.zeros(w.shape) for g, w in
                 zip(torch.autograd.grad(L, ws, allow_unused=True), ws)]
    return L.item(), grads, u.detach().numpy(), J.detach().numpy(), H.detach().numpy()
