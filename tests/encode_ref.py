"""float64 references of Model.encode_snapshots (tests/test_encode.py, tests/test_gpu_encode.py): the field of a latent from the
oracle, its latent Jacobian twice over -- central differences of the oracle's field, and torch autograd through an independent
restatement of the ShapeNet (tests/torch_ref.py's tensor program entered at the latent) --, the normal equations built from them, and
an engine double that serves them to the host loop."""
import numpy as np

from oracle import nif_oracle as O


# the nets of tests/test_gpu_encode.py: r = 1; r = 3; r = 7 (three k_jac launches, 3 + 3 + 1 latents); class NIF; so = 2 on a padded
# width; the last-layer class; its smallest wide case (129 units, the layer-by-layer x -> phi route)
NETS = ["ms_cfg2_64x4", "ms_64x2_mlp_pnet_r3", "ms_32x2_r7_si3", "nif_cfg1_32x2", "nif_pad_n30_tanh_r2_so2", "ll_plain_32x2_r3", "w129x1"]


def net_cfg(name):
    """(kind, cfg_shape_net, cfg_parameter_net) of a net of NETS"""
    from tests.test_gpu_parity import CONFIGS
    from tests.wide_ll_cases import CASES
    return (CONFIGS[name] if name in CONFIGS else CASES[name])[0]


def _names(spec):
    return [nm for nm, _ in spec.param_shapes()]


def field(spec, ws, z, x):
    """u(z; x) [M, so] in float64: one latent z [r] on the points x [M, si] (model_lr_to_w + shapenet_given_w; the last-layer
    class, whose latent is the coefficient vector a: Dot(model_x_to_phi, a) + bias)"""
    x = np.asarray(x, dtype=np.float64)
    lat = np.tile(np.asarray(z, dtype=np.float64), (x.shape[0], 1))
    if spec.kind == O.KIND_LL:
        return np.einsum("bsj,bj->bs", O.model_x_to_phi(spec, ws, x), lat) + ws[-1]
    return O.shapenet_given_w(spec, x, O.model_lr_to_w(spec, ws, lat))


def jac_fd(spec, ws, z, x, h=1e-5):
    """du/dz [M, so, r] by fourth-order central differences of field(): truncation h^4 u^(5) / 30, rounding ~1e-16 / h (the
    deepest SIREN net of the tests varies on a latent scale of 1e-2: h = 1e-5 keeps both below 1e-8 on every test net)"""
    z = np.asarray(z, dtype=np.float64)
    cols = []
    for k in range(z.size):
        e = np.zeros_like(z)
        e[k] = h
        cols.append((-field(spec, ws, z + 2 * e, x) + 8 * field(spec, ws, z + e, x) - 8 * field(spec, ws, z - e, x)
                     + field(spec, ws, z - 2 * e, x)) / (12 * h))
    return np.stack(cols, axis=2)


def _torch_field(spec, ws, lat, x):
    """torch restatement of the field from per-point latents lat [M, r] (reference model.py:253-324, :769-954, :1219-1269 behind the
    bottleneck): written apart from the oracle, differentiated by autograd"""
    import torch
    from tests.torch_ref import _act
    names = _names(spec)
    si, so, n, L, r = spec.si, spec.so, spec.n, spec.L, spec.r
    i_last = names.index("pnet_last_w")
    if spec.kind == O.KIND_LL:
        it = iter(ws[i_last + 2:])
        om = spec.omega_s
        w, b = next(it), next(it)
        h = torch.sin(om * (x @ w) + b)
        for _ in range(L):
            if spec.s_res:
                w, b, w2, b2 = next(it), next(it), next(it), next(it)
                t = torch.sin(om * (h @ w) + b)
                h = 0.5 * (h + torch.sin(om * (t @ w2) + b2))
            else:
                w, b = next(it), next(it)
                h = torch.sin(om * (h @ w) + b)
        w, b = next(it), next(it)
        phi = (h @ w + b).reshape(-1, so, r)
        return torch.einsum("bsj,bj->bs", phi, lat) + next(it)
    po = lat @ ws[i_last] + ws[i_last + 1]
    B = x.shape[0]
    nh = spec.n_hidden_mats
    off = 0
    W1 = po[:, off:off + si * n].reshape(B, si, n); off += si * n
    Wh = []
    for _ in range(nh):
        Wh.append(po[:, off:off + n * n].reshape(B, n, n)); off += n * n
    Wl = po[:, off:off + n * so].reshape(B, n, so); off += n * so
    b1 = po[:, off:off + n]; off += n
    bh = []
    for _ in range(nh):
        bh.append(po[:, off:off + n]); off += n
    bl = po[:, off:]
    ein = lambda a, w: torch.einsum("ai,aij->aj", a, w)
    if spec.kind == O.KIND_NIF:
        f = _act(spec.s_act)
        a = f(ein(x, W1) + b1)
        for i in range(L):
            a = f(ein(a, Wh[i]) + bh[i]) + a
    else:
        om = spec.omega_s
        a = torch.sin(om * ein(x, W1) + b1)
        if spec.s_res:
            for i in range(L):
                t = torch.sin(om * ein(a, Wh[2 * i]) + bh[2 * i])
                a = 0.5 * (a + torch.sin(om * ein(t, Wh[2 * i + 1]) + bh[2 * i + 1]))
        else:
            for i in range(L):
                a = torch.sin(om * ein(a, Wh[i]) + bh[i])
    return ein(a, Wl) + bl


def field_and_jac(spec, ws, z, x):
    """(u [M, so], du/dz [M, so, r]) in float64 by torch autograd: the rows of the tiled latent are independent"""
    import torch
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return np.zeros((0, spec.so)), np.zeros((0, spec.so, spec.r))
    tw = [torch.tensor(np.asarray(w, dtype=np.float64)) for w in ws]
    lat = torch.tensor(np.tile(np.asarray(z, dtype=np.float64), (x.shape[0], 1)), requires_grad=True)
    u = _torch_field(spec, tw, lat, torch.tensor(x))
    rows = []
    for i in range(spec.so):
        g, = torch.autograd.grad(u[:, i].sum(), lat, retain_graph=True)
        rows.append(g)
    return u.detach().numpy(), torch.stack(rows, 1).numpy()


def gram(u, J, y, w=None):
    """S [r + 1, r + 1] = sum_m w_m sum_i q q^T, q = [J_m[i, :], u_m[i] - y_m[i]], in float64"""
    M, so, r = J.shape
    q = np.concatenate([J, (u - np.asarray(y, dtype=np.float64))[:, :, None]], axis=2)
    wv = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
    S = np.einsum("m,mia,mib->ab", wv, q, q)
    return 0.5 * (S + S.T)


def normal_eq(spec, ws, latents, xs, ys, wts=None):
    """S [T, r + 1, r + 1] of T snapshots (xs, ys, wts: one array per snapshot; empty snapshots give zeros)"""
    out = np.zeros((len(xs), spec.r + 1, spec.r + 1))
    for t in range(len(xs)):
        if np.shape(xs[t])[0]:
            u, J = field_and_jac(spec, ws, np.asarray(latents[t], dtype=np.float64), xs[t])
            out[t] = gram(u, J, ys[t], None if wts is None else wts[t])
    return out


class RefSamples(object):
    def __init__(self, owner, xs, ys, wts):
        self.owner, self.xs, self.ys, self.wts, self.t = owner, xs, ys, wts, len(xs)

    def free(self):
        self.owner.freed += 1


class RefEngine(object):
    """The engine calls of Model.encode_snapshots on the float64 references above; every call is recorded"""

    def __init__(self, kind, cs, cp, seed=0, ws=None):
        self.ospec = O.Spec(kind, cs, cp)
        if ws is None:
            ws = O.init_weights(self.ospec, np.random.default_rng(seed), dtype=np.float32)
            if kind != O.KIND_NIF:      # (weight_init_factor 0.01 leaves the latent next to no say in the field: a usable scale)
                i = _names(self.ospec).index("pnet_last_w")
                ws[i] = ws[i] * (30.0 if kind == O.KIND_LL else 2.0)
        self.ws = [np.asarray(w, dtype=np.float64) for w in ws]
        self.calls = []
        self.freed = 0

    def p_to_lr(self, p):
        self.calls.append(("p_to_lr", np.shape(p)[0]))
        return O.model_p_to_lr(self.ospec, self.ws, np.asarray(p, dtype=np.float64)).astype(np.float32)

    def snapshot_samples(self, x, y, w=None, counts=None):
        s = self.ospec
        x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
        if counts is None:
            T = y.shape[0]
            xs, ys = [x] * T, [y[t] for t in range(T)]
            wts = None if w is None else [np.asarray(w, dtype=np.float32)[t] for t in range(T)]
        else:
            off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            assert x.shape == (off[-1], s.si) and y.shape == (off[-1], s.so)
            cut = lambda a: [a[off[t]:off[t + 1]] for t in range(len(counts))]
            xs, ys, wts = cut(x), cut(y), None if w is None else cut(np.asarray(w, dtype=np.float32))
        self.calls.append(("samples", [a.shape[0] for a in xs]))
        return RefSamples(self, xs, ys, wts)

    def snapshot_normal_eq(self, latents, samples):
        latents = np.asarray(latents)
        assert latents.dtype == np.float32 and latents.shape == (samples.t, self.ospec.r)
        self.calls.append(("normal_eq", latents.copy()))
        return normal_eq(self.ospec, self.ws, latents, samples.xs, samples.ys, samples.wts)
