/* nif_hip_snapfit.h -- the snapshot-wise training entries of libnif_hip.so: an extension of include/nif_hip.h like
 * include/nif_hip_encode.h (same library, same context, same error codes and conventions).  The other snapshot entries decode, encode
 * or differentiate whole fields without the [T M, pi + si] table; these two take the training step off it for the class whose field is
 * separable, NIFMultiScaleLastLayerParameterized: u_t(x_m) = phi(x_m) . a(p_t) + bias, phi the shared ShapeNet (sees x alone), a the
 * ParameterNet (sees p_t alone).  On T snapshots of one shared mesh of M points the loss and every gradient of the step are sums
 * over (t, m) that factor: the ShapeNet runs, is differentiated and reduced over the M mesh points, the ParameterNet over
 * the T rows of p, and only the head -- one read of y -- is O(T M).  Both entries take one versioned struct; each passes the door of
 * the C-ABI (NIF_ENTER) in its own body, and tests/test_fit_snapshots.py holds this header, the library's exports,
 * nif_amd/_lib.py::SNAPFIT_SIGNATURES and the struct's ctypes mirror equal. */
#ifndef NIF_HIP_SNAPFIT_H
#define NIF_HIP_SNAPFIT_H
#include "nif_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define NIF_SNAPFIT_ABI_VERSION 1

/* The step nif_loss_grad_dev computes on the expanded table [repeat(p, M) | tile(x, T)] with the targets y [T M, so] and the weights
 * sw [T M], from its factors: p [T, pi] the ParameterNet inputs of the snapshots, x [M, si] the shared mesh, y [T, M, so], sw [T, M]
 * or NULL (all 1).  batch_global is nif_loss_grad_dev's B_global (the divisor of the mean); 0 means T M.  The loss is the one of
 * nif_set_loss.  Leaves [grad | loss] in the context's gradient buffer exactly where nif_loss_grad_dev leaves it: nif_grad_read,
 * nif_opt_step_dev, nif_adam_step_dev, nif_grad_transform_dev, nif_metric_accumulate and the weight regularisers' term work
 * unchanged behind it.  T = 0 or M = 0: a zero gradient and a zero loss.  No atomics anywhere: two calls agree bit for bit.
 * NIF_ERR_INVALID ("not built"): the two hypernetwork classes; a mixed policy; an activity or latent-Jacobian regulariser set on the
 * context; so * latent_dim > 64; a wrong abi_version or a non-zero reserved field.  NIF_ERR_STATE inside nif_graph_begin /
 * nif_graph_end. */
typedef struct nif_snapfit_args {
  int32_t abi_version;          /* NIF_SNAPFIT_ABI_VERSION */
  int32_t reserved0;            /* 0 */
  nif_ctx* ctx;
  const float* p;               /* [T, pi] */
  int64_t T;
  const float* x;               /* [M, si] */
  int64_t M;
  const float* y;               /* [T, M, so] */
  const float* sw;              /* [T, M] or NULL */
  int64_t batch_global;         /* 0: T M */
  int64_t reserved[4];          /* 0 */
} nif_snapfit_args;

/* host pointers (p, x, y, sw); returns with [grad | loss] complete on the device (read it with nif_grad_read) */
int nif_snapshot_loss_grad(const nif_snapfit_args* args);
/* device pointers; asynchronous on the context's stream like nif_loss_grad_dev */
int nif_snapshot_loss_grad_dev(const nif_snapfit_args* args);

#ifdef __cplusplus
}
#endif
#endif
