/* nif_hip_encode.h -- the encoding entries of libnif_hip.so: an extension of include/nif_hip.h like include/nif_hip_snapshots.h (same
 * library, same context, same error codes and conventions).  nif_forward_snapshots decodes fields from one latent per mesh; these two
 * go the other way as far as the device is needed for it: ONE pass over the samples of T snapshots gives every snapshot's Gauss-Newton
 * normal equations in the latent, and the r x r solves and the Levenberg-Marquardt logic around them stay on the host
 * (nif_amd/encode.py).  Both entries take one versioned struct instead of a context-first parameter list; each passes
 * the door of the C-ABI (NIF_ENTER) in its own body, and tests/test_encode.py holds this header, the library's exports,
 * nif_amd/_lib.py::ENCODE_SIGNATURES and the struct's ctypes mirror equal. */
#ifndef NIF_HIP_ENCODE_H
#define NIF_HIP_ENCODE_H
#include "nif_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define NIF_ENCODE_ABI_VERSION 1

/* Snapshot t has the latent z_t = latents[t] (as nif_pnet_latent returns it; last-layer class: the coefficient vector a), the points
 * x_m, the targets y_m [so] and the weights w_m >= 0 (w NULL: all 1).  With e_m = u(z_t; x_m) - y_m, J_m = du/dz (z_t; x_m) [so, r]
 * and the augmented rows q = [J_m[i, :], e_m[i]] in R^(r+1):
 *     S_out[t] = sum_m w_m sum_i q q^T          float64 [r+1, r+1], full symmetric,
 * i.e. A_t = sum J^T W J in the leading r x r block, g_t = sum J^T W e in the last column (and row) and c_t = sum w |e|^2 in the
 * corner.  An empty snapshot gives zeros.  Meshes as in nif_forward_snapshots: offsets_host = NULL, x [M, si] shared by every
 * snapshot, y [T, M, so], w [T, M]; or offsets_host [T+1] (offsets[0] = 0, non-decreasing), x [offsets[T], si], y [offsets[T], so],
 * w [offsets[T]] concatenated, M ignored.  Products in fp32, sums of at most 32 points in fp32, float64 across them, in an order
 * that depends on the snapshot's own points alone: two calls agree bit for bit, and so do a snapshot's results at any position in
 * the call and under any chunk budget (nif_set_option "snapshot_image_bytes").  Reads theta only.
 * NIF_ERR_INVALID: a mixed policy (not built); a hypernetwork net the JacobianLayer kernels do not take; latent_dim > 64; a wrong
 * abi_version or a non-zero reserved field.  NIF_ERR_STATE inside nif_graph_begin / nif_graph_end. */
typedef struct nif_encode_args {
  int32_t abi_version;          /* NIF_ENCODE_ABI_VERSION */
  int32_t reserved0;            /* 0 */
  nif_ctx* ctx;
  const float* latents;         /* [T, r] */
  int64_t T;
  const float* x;
  const int64_t* offsets_host;  /* host memory in both entries, consumed before the call returns */
  int64_t M;
  const float* y;
  const float* w;               /* or NULL */
  double* S_out;                /* [T, r+1, r+1] */
  int64_t reserved[4];          /* 0 */
} nif_encode_args;

/* host pointers (latents, x, y, w, S_out); returns with S_out filled */
int nif_snapshot_normal_eq(const nif_encode_args* args);
/* device pointers; asynchronous on the context's stream like nif_forward_dev once offsets_host is consumed */
int nif_snapshot_normal_eq_dev(const nif_encode_args* args);

#ifdef __cplusplus
}
#endif
#endif
