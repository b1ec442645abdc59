/* nif_hip_snapparam.h -- the snapshot-wise parameter-derivative entries of libnif_hip.so: an extension of include/nif_hip.h like
 * include/nif_hip_snapshots.h, include/nif_hip_encode.h and include/nif_hip_snapderiv.h (same library, same context, same error
 * codes and conventions).  nif_snapshot_derivatives gives du/dx of the decoded fields; these two give the derivative in the other
 * half of the input vector, du/dp: what JacobianLayer returns for parameter columns on the expanded table of rows
 * [p_t | x], without that table -- or, given latents, the derivative of the field along directions in latent space.  Both entries
 * take one versioned struct instead of a context-first parameter list; each passes the door of the C-ABI (NIF_ENTER) in its own
 * body, and tests/test_snapshot_param_derivatives.py holds this header, the library's exports,
 * nif_amd/_lib.py::SNAPPARAM_SIGNATURES and the struct's ctypes mirror equal. */
#ifndef NIF_HIP_SNAPPARAM_H
#define NIF_HIP_SNAPPARAM_H
#include "nif_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define NIF_SNAPPARAM_ABI_VERSION 1

/* rows_are_latent = 0: rows [T, pi], p_idx [np]: DISTINCT ParameterNet input columns 0 <= c < pi, 1 <= np <= 16; drows NULL, nd 0.
 *     dudp[.., i, c] = du_{y_idx[i]} / dp_{p_idx[c]}                                  (the call's nd below is np)
 * rows_are_latent = 1: rows [T, r] latents as nif_pnet_latent returns them (last-layer class: the coefficient vector a) and
 * drows [T, nd, r], 1 <= nd <= 16 directions per snapshot; p_idx NULL, np 0.
 *     dudp[.., i, d] = sum_k du_{y_idx[i]} / dz_k (z_t; x) drows[t, d, k]
 * Meshes as in nif_forward_snapshots: offsets_host = NULL, x [M, si] shared by every snapshot, outputs [T, M, ...]; or offsets_host
 * [T+1] (offsets[0] = 0, non-decreasing), x [offsets[T], si] concatenated, outputs [offsets[T], ...], M ignored.  y_idx [ny <= 16]:
 * outputs, any order, repeats allowed.  The index arrays are host memory in both entries.
 *     u      [n, so]              every output
 *     dudp   [n, ny, nd]
 * Hypernetwork classes under the float32 policy on the shapes the JacobianLayer kernels take: the ParameterNet and its input
 * tangents run once per snapshot; the combined matrices w_t = b + sum_k z_t,k M^(k) and their tangents sum_k delta_t,d,k M^(k) are
 * formed in fp32 from theta and packed per call, and one launch per chunk of snapshots and group of three directions runs the
 * weight-tangent form of the tangent kernel as an r = 0 net: 1 + 2 g plane products per hidden layer for g directions.
 * Last-layer class (ShapeNets of up to 512 units): phi once per shared mesh, contracted with the coefficient vectors and their
 * tangents; per-snapshot meshes take the point-wise epilogues on coefficient tiles built on the device.  Mixed policies and the nets
 * on the legacy k_snet kernels, with rows_are_latent = 0: the table is expanded on the device and JacobianLayer's kernels run, bit
 * for bit nif_jacobian's result.
 * A snapshot's results do not depend on its position in the call nor on the chunk budget (nif_set_option "snapshot_image_bytes").
 * Reads theta only.  NIF_ERR_INVALID: rows_are_latent without drows, or drows / nd without it; p_idx / np with latents; nd or np
 * outside 1 .. 16; an index out of range or a repeated p_idx; rows_are_latent under a mixed policy (not built); what nif_jacobian
 * refuses (a hypernetwork ShapeNet wider than 128 units, a shape whose planes do not fit the LDS; under a mixed policy also the
 * last-layer nets wider than 128 units); a wrong abi_version or a non-zero reserved field.  NIF_ERR_STATE inside nif_graph_begin /
 * nif_graph_end. */
typedef struct nif_snapparam_args {
  int32_t abi_version;          /* NIF_SNAPPARAM_ABI_VERSION */
  int32_t rows_are_latent;
  nif_ctx* ctx;
  const float* rows;            /* [T, pi] or [T, r] */
  const float* drows;           /* [T, nd, r], rows_are_latent only */
  int32_t nd;
  int32_t np;
  const int32_t* p_idx;         /* host memory in both entries; rows [T, pi] only */
  int64_t T;
  const float* x;
  const int64_t* offsets_host;  /* host memory in both entries, consumed before the call returns */
  int64_t M;
  const int32_t* y_idx;         /* host memory in both entries */
  int32_t ny;
  int32_t reserved0;            /* 0 */
  float* u;
  float* dudp;
  int64_t reserved[4];          /* 0 */
} nif_snapparam_args;

/* host pointers (rows, drows, x, u, dudp); returns with the outputs filled */
int nif_snapshot_param_derivatives(const nif_snapparam_args* args);
/* device pointers; asynchronous on the context's stream once offsets_host and the index arrays are consumed */
int nif_snapshot_param_derivatives_dev(const nif_snapparam_args* args);

#ifdef __cplusplus
}
#endif
#endif
