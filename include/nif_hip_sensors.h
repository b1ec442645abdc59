/* nif_hip_sensors.h -- sensor placement on the basis of the last-layer class: an extension of include/nif_hip.h like
 * include/nif_hip_encode.h (same library, same context, same error codes and conventions).  For
 * NIFMultiScaleLastLayerParameterized every field is u_t(x) = phi(x) . a(p_t) + bias: a linear subspace with the learned basis phi.
 * nif_snapshot_normal_eq* (encode) recovers a from readings at sensor points; these two entries say where the sensors go, so that
 * the recovery is well conditioned: the pivots of a column-pivoted QR of Phi^T (QDEIM), computed greedily on the device (DESIGN
 * 2.12).  Both entries take one versioned struct; each passes the door of the C-ABI (NIF_ENTER) in its own body, and
 * tests/test_select_sensors.py holds this header, the library's exports, nif_amd/_lib.py::SENSORS_SIGNATURES and the struct's ctypes
 * mirror equal. */
#ifndef NIF_HIP_SENSORS_H
#define NIF_HIP_SENSORS_H
#include "nif_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define NIF_SENSORS_ABI_VERSION 1

/* The candidates are the N = M so rows of Phi = model_x_to_phi(x) [M, so, r] reshaped [M so, r] (what nif_x_to_phi computes under
 * the context's policy): row m so + s is output component s at mesh point m, and a sensor is such a (point, component) pair.  For
 * k = 0 .. K - 1:
 *     j_k = argmax over the eligible rows of |res_row|^2   (ties: the lowest row; eligible: mask[m] != 0 and not yet chosen)
 *     d_k = |res_row(j_k)|,  q_k = res_row(j_k) / d_k
 *     every row: res_row -= (res_row . q_k) q_k            (row j_k becomes exactly 0)
 * pivots_out[k] = j_k, diag_out[k] = d_k (the diagonal of R; non-increasing up to rounding).  When no eligible row has a positive
 * norm -- fewer candidates than K, or the rank of Phi exhausted -- that step and every later one return pivot -1 and d = 0.  A row's
 * arithmetic depends on that row and q_k alone and there are no atomics: two calls agree bit for bit, and a permuted mesh gives the
 * permuted pivots with the same d (as long as no exact tie is broken).  Reads theta only: the gradient, the optimizer state and
 * the loss metric stay as they are.
 * NIF_ERR_INVALID: the two hypernetwork classes (their basis depends on the latent: selection on du/dz at a given latent is not
 * built); K < 1 or K > latent_dim (the rows live in R^r: more sensors than r is a different, oversampling algorithm);
 * latent_dim > 64; M < 1; a null x or output; a wrong abi_version or a non-zero reserved field.  NIF_ERR_STATE inside
 * nif_graph_begin / nif_graph_end.  A mixed policy is allowed. */
typedef struct nif_sensors_args {
  int32_t abi_version;          /* NIF_SENSORS_ABI_VERSION */
  int32_t reserved0;            /* 0 */
  nif_ctx* ctx;
  const float* x;               /* [M, si] */
  int64_t M;
  const uint8_t* mask;          /* [M]: 0 = no sensor can stand at this point; NULL: every point is a candidate */
  int64_t K;
  int64_t* pivots_out;          /* [K] row indices m so + s, or -1 */
  float* diag_out;              /* [K] */
  int64_t reserved[4];          /* 0 */
} nif_sensors_args;

/* host pointers (x, mask, pivots_out, diag_out); returns with the outputs filled */
int nif_select_sensors(const nif_sensors_args* args);
/* device pointers; asynchronous on the context's stream */
int nif_select_sensors_dev(const nif_sensors_args* args);

#ifdef __cplusplus
}
#endif
#endif
