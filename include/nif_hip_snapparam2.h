/* nif_hip_snapparam2.h -- the second-order snapshot-wise parameter-derivative entries of libnif_hip.so: an extension of
 * include/nif_hip.h like include/nif_hip_snapparam.h (same library, same context, same error codes and conventions), which it leaves
 * as it is.  nif_snapshot_param_derivatives gives du/dp of the decoded fields; these two add the second order in the parameters or
 * along latent directions, d2u/dp2, and the mixed block d2u/dp dx: the blocks of what HessianLayer returns for
 * parameter and coordinate columns on the expanded table of rows [p_t | x], without that table.  Both entries take one versioned
 * struct; each passes the door of the C-ABI (NIF_ENTER) in its own body, and tests/test_snapshot_param_second_derivatives.py holds
 * this header, the library's exports, nif_amd/_lib.py::SNAPPARAM2_SIGNATURES and the struct's ctypes mirror equal. */
#ifndef NIF_HIP_SNAPPARAM2_H
#define NIF_HIP_SNAPPARAM2_H
#include "nif_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define NIF_SNAPPARAM2_ABI_VERSION 1

/* rows, drows, nd, np, p_idx, T, x, offsets_host, M, y_idx, ny: as in nif_snapparam_args, with 1 <= nd <= 8 (np likewise): 36 pairs.
 * rows_are_latent = 0: rows [T, pi], p_idx [np]; ddrows NULL.  With delta_c = dz/dp_{p_idx[c]} and dd_ab = d2z/dp_a dp_b this is
 *     the rows_are_latent = 1 formula below; dudp, d2udp2 and d2udpdx are the blocks J[:, :, :np], H[:, :, :np, :np] and
 *     H[:, :, :np, np:] of HessianLayer on the columns p_idx + [pi + j for j in x_idx] of the expanded table.
 * rows_are_latent = 1: rows [T, r], drows [T, nd, r], ddrows [T, nd, nd, r] or NULL (zeros), symmetric in its two direction axes (the
 *     entries read ddrows[t, a, b] for a <= b only):
 *     d2udp2 [.., i, a, b] = sum_kl d2u_i/dz_k dz_l drows[t,a,k] drows[t,b,l] + sum_k du_i/dz_k ddrows[t,a,b,k]
 *     d2udpdx[.., i, a, j] = sum_k d2u_i/dz_k dx_{x_idx[j]} drows[t,a,k]
 *     (last-layer class: the latent is the coefficient vector a, so the first term of d2udp2 vanishes)
 * x_idx [nxc]: DISTINCT coordinate indices 0 <= j < si, host memory; nxc = 0 (x_idx NULL): no coordinate columns, dudx and d2udpdx
 * NULL.  They are NULL exactly when nxc is 0.
 *     u       [n, so]              every output            (bit for bit nif_snapshot_param_derivatives')
 *     dudp    [n, ny, nd]                                  (bit for bit nif_snapshot_param_derivatives')
 *     d2udp2  [n, ny, nd, nd]      [.., a, b] and [.., b, a] are one value written twice
 *     dudx    [n, ny, nxc]                                 (bit for bit nif_snapshot_derivatives' at order 1)
 *     d2udpdx [n, ny, nd, nxc]
 * Hypernetwork classes under the float32 policy on the shapes nif_snapshot_param_derivatives runs its weight-tangent kernel on: per
 * chunk of snapshots the combined slot vector w_t, one tangent slot vector per direction and one per pair with a second direction,
 * their planes packed once, and one launch of the second-order weight-tangent kernel per pair a <= b and per (direction, coordinate):
 * 9 plane products per hidden layer for a general pair, 6 for a diagonal or a mixed one (one less without a second direction).
 * Last-layer class under the float32 policy: d2udp2 = phi . a''_ab (a'' = d2z/dp2 last_w, or ddrows itself) and d2udpdx = phi'_j . a'_a;
 * on a shared mesh phi once per call and phi'_j once per coordinate, each contracted with every coefficient row; per-snapshot meshes
 * take the point-wise epilogue on coefficient tiles built on the device.  ShapeNets of 129 .. 512 units run when nxc is 0 (phi alone).
 * Everything else with rows_are_latent = 0 (mixed policies, the nets on the legacy k_snet kernels): the table is expanded on the device
 * and HessianLayer's kernels run, bit for bit nif_hessian's blocks.  A snapshot's results do not depend on its position in the call
 * nor on the chunk budget.
 * Reads theta only.  NIF_ERR_INVALID: what nif_snapshot_param_derivatives refuses, with nd or np outside 1 .. 8; ddrows without
 * latent rows; x_idx out of range or repeated, nxc < 0 or > si, dudx / d2udpdx set without coordinate columns or missing with them;
 * coordinate columns on a ShapeNet wider than 128 units; rows_are_latent under a mixed policy and on the nets on the legacy kernels
 * (not built); what nif_hessian refuses; a wrong abi_version or a non-zero reserved field.  NIF_ERR_STATE inside nif_graph_begin /
 * nif_graph_end. */
typedef struct nif_snapparam2_args {
  int32_t abi_version;          /* NIF_SNAPPARAM2_ABI_VERSION */
  int32_t rows_are_latent;
  nif_ctx* ctx;
  const float* rows;            /* [T, pi] or [T, r] */
  const float* drows;           /* [T, nd, r], rows_are_latent only */
  const float* ddrows;          /* [T, nd, nd, r], rows_are_latent only, may be NULL */
  int32_t nd;
  int32_t np;
  const int32_t* p_idx;         /* host memory in both entries; rows [T, pi] only */
  int64_t T;
  const float* x;
  const int64_t* offsets_host;  /* host memory in both entries, consumed before the call returns */
  int64_t M;
  const int32_t* y_idx;         /* host memory in both entries */
  int32_t ny;
  int32_t nxc;
  const int32_t* x_idx;         /* host memory in both entries, may be NULL (nxc 0) */
  float* u;
  float* dudp;
  float* d2udp2;
  float* dudx;
  float* d2udpdx;
  int64_t reserved[4];          /* 0 */
} nif_snapparam2_args;

/* host pointers (rows, drows, ddrows, x and the outputs); returns with the outputs filled */
int nif_snapshot_param_second_derivatives(const nif_snapparam2_args* args);
/* device pointers; asynchronous on the context's stream once offsets_host and the index arrays are consumed */
int nif_snapshot_param_second_derivatives_dev(const nif_snapparam2_args* args);

#ifdef __cplusplus
}
#endif
#endif
