/* nif_hip_snapderiv.h -- the snapshot-wise derivative entries of libnif_hip.so: an extension of include/nif_hip.h like
 * include/nif_hip_snapshots.h and include/nif_hip_encode.h (same library, same context, same error codes and conventions).
 * nif_forward_snapshots decodes u for T snapshots, each ONE ParameterNet input or latent for a whole mesh; these two give du/dx and
 * d2u/dx2 of the same fields in the coordinates: what HessianLayer returns on the expanded table of rows [p_t | x],
 * without that table.  Both entries take one versioned struct instead of a context-first parameter list; each passes the door of
 * the C-ABI (NIF_ENTER) in its own body, and tests/test_snapshot_derivatives.py holds this header, the library's exports,
 * nif_amd/_lib.py::SNAPDERIV_SIGNATURES and the struct's ctypes mirror equal. */
#ifndef NIF_HIP_SNAPDERIV_H
#define NIF_HIP_SNAPDERIV_H
#include "nif_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define NIF_SNAPDERIV_ABI_VERSION 1

/* rows [T, pi] (rows_are_latent = 0) or [T, r] latents as nif_pnet_latent returns them (rows_are_latent = 1: the ParameterNet is
 * skipped; last-layer class: the coefficient vector a).  Meshes as in nif_forward_snapshots: offsets_host = NULL, x [M, si] shared by
 * every snapshot, outputs [T, M, ...]; or offsets_host [T+1] (offsets[0] = 0, non-decreasing), x [offsets[T], si] concatenated,
 * outputs [offsets[T], ...], M ignored.  x_idx [nx]: DISTINCT coordinate indices 0 <= j < si (JacobianLayer's x_index minus pi_dim;
 * at most 16); y_idx [ny <= 16]: outputs, any order, repeats allowed.  Both index arrays are host memory in both entries.
 *     u      [n, so]              every output, as HessianLayer returns y
 *     dudx   [n, ny, nx]
 *     d2udx2 [n, ny, nx, nx]      order = 2 only (order = 1: ignored, may be NULL); bit-symmetric in its last two axes
 * Hypernetwork classes under the float32 policy on the shapes the JacobianLayer kernels take: the ParameterNet runs once per
 * snapshot, the combined matrices b + sum_k latent_k M^(k) are formed in fp32 from theta and packed per call, and ONE launch per
 * chunk of snapshots and seed group (order 1: three coordinates; order 2: one coordinate pair j <= k) runs the tangent kernel as an
 * r = 0 net -- one plane product per hidden layer and stream instead of r + 1.  Last-layer class: the ShapeNet tangents run once per
 * mesh on a shared mesh and are contracted with all T coefficient vectors; per-snapshot meshes take the point-wise kernels on
 * coefficient tiles built on the device.  Mixed policies and the nets on the legacy k_snet kernels, with rows_are_latent = 0: the
 * table is expanded on the device and the point-wise derivative kernels run, bit for bit nif_hessian_dev's result.
 * A snapshot's results do not depend on its position in the call nor on the chunk budget (nif_set_option "snapshot_image_bytes").
 * Reads theta only.  NIF_ERR_INVALID: rows_are_latent under a mixed policy (not built); what nif_hessian refuses (a ShapeNet wider
 * than 128 units, a shape whose planes do not fit the LDS, more than 16 coordinates); an index out of range or a repeated x_idx; an
 * order other than 1 or 2; a wrong abi_version or a non-zero reserved field.  NIF_ERR_STATE inside nif_graph_begin / nif_graph_end. */
typedef struct nif_snapderiv_args {
  int32_t abi_version;          /* NIF_SNAPDERIV_ABI_VERSION */
  int32_t order;                /* 1 or 2 */
  nif_ctx* ctx;
  const float* rows;            /* [T, pi] or [T, r] */
  int32_t rows_are_latent;
  int32_t reserved0;            /* 0 */
  int64_t T;
  const float* x;
  const int64_t* offsets_host;  /* host memory in both entries, consumed before the call returns */
  int64_t M;
  const int32_t* y_idx;         /* host memory in both entries */
  int32_t ny;
  int32_t reserved1;            /* 0 */
  const int32_t* x_idx;         /* host memory in both entries */
  int32_t nx;
  int32_t reserved2;            /* 0 */
  float* u;
  float* dudx;
  float* d2udx2;                /* order 2 */
  int64_t reserved[4];          /* 0 */
} nif_snapderiv_args;

/* host pointers (rows, x, u, dudx, d2udx2); returns with the outputs filled */
int nif_snapshot_derivatives(const nif_snapderiv_args* args);
/* device pointers; asynchronous on the context's stream like nif_hessian_dev once offsets_host and the index arrays are consumed */
int nif_snapshot_derivatives_dev(const nif_snapderiv_args* args);

#ifdef __cplusplus
}
#endif
#endif
