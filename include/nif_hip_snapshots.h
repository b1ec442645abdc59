/* nif_hip_snapshots.h -- the snapshot-wise inference entries of libnif_hip.so: an extension of include/nif_hip.h (same library, same
 * context, same error codes and conventions; include that header first or let this one do it).  Kept in a header of its own because
 * include/nif_hip.h is the list the call-order sweep of the test suite is held equal to export by export; the orders of these two
 * entries (weights set, a deferred optimizer tail, nif_forward around them, a graph capture) are tested by hand in
 * tests/test_gpu_snapshots.py, and tests/test_snapshots.py holds this header, the library's exports and
 * nif_amd/_lib.py::SNAPSHOT_SIGNATURES equal. */
#ifndef NIF_HIP_SNAPSHOTS_H
#define NIF_HIP_SNAPSHOTS_H
#include "nif_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Snapshot-wise model.predict: T snapshots, each ONE ParameterNet input for a whole mesh -- what the reference serves with its
 * three-stage factorisation (README.md:99-117, model.py:956-986), without the [M, po] weight tensor and without a [T M, pi+si] host
 * table.  rows [T, pi] (rows_are_latent = 0) or [T, r] latents as nif_pnet_latent returns them (rows_are_latent = 1: the ParameterNet
 * is skipped; last-layer class: the coefficient vector a).  Meshes: offsets_host = NULL, x [M, si] shared by every snapshot, u [T, M, so];
 * or offsets_host [T+1] (offsets[0] = 0, non-decreasing; snapshot t owns the points offsets[t] .. offsets[t+1]), x [offsets[T], si]
 * concatenated, u [offsets[T], so]; M is ignored then.  u of snapshot t is nif_forward of the rows [p_t | x] -- on nets under a mixed
 * policy or on the legacy k_snet kernels bit for bit (the table is expanded on the device and the point-wise kernels run); else
 * the ParameterNet runs once per snapshot, the hypernetwork classes run ONE set of hidden products per layer on the snapshot's
 * combined matrices sum_k latent_k M^(k) (formed in fp32 from theta, packed per call) instead of r + 1 per point, and the last-layer
 * class on a shared mesh runs the ShapeNet x -> phi once per call (k_snap.hip).  offsets_host is host memory in both forms and consumed before the call returns; _dev is otherwise asynchronous like
 * nif_forward_dev.  Reads theta only; rebuilt from it on every call.  NIF_ERR_STATE inside nif_graph_begin / nif_graph_end. */
int nif_forward_snapshots(nif_ctx* ctx, const float* rows_host, int32_t rows_are_latent, int64_t T, const float* x_host,
                          const int64_t* offsets_host, int64_t M, float* u_host);
int nif_forward_snapshots_dev(nif_ctx* ctx, const float* rows_dev, int32_t rows_are_latent, int64_t T, const float* x_dev,
                              const int64_t* offsets_host, int64_t M, float* u_dev);

#ifdef __cplusplus
}
#endif
#endif
