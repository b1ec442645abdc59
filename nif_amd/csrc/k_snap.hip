// k_snap.hip -- snapshot-wise inference (include/nif_hip_snapshots.h): T snapshots, each one ParameterNet input
// (or one latent vector) for a whole mesh of points (reference README.md:99-117, model.py:956-986).
//   k_snet4<.., SNAP>: the hypernetwork classes.  Every point of a snapshot sees the same combined matrices W_t = sum_k zt_k(t) M^(k), so
//                  the (r + 1) plane products per hidden layer of the point-wise kernel are one: nif_api forms the slot vector w_t of
//                  every snapshot in fp32 from theta (launch_latent_to_w), packs its hidden matrices in the forward kernel's own chunk
//                  format (launch_pack16b_batch: half pairs + a power of two per (snapshot, matrix) for SIREN nets, bf16 splits for
//                  class NIF), and ONE launch of the r = 0 forward runs all snapshots (blockIdx.y = snapshot, k_snet4_dev.h).
//   k_snap_expand: the nets off that path.  The per-point operands of the unchanged forward kernels, built on the device from the T rows -- the [p_t | x]
//                  table and / or the latent tiles Z [tile][r][32] with every point of snapshot t carrying latent t.  No host table.
//   k_phi_dot:     last-layer class on a shared mesh: u[t][m][s] = sum_c phi[m][s][c] a[t][c] + bias[s], phi of a 32-point tile held
//                  in LDS and reused over all T snapshots (one ShapeNet pass for the whole call).
#include "k_snet4_dev.h"

// the snapshot of point i: shared mesh i / M; ragged the last t with offsets[t] <= i (empty snapshots own no point)
__device__ __forceinline__ long snap_of(const SnapArgs& A, long i) {
  if (!A.offsets) return i / A.M;
  long lo = 0, hi = A.T;       // offsets[lo] <= i < offsets[hi]
  while (hi - lo > 1) {
    const long mid = (lo + hi) >> 1;
    if (A.offsets[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// one thread per point of the padded tiles; padding points repeat the last real point's latent (as k_rows_to_tiles does)
__global__ __launch_bounds__(256) void k_snap_expand(SnapArgs A) {
  const long pt = (long)blockIdx.x * 256 + threadIdx.x;
  const long ntiles = (A.n + 31) / 32;
  if (pt >= ntiles * 32) return;
  const bool valid = pt < A.n;
  const long i = valid ? pt : A.n - 1;
  const long t = snap_of(A, i);
  if (A.table && valid) {
    const int ncol = A.pi + A.si;
    float* row = A.table + pt * ncol;
    for (int d = 0; d < A.pi; ++d) row[d] = A.p ? A.p[t * A.pi + d] : 0.f;
    const float* xr = A.x + (A.offsets ? i : i - t * A.M) * A.si;
    for (int d = 0; d < A.si; ++d) row[A.pi + d] = xr[d];
  }
  if (A.Z) {
    float* z = A.Z + (pt >> 5) * (long)A.r * 32 + (pt & 31);
    for (int k = 0; k < A.r; ++k) z[k * 32] = A.lat[t * A.r + k];
  }
}
void launch_snap_expand(const SnapArgs& a, hipStream_t st) {
  const long ntiles = (a.n + 31) / 32;
  hipLaunchKernelGGL(k_snap_expand, dim3((unsigned)((ntiles * 32 + 255) / 256)), dim3(256), 0, st, a);
}

// One workgroup per 32-point tile of the mesh: the tile's phi rows [so * r][32] go to LDS once, then the 8 point groups of the
// workgroup walk the snapshots t = g, g + 8, ...  The sum runs in k_ll_out's order (bias first, then c = 0 .. r - 1 by fma), so a
// snapshot's values are the ones the point-wise epilogue gives for the same phi and a.
__global__ __launch_bounds__(256) void k_phi_dot(const float* __restrict__ PHI, const float* __restrict__ a, const float* __restrict__ bias,
                                                 long T, long M, int r, int so, float* __restrict__ u) {
  extern __shared__ float phi[];
  const long tile = blockIdx.x;
  const int sop = so * r;
  for (int e = threadIdx.x; e < sop * 32; e += 256) phi[e] = PHI[tile * (long)sop * 32 + e];
  __syncthreads();
  const int p = threadIdx.x & 31;
  const long m = tile * 32 + p;
  if (m >= M) return;
  for (long t = threadIdx.x >> 5; t < T; t += 8) {
    const float* at = a + t * r;
    float* ut = u + (t * M + m) * so;
    for (int s = 0; s < so; ++s) {
      float acc = bias[s];
      for (int c = 0; c < r; ++c) acc = fmaf(phi[(s * r + c) * 32 + p], at[c], acc);
      ut[s] = acc;
    }
  }
}
bool phi_dot_supported(int r, int so) { return (long)r * so * 32 * sizeof(float) <= 48 * 1024; }
void launch_phi_dot(const float* PHI, const float* a, const float* bias, long T, long M, int r, int so, float* u, hipStream_t st) {
  const long ntiles = (M + 31) / 32;
  hipLaunchKernelGGL(k_phi_dot, dim3((unsigned)ntiles), dim3(256), sizeof(float) * (size_t)r * so * 32, st, PHI, a, bias, T, M, r, so, u);
}

// ---- the combined-net forward: launch_snet4's grid and instantiation choice for the SNAP forms -------------------------------------
int launch_snet4_snap(const SNetArgs& a, long T, long Mmax, hipStream_t st) {
  const int NBL = snet3_nbl(a.n);
  if (a.r != 0 || a.ll || a.prec != 0 || T < 1 || T > 65535 || !snet4_supported(a)) return -1;
  const long ngroups = (2 * ((Mmax + 31) / 32) + 3) / 4;
  const long cap = NBL <= 4 ? 256 * NIF_S4_OCC : 256 * NIF_S4_OCC_WIDE;      // workgroups that fill the device, shared by the T snapshots
  long per = (cap + T - 1) / T;
  if (per > ngroups) per = ngroups;
  if (per < 1) per = 1;
  dim3 grid((unsigned)per, (unsigned)T), block(256);
  const size_t shm = snet4_shmem(a, NBL);
#define S4L(NBL_, ACT_, MODE_, PR_)                                                                                \
  {                                                                                                              \
    if (shm > 48 * 1024)                                                                                         \
      (void)hipFuncSetAttribute((const void*)k_snet4<NBL_, false, ACT_, MODE_, false, false, PR_, true>,         \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);                           \
    hipLaunchKernelGGL((k_snet4<NBL_, false, ACT_, MODE_, false, false, PR_, true>), grid, block, shm, st, a);   \
  }
// class NIF: the bf16 splits (its activations are not bounded); SIREN nets, plain or resblock: the half pairs
#define S4(NBL_)                                                  \
  if (a.nif_skip) S4L(NBL_, -1, 2, 0)                             \
  else if (!a.wscale) return -1;                                  \
  else if (a.res) S4L(NBL_, ACT_SINE, 1, 3)                       \
  else S4L(NBL_, ACT_SINE, 0, 3)
  switch (NBL) {
    case 2: S4(2) break;
    case 4: S4(4) break;
    case 6: S4(6) break;
    default: S4(8) break;
  }
#undef S4
#undef S4L
  return (int)per;
}
