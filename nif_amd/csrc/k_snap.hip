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
//   k_phi_dot_d2:  the same with the ShapeNet's first- and second-order tangents: u, du/dx, d2u/dx2 of nif_snapshot_derivatives* (whose
//                  hypernetwork route is k_jac<.., SNAP>, k_jac_snap.hip); k_jac_gather takes the rows y_idx of that route's order 1.
//   k_dlatent_to_w, k_dir_rows, k_snapparam_gather: the small kernels of nif_snapshot_param_derivatives*  -- the tangent slot
//                  vectors of a combined net along latent directions (the bias-free companion of k_latent_to_w; the route's tangent
//                  kernel is k_jac_wt, k_jac_wtan.hip), the directions as direction-major rows, and the last-layer route's gather.
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

// ---- snapshot-wise derivatives (include/nif_hip_snapderiv.h) ------------------------------------------------------------
// order 1 on the combined path: rows y_idx of k_jac<.., SNAP>'s [n][so][nx] -> [n][ny][nx] (order 2 gathers with k_hess_gather)
__global__ __launch_bounds__(256) void k_jac_gather(const float* __restrict__ fj, long n, int so, int nx, HessIdx I, float* __restrict__ dydx) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;      // (point, i)
  if (e >= n * I.ny) return;
  const long a = e / I.ny; const int i = (int)(e - a * I.ny);
  const long src = a * so + I.y_idx[i];
  for (int j = 0; j < nx; ++j) dydx[e * nx + j] = fj[src * nx + j];
}
void launch_jac_gather(const float* fj, long n, int so, int nx, const HessIdx& I, float* dydx, hipStream_t st) {
  hipLaunchKernelGGL(k_jac_gather, dim3((unsigned)((n * I.ny + 255) / 256)), dim3(256), 0, st, fj, n, so, nx, I, dydx);
}

// Last-layer class on a shared mesh: k_phi_dot with the ShapeNet's tangents.  One workgroup per 32-point tile of the mesh: the tile's
// rows [phi | phi' | phi''] of the second-order tangent kernel (point-major, as hessian_core leaves them: f0 [M][so r], fj [M][so r][nx],
// fh [M][so r][nx][nx]; fh null: order 1) go to LDS once, one row per point at an odd stride, then the 8 point groups of the workgroup
// walk the snapshots t = g, g + 8, ...  Every sum runs in k_ll_hess' order (u: bias first; then c = 0 .. r - 1 by fma), so a
// snapshot's values are the ones the point-wise epilogue gives for the same tangents and coefficients.
__device__ __host__ inline int phi_dot_d2_stride(int r, int so, int nx, bool order2) { return (so * r * (1 + nx + (order2 ? nx * nx : 0))) | 1; }
__global__ __launch_bounds__(256) void k_phi_dot_d2(const float* __restrict__ f0, const float* __restrict__ fj, const float* __restrict__ fh,
                                                    const float* __restrict__ a, const float* __restrict__ bias, long T, long M, int r, int so,
                                                    int nx, HessIdx I, float* __restrict__ u, float* __restrict__ dudx, float* __restrict__ d2) {
  extern __shared__ float rows[];
  const long m0 = (long)blockIdx.x * 32;
  const int sop = so * r, e1 = sop * nx, e2 = fh ? e1 * nx : 0;
  const int stride = phi_dot_d2_stride(r, so, nx, fh != nullptr);
  const int np = M - m0 < 32 ? (int)(M - m0) : 32;
  for (int idx = threadIdx.x; idx < np * sop; idx += 256) { const int p = idx / sop; rows[p * stride + (idx - p * sop)] = f0[m0 * sop + idx]; }
  for (int idx = threadIdx.x; idx < np * e1; idx += 256) { const int p = idx / e1; rows[p * stride + sop + (idx - p * e1)] = fj[m0 * e1 + idx]; }
  for (int idx = threadIdx.x; idx < np * e2; idx += 256) { const int p = idx / e2; rows[p * stride + sop + e1 + (idx - p * e2)] = fh[m0 * e2 + idx]; }
  __syncthreads();
  const int p = threadIdx.x & 31;
  if (p >= np) return;
  const float* g0 = rows + p * stride;
  const float* gj = g0 + sop;
  const float* gh = gj + e1;
  const int ny = I.ny;
  for (long t = threadIdx.x >> 5; t < T; t += 8) {
    const float* at = a + t * r;
    const long pt = t * M + m0 + p;
    for (int o = 0; o < so; ++o) {
      float acc = bias[o];
      for (int c = 0; c < r; ++c) acc = fmaf(g0[o * r + c], at[c], acc);
      u[pt * so + o] = acc;
    }
    for (int i = 0; i < ny; ++i) {
      const int src = I.y_idx[i] * r;
      float* dy = dudx + (pt * ny + i) * nx;
      for (int j = 0; j < nx; ++j) {
        float t1 = 0.f;
        for (int c = 0; c < r; ++c) t1 = fmaf(gj[(src + c) * nx + j], at[c], t1);
        dy[j] = t1;
        if (fh) {
          float* h = d2 + ((pt * ny + i) * nx + j) * nx;
          for (int k = 0; k < nx; ++k) {
            float t2 = 0.f;
            for (int c = 0; c < r; ++c) t2 = fmaf(gh[((src + c) * nx + j) * nx + k], at[c], t2);
            h[k] = t2;
          }
        }
      }
    }
  }
}
bool phi_dot_d2_supported(int r, int so, int nx, bool order2) { return (long)phi_dot_d2_stride(r, so, nx, order2) * 32 * sizeof(float) <= 64 * 1024; }
void launch_phi_dot_d2(const float* f0, const float* fj, const float* fh, const float* a, const float* bias, long T, long M, int r,
                       int so, int nx, const HessIdx& I, float* u, float* dudx, float* d2, hipStream_t st) {
  const size_t shm = sizeof(float) * 32 * (size_t)phi_dot_d2_stride(r, so, nx, fh != nullptr);
  if (shm > 48 * 1024) (void)hipFuncSetAttribute((const void*)k_phi_dot_d2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  hipLaunchKernelGGL(k_phi_dot_d2, dim3((unsigned)((M + 31) / 32)), dim3(256), shm, st, f0, fj, fh, a, bias, T, M, r, so, nx, I, u, dudx, d2);
}

// ---- snapshot-wise parameter derivatives (include/nif_hip_snapparam.h) --------------------------------------------------
// The bias-free companion of k_latent_to_w: wd[a][s] = sum_k d[a][k] Wh[k][s] for `rows` direction rows d [rows][r] -- the tangent
// slot vector of a combined net along a latent direction (same slot layout as w_t; the hyper bias does not move).  The sum runs
// k = 0 .. r - 1 by fma from 0: scaling a direction by a power of two scales its row exactly.
__global__ __launch_bounds__(256) void k_dlatent_to_w(const float* __restrict__ theta, long off_Wh, int r, long po, const float* __restrict__ d,
                                                      float* __restrict__ wd) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= po) return;
  const float* dr = d + (long)blockIdx.y * r;
  float acc = 0.f;
  for (int k = 0; k < r; ++k) acc = fmaf(dr[k], theta[off_Wh + (long)k * po + s], acc);
  wd[(long)blockIdx.y * po + s] = acc;
}
void launch_dlatent_to_w(const float* theta, long off_Wh, int r, long po, const float* d, long rows, float* wd, hipStream_t st) {
  hipLaunchKernelGGL(k_dlatent_to_w, dim3((unsigned)((po + 255) / 256), (unsigned)rows), dim3(256), 0, st, theta, off_Wh, r, po, d, wd);
}
// the caller's directions [T][nd][r] -> direction-major rows [nd][T][r] (the layout the ParameterNet's tangents arrive in)
__global__ __launch_bounds__(256) void k_dir_rows(const float* __restrict__ drows, long T, int nd, int r, float* __restrict__ D) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= T * nd * r) return;
  const int k = (int)(e % r);
  const long td = e / r;
  const int d = (int)(td % nd);
  const long t = td / nd;
  D[((long)d * T + t) * r + k] = drows[e];
}
void launch_dir_rows(const float* drows, long T, int nd, int r, float* D, hipStream_t st) {
  hipLaunchKernelGGL(k_dir_rows, dim3((unsigned)((T * nd * r + 255) / 256)), dim3(256), 0, st, drows, T, nd, r, D);
}
// last-layer class on a shared mesh: k_phi_dot's result over the direction-major tangent coefficient rows, f [nd][T][M][so], ->
// rows y_idx of dudp [T][M][ny][nd]
__global__ __launch_bounds__(256) void k_snapparam_gather(const float* __restrict__ f, long T, long M, int so, int nd, HessIdx I,
                                                          float* __restrict__ dudp) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;      // (snapshot, point, i)
  if (e >= T * M * I.ny) return;
  const long a = e / I.ny; const int i = (int)(e - a * I.ny);
  for (int d = 0; d < nd; ++d) dudp[e * nd + d] = f[((long)d * T * M + a) * so + I.y_idx[i]];
}
void launch_snapparam_gather(const float* f, long T, long M, int so, int nd, const HessIdx& I, float* dudp, hipStream_t st) {
  hipLaunchKernelGGL(k_snapparam_gather, dim3((unsigned)((T * M * I.ny + 255) / 256)), dim3(256), 0, st, f, T, M, so, nd, I, dudp);
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

// second order (include/nif_hip_snapparam2.h), the table route: the parameter rows of HessianLayer's result over the
// columns [np parameters | nxc coordinates], H [rows][nx][nx] -> d2pp [rows][np][np] and d2px [rows][np][nxc]
__global__ __launch_bounds__(256) void k_snapparam2_blocks(const float* __restrict__ H, long rows, int np, int nxc, float* __restrict__ d2pp,
                                                           float* __restrict__ d2px) {
  const int nx = np + nxc;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * np * nx) return;
  const long row = idx / (np * nx);
  const int e = (int)(idx - row * (np * nx)), a = e / nx, col = e - a * nx;
  const float v = H[(row * nx + a) * nx + col];
  if (col < np) d2pp[(row * np + a) * np + col] = v;
  else d2px[(row * np + a) * nxc + (col - np)] = v;
}
void launch_snapparam2_blocks(const float* H, long rows, int np, int nxc, float* d2pp, float* d2px, hipStream_t st) {
  hipLaunchKernelGGL(k_snapparam2_blocks, dim3((unsigned)((rows * np * (np + nxc) + 255) / 256)), dim3(256), 0, st, H, rows, np, nxc, d2pp, d2px);
}
__global__ __launch_bounds__(256) void k_snapparam2_gather(const float* __restrict__ f, long n, long s_r, long s_n, long s_y, HessIdx I, Sp2Map map,
                                                           float* __restrict__ out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;      // (point, i)
  if (e >= n * I.ny) return;
  const long a = e / I.ny; const int i = (int)(e - a * I.ny);
  const float* src = f + a * s_n + I.y_idx[i] * s_y;
  for (int col = 0; col < map.n; ++col) out[e * map.n + col] = src[map.src[col] * s_r];
}
void launch_snapparam2_gather(const float* f, long n, long s_r, long s_n, long s_y, const HessIdx& I, const Sp2Map& map, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_snapparam2_gather, dim3((unsigned)((n * I.ny + 255) / 256)), dim3(256), 0, st, f, n, s_r, s_n, s_y, I, map, out);
}
// the source offsets k_through_lw takes, for a contiguous stack of n vectors of `stride` floats
__global__ void k_stride_offsets(long* __restrict__ off, int n, long stride) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) off[q] = (long)q * stride;
}
void launch_stride_offsets(long* off, int n, long stride, hipStream_t st) {
  hipLaunchKernelGGL(k_stride_offsets, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, off, n, stride);
}
