// k_encode.hip -- per-snapshot Gauss-Newton normal equations in the latent (include/nif_hip_encode.h): the device half of
// Model.encode_snapshots.  For snapshot t with latent z_t, points x_m, targets y_m and weights w_m
//     S_t = sum_m w_m sum_i q q^T,   q = [du_i/dz (z_t; x_m), u_i(z_t; x_m) - y_m,i]  in R^(r+1)
// (A = J^T W J in the leading block, g = J^T W e in the last column, c = sum w |e|^2 in the corner).
//   k_encode_expand: the operands of the UNCHANGED point-wise kernels in a padded layout where every snapshot owns whole 32-point
//                    tiles -- the latent tiles Z with every point of snapshot t carrying z_t, the padded coordinates, and the unit
//                    pattern whose shifted views are the unit tiles e_k: k_jac's parameter-seed stream adds, in every layer,
//                    sum_k z'_k (h . M^(k)) + z'_k b^(k); seeded with z' = e_k it carries du/dz_k (nif_api.hip: nif_snapshot_normal_eq_dev).
//   k_encode_gram:   one workgroup per snapshot reads J, u, y and w once and forms S_t: products in fp32, the 32 points of one
//                    (tile, output) unit summed in fp32, float64 across the units, in an order fixed by the snapshot's own point
//                    count.  No atomics: two calls agree bit for bit, and a snapshot's result does not depend on where in the
//                    call (or in which chunk) it sits.  Last-layer class: u = phi . a + bias is linear in a, J = phi, both read
//                    from the phi tiles of the x -> phi pass.
// Roofline of the reducer: 4 so (r + 1) bytes and so (r + 1)^2 FMAs per point -- (r + 1) / 4 FMA/B against 157.3 TFLOP/s / 2 / 6.29 TB/s
// = 12.5 FMA/B of the fp32 vector rate: HBM-bound below r ~ 50, so plain FMAs from LDS, no MFMA form.
#include "nif_internal.h"

// the last t in [t0, t1) with tile_start[t] <= gt (snapshots without points own no tile)
__device__ __forceinline__ long enc_snap_of(const EncArgs& A, long gt) {
  long lo = A.t0, hi = A.t1;
  while (hi - lo > 1) {
    const long mid = (lo + hi) >> 1;
    if (A.tile_start[mid] <= gt) lo = mid; else hi = mid;
  }
  return lo;
}

// one thread per point of the chunk's padded tiles
__global__ __launch_bounds__(256) void k_encode_expand(EncArgs A, long ntiles) {
  const long pt = (long)blockIdx.x * 256 + threadIdx.x;
  if (pt >= ntiles * 32) return;
  const long tile = pt >> 5;
  const int p = (int)(pt & 31), r = A.r;
  const long gt = tile + A.tile_start[A.t0];
  const long t = enc_snap_of(A, gt);
  if (A.Z) {
    float* z = A.Z + tile * (long)r * 32 + p;
    for (int k = 0; k < r; ++k) z[k * 32] = A.lat[t * r + k];
  }
  if (A.unit) {
    float* un = A.unit + tile * (long)r * 32 + p;
    for (int k = 0; k < r; ++k) un[k * 32] = k == 0 ? 1.f : 0.f;
    if (tile == ntiles - 1)
      for (int k = 0; k < r; ++k) un[(r + k) * 32] = k == 0 ? 1.f : 0.f;
  }
  if (A.xpad) {
    const long m_t = A.offsets ? A.offsets[t + 1] - A.offsets[t] : A.M;
    long local = (gt - A.tile_start[t]) * 32 + p;
    if (local > m_t - 1) local = m_t - 1;        // padding repeats the snapshot's last point (weight 0 in the reducer)
    const float* xr = A.x + ((A.offsets ? A.offsets[t] : 0) + local) * A.si;
    float* row = A.xpad + pt * A.si;
    for (int d = 0; d < A.si; ++d) row[d] = xr[d];
  }
}
void launch_encode_expand(const EncArgs& a, long ntiles, hipStream_t st) {
  if (ntiles <= 0) return;
  hipLaunchKernelGGL(k_encode_expand, dim3((unsigned)((ntiles * 32 + 255) / 256)), dim3(256), 0, st, a, ntiles);
}

// Workgroup = snapshot.  A unit is one (tile, output channel) pair: 32 rows q.  E = (r + 1)^2 elements of S; with E <= 256 the
// workgroup holds G = 256 / E units at a time and thread (g, e) sums element e of the units g, g + G, ... in float64; else G = 1 and a
// thread owns the elements tid, tid + 256, ...  LDS: acc [G][E] float64 | q [G][32][r + 1] | wq [G][32]
__global__ __launch_bounds__(256) void k_encode_gram(EncArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char enc_smem[];
  const int tid = threadIdx.x, r = A.r, so = A.so, Q = r + 1, E = Q * Q;
  const int G = E <= 256 ? 256 / E : 1;
  double* acc = reinterpret_cast<double*>(enc_smem);
  float* qs = reinterpret_cast<float*>(acc + (size_t)G * E);
  float* wq = qs + (size_t)G * 32 * Q;
  const long t = A.t0 + blockIdx.x;
  const long tile0 = A.tile_start[t] - A.tile_start[A.t0], ntile = A.tile_start[t + 1] - A.tile_start[t];
  const long m_t = A.offsets ? A.offsets[t + 1] - A.offsets[t] : A.M;
  const long base = A.offsets ? A.offsets[t] : t * A.M;       // first row of the snapshot in y / w
  const long nunits = ntile * so;
  const float* lat = A.lat + t * r;
  for (int i = tid; i < G * E; i += 256) acc[i] = 0.0;
  const int my_g = E <= 256 ? tid / E : 0;
  const int e0 = E <= 256 ? tid - my_g * E : tid, estep = E <= 256 ? E : 256;
  const bool worker = my_g < G;
  __syncthreads();
  for (long ub = 0; ub < nunits; ub += G) {
    for (int idx = tid; idx < G * 32 * Q; idx += 256) {
      const int g = idx / (32 * Q), rem = idx - g * 32 * Q, p = rem / Q, k = rem - p * Q;
      const long u = ub + g;
      float v = 0.f;
      if (u < nunits) {
        const long tl = u / so; const int o = (int)(u - tl * so);
        const long local = tl * 32 + p;
        const bool valid = local < m_t;
        if (A.PHI) {
          const float* ph = A.PHI + ((A.phi_shared ? tl : tile0 + tl) * so + o) * (long)r * 32 + p;
          if (k < r) v = valid ? ph[k * 32] : 0.f;      // (a padding lane of the mesh's last phi tile holds nothing)
          else {
            float s = A.bias[o];      // k_ll_out's order: the bias first, then c = 0 .. r - 1 by fma
            for (int c = 0; c < r; ++c) s = fmaf(ph[c * 32], lat[c], s);
            v = valid ? s - A.y[(base + local) * so + o] : 0.f;
          }
        } else {
          const long row = ((tile0 + tl) * 32 + p) * so + o;
          if (k < r) v = valid ? A.dydx[row * r + k] : 0.f;
          else v = valid ? A.u[row] - A.y[(base + local) * so + o] : 0.f;
        }
        if (k == 0) wq[g * 32 + p] = valid ? (A.w ? A.w[base + local] : 1.f) : 0.f;
      }
      qs[idx] = v;
    }
    __syncthreads();
    if (worker && ub + my_g < nunits) {
      const float* q = qs + (size_t)my_g * 32 * Q;
      const float* wv = wq + my_g * 32;
      for (int e = e0; e < E; e += estep) {
        const int a = e / Q, b = e - a * Q;
        float s = 0.f;
#pragma unroll 8
        for (int p = 0; p < 32; ++p) s = fmaf(wv[p], q[p * Q + a] * q[p * Q + b], s);      // (q_a q_b first: S is symmetric bit for bit)
        acc[my_g * E + e] += (double)s;
      }
    }
    __syncthreads();
  }
  double* S = A.S + t * (long)E;
  for (int e = tid; e < E; e += 256) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += acc[g * E + e];
    S[e] = s;
  }
}
void launch_encode_gram(const EncArgs& a, hipStream_t st) {
  if (a.t1 <= a.t0) return;
  const int Q = a.r + 1, E = Q * Q, G = E <= 256 ? 256 / E : 1;
  const size_t shm = sizeof(double) * (size_t)G * E + sizeof(float) * ((size_t)G * 32 * Q + (size_t)G * 32);
  hipLaunchKernelGGL(k_encode_gram, dim3((unsigned)(a.t1 - a.t0)), dim3(256), shm, st, a);
}
