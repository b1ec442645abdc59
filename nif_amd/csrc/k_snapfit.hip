// k_snapfit.hip -- the head of the snapshot-wise training step (include/nif_hip_snapfit.h): the last-layer class on T
// snapshots of one shared mesh of M points, u[t][m][s] = sum_c phi[m][s][c] a[t][c] + bias[s].  The ShapeNet has run over the M mesh
// points (PHI [mesh tiles][so r][32]) and the ParameterNet over the T rows of p (a as tiles [snapshot tiles][r][32]); the head is the
// only O(T M) work of the step: one read of y, the loss, and the three sums the two adjoints start from
//     du[t][m][s]    = loss'(u - y) sw[t][m] / (Bg so)
//     DPHI[m][s][c]  = sum_t du[t][m][s] a[t][c]            DU[m][s] = sum_t du[t][m][s]            (inside the mesh tile's workgroup)
//     dL/da[t][c]    = sum_m sum_s phi[m][s][c] du[t][m][s]                                         (across workgroups)
//   k_sf_head:  one workgroup per 32-point mesh tile, k_phi_dot's shape: the tile's phi rows in LDS, the 8 point groups of the
//               workgroup walk the snapshots t = g, g + 8, ... (a of 32 snapshots at a time in LDS, y one snapshot ahead); u in
//               k_ll_out's order (bias first, then c = 0 .. r - 1 by fma).  Every thread keeps its point's so r DPHI sums and so DU
//               sums in registers (compile-time extents SOB x RB >= so x r, at most 64: nothing is indexed at run time, nothing
//               spills) and the 8 groups combine through LDS in the order g = 0 .. 7.  The sum over the tile's 32 points for dL/da
//               is a lane-transposing tree over the half wave (about pow2(r) exchanges instead of 5 r), stored as this tile's
//               partial DAP [mesh tile][T][r].
//   k_sf_da:    one workgroup per 32 snapshots and four columns of a: the partials of the mesh tiles summed in a fixed order (8
//               contiguous runs of tiles, then the runs in order) into DA [snapshot tiles][r][32]; k_sf_dzl: DZL = DA last_w^T in
//               k_ll_out's order.  Per-tile partials and this ordered second kernel rather than a second pass over y: the partials
//               are r / (32 so) of y's bytes, a second pass would read y twice and recompute u.
// No atomics: two calls agree bit for bit.
#include "nif_internal.h"

namespace {

// v[c], c < RP (a power of two <= 64), of the 32 lanes of a half wave -> their sums over the 32 lanes: every halving step sends one
// value of each pair to the partner lane and keeps the other, so RP values cost RP - 1 exchanges (+ 1 per step left when one value
// remains).  Afterwards lane p holds in v[j] the sum of index sf_lane_index(p) + 32 j
template <int RP>
__device__ __forceinline__ void sf_lane_sums(float (&v)[RP], int p) {
  int n = RP;
#pragma unroll
  for (int off = 16; off >= 1; off >>= 1) {
    if (n > 1) {
      const bool hi = (p & off) != 0;
#pragma unroll
      for (int i = 0; i < RP / 2; ++i)
        if (i < n / 2) {
          const float send = hi ? v[2 * i] : v[2 * i + 1];
          const float keep = hi ? v[2 * i + 1] : v[2 * i];
          v[i] = keep + __shfl_xor(send, off, 32);
        }
      n /= 2;
    } else {
      v[0] += __shfl_xor(v[0], off, 32);
    }
  }
}
// bit b of the index (b < min(5, log2 RP)) is bit 4 - b of the lane
template <int RP>
__device__ __forceinline__ int sf_lane_index(int p) {
  int c = 0;
#pragma unroll
  for (int b = 0; b < 5; ++b)
    if ((1 << b) < RP) c |= ((p >> (4 - b)) & 1) << b;
  return c;
}
constexpr int sf_pow2(int r) { return r <= 1 ? 1 : 2 * sf_pow2((r + 1) / 2); }

}  // namespace

template <int SOB, int RB>
__global__ __launch_bounds__(256) void k_sf_head(SnapFitArgs A) {
  extern __shared__ __attribute__((aligned(16))) float sf_lds[];      // phi [so r][32] | red [8 sums][8 groups][32] | a [r][32]
  __shared__ float lsum[4];
  constexpr int RP = sf_pow2(RB), NACC = SOB * RB;
  const int r = A.r, so = A.so, sop = so * r;
  float* phi = sf_lds;
  float* red = sf_lds + sop * 32;
  float* a_t = red + 8 * 8 * 32;      // a of the 32 snapshots of one snapshot tile [r][32]
  const long tile = blockIdx.x;
  for (int e = threadIdx.x; e < sop * 32; e += 256) phi[e] = A.PHI[tile * (long)sop * 32 + e];
  const int p = threadIdx.x & 31, g = threadIdx.x >> 5;
  const long m = tile * 32 + p;
  const bool valid = m < A.M;
  const long mc = valid ? m : A.M - 1;
  float bias[SOB], acc[NACC], dus[SOB];
#pragma unroll
  for (int s = 0; s < SOB; ++s) { bias[s] = s < so ? A.bias[s] : 0.f; dus[s] = 0.f; }
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
  float loss_lane = 0.f;
  // the targets and the weight of this group's next snapshot, loaded one snapshot ahead (the group walks t = g, g + 8, ...)
  float yn[SOB], wn = 0.f;
#pragma unroll
  for (int s = 0; s < SOB; ++s) yn[s] = 0.f;
  auto load_next = [&](long t) {
    if (t < A.T) {
      wn = valid ? (A.sw ? A.sw[t * A.M + mc] : 1.0f) : 0.0f;
      const float* yt = A.y + (t * A.M + mc) * so;
#pragma unroll
      for (int s = 0; s < SOB; ++s)
        if (s < so) yn[s] = yt[s];
    }
  };
  load_next(g);
  const long ttiles = (A.T + 31) / 32;
  for (long tt = 0; tt < ttiles; ++tt) {
    __syncthreads();      // (the first: phi is in place; later: the groups are done with the last tile's a)
    for (int e = threadIdx.x; e < r * 32; e += 256) a_t[e] = A.A[tt * (long)r * 32 + e];
    __syncthreads();
    for (int tl = g; tl < 32; tl += 8) {
      const long t = tt * 32 + tl;
      if (t >= A.T) break;
      float a[RB], du[SOB], dv[RP], yc[SOB];
#pragma unroll
      for (int c = 0; c < RB; ++c) a[c] = c < r ? a_t[c * 32 + tl] : 0.f;
      const float wsamp = wn;
#pragma unroll
      for (int s = 0; s < SOB; ++s) yc[s] = yn[s];
      load_next(t + 8);
      float se = 0.f;
#pragma unroll
      for (int s = 0; s < SOB; ++s) {
        du[s] = 0.f;
        if (s < so) {
          float u = bias[s];
#pragma unroll
          for (int c = 0; c < RB; ++c)
            if (c < r) u = fmaf(phi[(s * r + c) * 32 + p], a[c], u);
          const float e = u - yc[s];
          NIF_LOSS_ACC(A.loss_kind, e, se, dfac)
          du[s] = dfac * wsamp * A.inv_bg / (float)so;
          dus[s] += du[s];
#pragma unroll
          for (int c = 0; c < RB; ++c)
            if (c < r) acc[s * RB + c] = fmaf(du[s], a[c], acc[s * RB + c]);
        }
      }
      loss_lane += wsamp * se / (float)so * A.inv_bg;
      // this tile's share of dL/da[t]: k_ll_out's sum over s per point, then the 32 points
#pragma unroll
      for (int c = 0; c < RP; ++c) {
        float v = 0.f;
        if (c < r) {
#pragma unroll
          for (int s = 0; s < SOB; ++s)
            if (s < so) v = fmaf(phi[(s * r + c) * 32 + p], du[s], v);
        }
        dv[c] = v;
      }
      sf_lane_sums<RP>(dv, p);
      const int cl = sf_lane_index<RP>(p);
      float* dap = A.DAP + (tile * A.T + t) * r;
      if (RP >= 32 || (p & ((32 / RP) - 1)) == 0) {      // (below 32 values the lanes that differ in the low bits hold copies)
        if (cl < r) dap[cl] = dv[0];
        if (RP > 32 && cl + 32 < r) dap[cl + 32] = dv[RP > 32 ? 1 : 0];
      }
    }
  }
  __syncthreads();
  // the 8 groups' sums over their snapshots, in the order g = 0 .. 7: eight sums per pass, thread (g, p) adds up sum g of the pass
#pragma unroll
  for (int q = 0; q < (NACC + 7) / 8; ++q) {
    if ((q * 8) / RB < so) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (q * 8 + j < NACC) red[(j * 8 + g) * 32 + p] = acc[q * 8 + j];
      __syncthreads();
      const int k = q * 8 + g, s = k / RB, c = k - s * RB;
      if (k < NACC && s < so && c < r) {
        float v = red[(g * 8) * 32 + p];
        for (int gg = 1; gg < 8; ++gg) v += red[(g * 8 + gg) * 32 + p];
        A.DPHI[(tile * (long)sop + s * r + c) * 32 + p] = v;
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int q = 0; q < (SOB + 7) / 8; ++q) {
    if (q * 8 < so) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (q * 8 + j < SOB) red[(j * 8 + g) * 32 + p] = dus[q * 8 + j];
      __syncthreads();
      const int s = q * 8 + g;
      if (s < so) {
        float v = red[(g * 8) * 32 + p];
        for (int gg = 1; gg < 8; ++gg) v += red[(g * 8 + gg) * 32 + p];
        A.DU[(tile * so + s) * 32 + p] = v;
      }
      __syncthreads();
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int off = 32; off > 0; off >>= 1) loss_lane += __shfl_down(loss_lane, off);
  if (lane == 0) lsum[wid] = loss_lane;
  __syncthreads();
  if (threadIdx.x == 0) A.loss_partial[blockIdx.x] = (lsum[0] + lsum[1]) + (lsum[2] + lsum[3]);
}

// grid = (snapshot tiles, groups of four columns of a).  Thread (run, p): snapshot t = 32 tile + p, the mesh tiles of run `run` (8
// contiguous runs) in order; then the runs in order
__global__ __launch_bounds__(256) void k_sf_da(SnapFitArgs A) {
  __shared__ float red[4][8][32];
  const int r = A.r, c0 = blockIdx.y * 4;
  const long tt = blockIdx.x, mtiles = (A.M + 31) / 32;
  const int p = threadIdx.x & 31, run = threadIdx.x >> 5;
  const long t = tt * 32 + p;
  const bool valid = t < A.T;      // (the padding rows of the last snapshot tile: zeros, as k_ll_out leaves them)
  const long per = (mtiles + 7) / 8;
  const long lo = run * per, hi = lo + per < mtiles ? lo + per : mtiles;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid)
    for (long tile = lo; tile < hi; ++tile) {
      const float* q = A.DAP + (tile * A.T + t) * r + c0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < r) s[j] += q[j];
    }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[j][run][p] = s[j];
  __syncthreads();
  if (run < 4 && c0 + run < r) {      // (thread (j, p) adds up column c0 + j)
    float v = red[run][0][p];
    for (int k = 1; k < 8; ++k) v += red[run][k][p];
    A.DA[(tt * r + c0 + run) * 32 + p] = v;
  }
}
// grid = snapshot tiles: DZL = DA last_w^T, k_ll_out's sum (c = 0 .. r - 1 by fma)
__global__ __launch_bounds__(256) void k_sf_dzl(SnapFitArgs A) {
  const int r = A.r;
  const long tt = blockIdx.x;
  for (int e = threadIdx.x; e < r * 32; e += 256) {
    const int k = e >> 5, pp = e & 31;
    float dz = 0.f;
    for (int c = 0; c < r; ++c) dz = fmaf(A.DA[(tt * r + c) * 32 + pp], A.last_w[(long)k * r + c], dz);
    A.DZL[(tt * r + k) * 32 + pp] = dz;
  }
}

bool snapfit_supported(int r, int so) { return r >= 1 && so >= 1 && (long)r * so <= 64; }
long snapfit_dap_floats(long T, long M, int r) { return ((M + 31) / 32) * T * r; }

// The extents SOB x RB >= so x r of the head's register sums, at most 64 in every form.  The forms cover every (so, r) with
// so r <= 64: so <= 8 fits <so', 64 / so'>, anything larger has r <= 7 and fits <64 / r, r>.  Of the forms that fit, the one with the
// fewest exchanges and guarded iterations per sample (pow2(RB) + SOB) runs
#define NIF_SF_FORMS(X) \
  X(64, 1) X(32, 2) X(16, 4) X(8, 8) X(4, 16) X(2, 32) X(1, 64) X(3, 21) X(5, 12) X(6, 10) X(7, 9) X(21, 3) X(12, 5) X(10, 6) X(9, 7)
void launch_snapfit_head(const SnapFitArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.M + 31) / 32)), block(256);
  const size_t shm = sizeof(float) * ((size_t)a.r * a.so * 32 + 8 * 8 * 32 + (size_t)a.r * 32);
  int best_sob = 0, best_rb = 0, best_cost = 1 << 30;
#define NIF_SF_PICK(SOB_, RB_)                                                                                             \
  if (SOB_ >= a.so && RB_ >= a.r && sf_pow2(RB_) + SOB_ < best_cost) { best_cost = sf_pow2(RB_) + SOB_; best_sob = SOB_; best_rb = RB_; }
  NIF_SF_FORMS(NIF_SF_PICK)
#undef NIF_SF_PICK
#define NIF_SF_RUN(SOB_, RB_) \
  if (best_sob == SOB_ && best_rb == RB_) { hipLaunchKernelGGL((k_sf_head<SOB_, RB_>), grid, block, shm, st, a); return; }
  NIF_SF_FORMS(NIF_SF_RUN)
#undef NIF_SF_RUN
}
void launch_snapfit_da(const SnapFitArgs& a, hipStream_t st) {
  const unsigned ttiles = (unsigned)((a.T + 31) / 32);
  hipLaunchKernelGGL(k_sf_da, dim3(ttiles, (unsigned)((a.r + 3) / 4)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_sf_dzl, dim3(ttiles), dim3(256), 0, st, a);
}
