// k_sensors.hip -- sensor placement on the last-layer class's basis (include/nif_hip_sensors.h): greedy column-pivoted QR
// (Businger-Golub, QDEIM) of Phi^T, Phi = model_x_to_phi(x) as N = M so candidate rows of r floats, row m so + s = output s at mesh
// point m.  Step k takes the eligible row of the largest squared norm (ties: the lowest row), d_k its norm and q_k = row / d_k, and
// takes q_k out of every row: row -= (row . q_k) q_k.  A row's score is recomputed from its updated values in the pass that updates
// it, so there is no norm down-dating and none of LAPACK's cancellation guard.
//   RES [tiles][so r][32]   the running residual in PHI's own tile layout (lane = point: a wave's loads are 128-byte rows); c->PHI
//                           itself belongs to the other entries
//   SC  [tiles][so][32]     a row's score; -1 = no candidate (masked, a padding lane of the last tile, already chosen)
//   PS, PR [workgroups]     every workgroup's best (score, row) of the last pass: the grid is persistent and bounded (sens_grid), so
//                           the list has a fixed length
//   k_sens_init:    PHI -> RES, every score, the partials
//   k_sens_pivot:   one workgroup: the partials' argmax, q_k / pivots[k] / d[k] from the row as stored -- or -1 / 0 / a zero q_k when
//                   no eligible row has a positive score (too few candidates, rank exhausted)
//   k_sens_update:  a thread owns a point and loops over its so rows; r padded to a compile-time RB (nothing is register-indexed at
//                   run time); alpha = sum_c q_c v_c by fma in the order c = 0 .. r - 1, v -= alpha q, the new score, the store; the
//                   chosen row is zeroed and scored -1; the block's argmax is the partial of the next step
// The argmax is a maximum under a total order (score, then the lower row): any reduction order gives the same pair.  No atomics: two
// calls agree bit for bit.  A row's arithmetic depends on that row and q_k alone, so a permuted mesh gives the permuted pivots.
#include "nif_internal.h"

namespace {

constexpr long long SENS_NOROW = 0x7fffffffffffffffLL;

__device__ __forceinline__ bool sens_better(float s, long long row, float bs, long long brow) {
  return s > bs || (s == bs && row < brow);
}
// the workgroup's best pair, valid in thread 0
__device__ __forceinline__ void sens_block_best(float& bs, long long& br) {
  __shared__ float ws[4];
  __shared__ long long wr[4];
  for (int off = 32; off > 0; off >>= 1) {
    const float s = __shfl_down(bs, off);
    const long long row = __shfl_down(br, off);
    if (sens_better(s, row, bs, br)) { bs = s; br = row; }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { ws[wid] = bs; wr[wid] = br; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w)
      if (sens_better(ws[w], wr[w], bs, br)) { bs = ws[w]; br = wr[w]; }
}

}  // namespace

// grid = sens_grid(M, r) workgroups of 8 tiles each per stride
__global__ __launch_bounds__(256) void k_sens_init(SensArgs A) {
  const int r = A.r, so = A.so, sop = r * so;
  const long tiles = (A.M + 31) / 32;
  const int p = threadIdx.x & 31, g = threadIdx.x >> 5;
  float bs = -1.f;
  long long br = SENS_NOROW;
  for (long tile = blockIdx.x * 8L + g; tile < tiles; tile += gridDim.x * 8L) {
    const long m = tile * 32 + p;
    const bool valid = m < A.M;
    const bool elig = valid && (!A.mask || A.mask[m] != 0);
    for (int s = 0; s < so; ++s) {
      const long base = (tile * sop + (long)s * r) * 32 + p;
      float sc = 0.f;
      for (int c = 0; c < r; ++c) {
        const float v = valid ? A.PHI[base + c * 32] : 0.f;
        A.RES[base + c * 32] = v;
        sc = fmaf(v, v, sc);
      }
      if (!elig) sc = -1.f;
      A.SC[(tile * so + s) * 32 + p] = sc;
      const long long row = (long long)m * so + s;
      if (sens_better(sc, row, bs, br)) { bs = sc; br = row; }
    }
  }
  sens_block_best(bs, br);
  if (threadIdx.x == 0) { A.PS[blockIdx.x] = bs; A.PR[blockIdx.x] = br; }
}

// one workgroup; nparts = the grid of the pass before
__global__ __launch_bounds__(256) void k_sens_pivot(SensArgs A, int nparts) {
  __shared__ float s_bs;
  __shared__ long long s_br;
  const int r = A.r, so = A.so, k = A.k;
  float bs = -1.f;
  long long br = SENS_NOROW;
  for (int i = threadIdx.x; i < nparts; i += 256) {
    const float s = A.PS[i];
    const long long row = A.PR[i];
    if (sens_better(s, row, bs, br)) { bs = s; br = row; }
  }
  sens_block_best(bs, br);
  if (threadIdx.x == 0) { s_bs = bs; s_br = br; }
  __syncthreads();
  bs = s_bs; br = s_br;
  const int c = threadIdx.x;
  if (!(bs > 0.f)) {      // nothing left: this step and, the partials staying as they are, every later one
    if (c < r) A.Q[(long)k * r + c] = 0.f;
    if (c == 0) { A.piv[k] = -1; A.d[k] = 0.f; }
    return;
  }
  const long m = (long)(br / so);
  const int s = (int)(br - (long long)m * so);
  const float* row = A.RES + ((m >> 5) * (long)(r * so) + (long)s * r) * 32 + (m & 31);
  float ss = 0.f;
  for (int j = 0; j < r; ++j) { const float v = row[j * 32]; ss = fmaf(v, v, ss); }
  const float d = sqrtf(ss);
  if (c < r) A.Q[(long)k * r + c] = row[c * 32] / d;
  if (c == 0) { A.piv[k] = br; A.d[k] = d; }
}

// RMIN <= r <= RB: the columns below RMIN need no guard
template <int RB, int RMIN>
__global__ __launch_bounds__(256) void k_sens_update(SensArgs A) {
  const long long piv = A.piv[A.k];
  if (piv < 0) return;      // (the partials stay: the next k_sens_pivot finds nothing again)
  const int r = A.r, so = A.so, sop = r * so;
  const long tiles = (A.M + 31) / 32;
  const int p = threadIdx.x & 31, g = threadIdx.x >> 5;
  // q_k is uniform: up to 16 values stay in scalar registers; a longer one would spill them, and goes through LDS (broadcast reads)
  constexpr bool QL = RB > 16;
  __shared__ float qs[QL ? RB : 1];
  float qr[QL ? 1 : RB];
  if constexpr (QL) {
    if ((int)threadIdx.x < RB) qs[threadIdx.x] = (int)threadIdx.x < r ? A.Q[(long)A.k * r + threadIdx.x] : 0.f;
    __syncthreads();
  } else {
#pragma unroll
    for (int c = 0; c < RB; ++c) qr[c] = c < r ? A.Q[(long)A.k * r + c] : 0.f;
  }
  auto q = [&](int c) { if constexpr (QL) return qs[c]; else return qr[c]; };
  float bs = -1.f;
  long long br = SENS_NOROW;
  for (long tile = blockIdx.x * 8L + g; tile < tiles; tile += gridDim.x * 8L) {
    const long m = tile * 32 + p;
    for (int s = 0; s < so; ++s) {
      const long si = (tile * so + s) * 32 + p;
      if (A.SC[si] < 0.f) continue;      // no candidate: its residual is never read again
      float* row = A.RES + (tile * sop + (long)s * r) * 32 + p;
      const long long rowi = (long long)m * so + s;
      float v[RB];
#pragma unroll
      for (int c = 0; c < RB; ++c) v[c] = (c < RMIN || c < r) ? row[c * 32] : 0.f;
      float al = 0.f;
#pragma unroll
      for (int c = 0; c < RB; ++c) al = fmaf(q(c), v[c], al);      // (the padding adds fma(0, 0, al) = al)
      float sc = 0.f;
#pragma unroll
      for (int c = 0; c < RB; ++c) { v[c] = fmaf(-al, q(c), v[c]); sc = fmaf(v[c], v[c], sc); }
      const bool chosen = rowi == piv;
      if (chosen) sc = -1.f;
#pragma unroll
      for (int c = 0; c < RB; ++c)
        if (c < RMIN || c < r) row[c * 32] = chosen ? 0.f : v[c];
      A.SC[si] = sc;
      if (sens_better(sc, rowi, bs, br)) { bs = sc; br = rowi; }
    }
  }
  sens_block_best(bs, br);
  if (threadIdx.x == 0) { A.PS[blockIdx.x] = bs; A.PR[blockIdx.x] = br; }
}

// 1024 workgroups of four waves are 16 waves on each of the 256 CUs: at r = 10 about 10 MB of loads in flight, what the HBM's
// latency-bandwidth product asks for.  Above r = 40 a row takes 150 and more vector registers and two workgroups fit a CU: 512, so
// that every workgroup is resident and the strides end together.  One workgroup takes 8 tiles per stride
int sens_grid(long M, int r) {
  const long groups = ((M + 31) / 32 + 7) / 8, bound = r > 40 ? NIF_SENS_GRID / 2 : NIF_SENS_GRID;
  return (int)(groups < bound ? groups : bound);
}
bool sens_supported(int r) { return r >= 1 && r <= 64; }
void launch_sens_init(const SensArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_sens_init, dim3((unsigned)sens_grid(a.M, a.r)), dim3(256), 0, st, a);
}
void launch_sens_pivot(const SensArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_sens_pivot, dim3(1), dim3(256), 0, st, a, sens_grid(a.M, a.r));
}
// (RB, RMIN): RB the register extent, RMIN - 1 the form before it: at most seven guarded columns in any form
#define NIF_SENS_FORMS(X) \
  X(1, 1) X(2, 2) X(3, 3) X(4, 4) X(5, 5) X(6, 6) X(7, 7) X(8, 8) X(10, 9) X(12, 11) X(14, 13) X(16, 15) X(20, 17) X(24, 21) X(28, 25) \
  X(32, 29) X(40, 33) X(48, 41) X(56, 49) X(64, 57)
void launch_sens_update(const SensArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)sens_grid(a.M, a.r)), block(256);
#define NIF_SENS_RUN(RB_, RMIN_) \
  if (a.r <= RB_) { hipLaunchKernelGGL((k_sens_update<RB_, RMIN_>), grid, block, 0, st, a); return; }
  NIF_SENS_FORMS(NIF_SENS_RUN)
#undef NIF_SENS_RUN
}
