// k_gradtf.hip -- the gradient transform in front of the optimizer update (gfx950; include/nif_hip.h nif_set_grad_transform; reference
// nif/optimizers/gtcf.py:7-67 and Keras' clipnorm / clipvalue / global_clipnorm): centralise every matrix gradient over its rows, clip
// by value, clip by norm per tensor or by the global norm, in place on the flat gradient g[0, P) (the loss slot g[P] is not touched).
// The work is a few megabytes spread over 8..40 tensors of very different sizes, so it is cut by (tensor, column block), not by tensor:
//   * a work block (GtBlk) of a matrix [rows, cols] is 64 columns over ALL rows, so the block forms the column means and the centred
//     sum of squares of its columns without a grid-wide dependency; a vector is cut into chunks of 4096 floats, laid out as 64 columns.
//   * k_gt_reduce: thread (column c, row group rg of 4) sums its rows i = rg, rg + 4, ... in order; the four row groups add as
//     (s0 + s1) + (s2 + s3); mean = sum / rows; x = g - mean (stored); the squares add the same way, then the 64 columns of the block
//     by a shuffle tree (lane l += lane l + 32, 16, 8, 4, 2, 1) into ONE partial per block.  Where no norm stage follows, the clamp
//     (Keras' clipvalue, or gtcf's with clipnorm off) runs here as well and the transform is this one launch.
//   * k_gt_apply: every block re-adds the partials it needs -- its tensor's (Keras clipnorm) and all of them in block order (global
//     norms) -- with block_sum: thread t adds partials t, t + 256, ... in order, then a halving tree over the 256 threads.  The same
//     code over the same numbers in every block and on every rank: no floating-point atomics, one scale per tensor, bit-identical
//     replicas.  Then one pass rewrites g: scale, and gtcf's clamp behind it.
// Longest chain of additions: 32 rows + 2 + 6 in a block, then a few partials per thread + 8: the sum of squares is off by a few
// 1e-6 relative at worst.  Flags and constants come from device memory (GtDev) in every form, so a captured graph replays with the
// constants of the replay.  Contraction off and every per-element expression written once, so that tests/gradtf_ref.py can follow
// the float sequence.
#include "nif_internal.h"

#pragma clang fp contract(off)

namespace {

struct GtPlan { bool cen, norm, clamp_a, clamp_b; int stage; };      // stage: 0 none, 3 per tensor, 4 Keras global, 5 gtcf global
__device__ __forceinline__ GtPlan gt_plan(const GtDev& d, bool matrix) {
  GtPlan p;
  const bool gtcf = (d.flags & GT_GTCF) != 0;
  p.cen = (d.flags & GT_CENTRALIZE) && matrix;
  p.stage = gtcf ? (d.clipnorm > 0.f ? 5 : 0) : (d.clipnorm > 0.f ? 3 : (d.global_clipnorm > 0.f ? 4 : 0));
  p.norm = p.stage != 0;
  p.clamp_a = !p.norm && d.clipvalue > 0.f;
  p.clamp_b = p.norm && gtcf && d.clipvalue > 0.f;
  return p;
}

// min(max(x, -c), c) as tf.clip_by_value: NaN stays NaN, -0 stays -0
__device__ __forceinline__ float clamp_1(float x, float c) { return x < -c ? -c : (x > c ? c : x); }
// Keras clipnorm (tf.clip_by_norm): (x c) / max(n, c)
__device__ __forceinline__ float clipnorm_1(float x, float c, float n) { return (x * c) / ((n != n || n > c) ? n : c); }
// gtcf clipnorm (legacy clip_norm): (x c) / n where n >= c
__device__ __forceinline__ float gtcf_norm_1(float x, float c, float n) { return n >= c ? (x * c) / n : x; }
// Keras global_clipnorm (tf.clip_by_global_norm): the factor c min(1 / n, 1 / c); NaN for a non-finite norm
__device__ __forceinline__ float global_factor(float c, float n) {
  if (!(n - n == 0.f)) return __uint_as_float(0x7fc00000u);
  const float a = 1.0f / n, b = 1.0f / c;
  return c * (a < b ? a : b);
}

// the sum of p[0, n) on every thread of a 256-thread block: thread t adds p[t], p[t + 256], ... in order, then a halving tree
__device__ __forceinline__ float block_sum(const float* __restrict__ p, int n, float* red) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += p[i];
  __syncthreads();      // (red may still be read from the previous sum)
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  return red[0];
}

}  // namespace

// one block per GtBlk: centralise (stored), clamp where no norm stage follows (stored), the block's sum of squares into part[block]
__global__ __launch_bounds__(256) void k_gt_reduce(float* __restrict__ g, const GtBlk* __restrict__ blks, float* __restrict__ part,
                                                   const GtDev* __restrict__ gd) {
  __shared__ float red[4][64];
  const GtBlk b = blks[blockIdx.x];
  const GtDev d = *gd;
  const GtPlan p = gt_plan(d, b.matrix != 0);
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  float* __restrict__ gb = g + b.base;
  const bool col_ok = c < b.nc;
  float mean = 0.f;
  if (p.cen) {
    float s = 0.f;
    if (col_ok)
      for (int i = rg; i < b.rows; i += 4) { const long e = (long)i * b.stride + c; if (e < b.lim) s += gb[e]; }
    red[rg][c] = s;
    __syncthreads();
    mean = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) / (float)b.rows;
    __syncthreads();
  }
  float q = 0.f;
  if (col_ok)
    for (int i = rg; i < b.rows; i += 4) {
      const long e = (long)i * b.stride + c;
      if (e < b.lim) {
        float x = gb[e];
        if (p.cen) x = x - mean;
        if (p.clamp_a) x = clamp_1(x, d.clipvalue);
        if (p.cen || p.clamp_a) gb[e] = x;
        q += x * x;
      }
    }
  red[rg][c] = q;
  __syncthreads();
  if (threadIdx.x < 64) {
    float v = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
  }
}

// one block per GtBlk: the norms from the partials (norms[t] per tensor, norms[ntensor] global), then the norm stage and gtcf's clamp.
// write = 0: the norms only (nif_grad_norms behind a transform without a norm stage)
__global__ __launch_bounds__(256) void k_gt_apply(float* __restrict__ g, const GtBlk* __restrict__ blks, int nblk, int ntensor,
                                                  const float* __restrict__ part, float* __restrict__ norms,
                                                  const GtDev* __restrict__ gd, int write) {
  __shared__ float red[256];
  const GtBlk b = blks[blockIdx.x];
  const GtDev d = *gd;
  const GtPlan p = gt_plan(d, b.matrix != 0);
  const bool first = (int)blockIdx.x == b.pb0;
  float nt = 0.f, ng = 0.f;
  if (p.stage == 3 || first) nt = sqrtf(block_sum(part + b.pb0, b.pbn, red));
  if (p.stage >= 4 || blockIdx.x == 0) ng = sqrtf(block_sum(part, nblk, red));
  if (threadIdx.x == 0) {
    if (first) norms[b.tensor] = nt;
    if (blockIdx.x == 0) norms[ntensor] = ng;
  }
  if (!write || !p.norm) return;
  const float cn = d.clipnorm, f4 = p.stage == 4 ? global_factor(d.global_clipnorm, ng) : 0.f;
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  float* __restrict__ gb = g + b.base;
  if (c >= b.nc) return;
  for (int i = rg; i < b.rows; i += 4) {
    const long e = (long)i * b.stride + c;
    if (e < b.lim) {
      float x = gb[e];
      if (p.stage == 3) x = clipnorm_1(x, cn, nt);
      else if (p.stage == 4) x = x * f4;
      else x = gtcf_norm_1(x, cn, ng);
      if (p.clamp_b) x = clamp_1(x, d.clipvalue);
      gb[e] = x;
    }
  }
}

void launch_gt_reduce(float* g, const GtBlk* blks, int nblk, float* part, const GtDev* gd, hipStream_t st) {
  hipLaunchKernelGGL(k_gt_reduce, dim3((unsigned)nblk), dim3(256), 0, st, g, blks, part, gd);
}
void launch_gt_apply(float* g, const GtBlk* blks, int nblk, int ntensor, const float* part, float* norms, const GtDev* gd, bool write,
                     hipStream_t st) {
  hipLaunchKernelGGL(k_gt_apply, dim3((unsigned)nblk), dim3(256), 0, st, g, blks, nblk, ntensor, part, norms, gd, write ? 1 : 0);
}
