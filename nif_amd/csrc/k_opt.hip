// k_opt.hip -- the reference's Lion and AdaBelief updates (nif/optimizers/external_optimizers.py:631-735, :322-628) on the flat
// parameter vector (gfx950).  Three forms of each, like Adam's in k_misc.hip:
//   * k_lion / k_adabelief<AMS>: the update alone over [0, P), behind an all-reduce, a regulariser or a flushed row reduction.  A stream
//     bound by bandwidth: Lion reads theta, g, m (12 B) and writes theta, m (8 B) per parameter; AdaBelief 16 B / 12 B, with amsgrad
//     20 B / 16 B.  Four parameters per thread with 16-byte accesses where every buffer is 16-byte aligned, a scalar tail for P % 4.
//   * k_reduce_lion / k_reduce_adabelief<AMS>: k_reduce's row sum of column i (same summation order), g[i] and the loss g[P] still
//     written, then the update of column i behind its sum -- bit-identical to k_reduce followed by the standalone update.
//   * k_lion_dev / k_adabelief_dev<AMS>: hyper-parameters and iteration count from device memory (OptDev) for captured graphs; each
//     block forms the step's scalars in fp64 (opt_scalars, the host's own function), k_opt_step_inc bumps the count behind the update.
// Every form runs the same per-element expressions (lion_1 / adab_1) with contraction off, so that the update is the same float
// sequence the NumPy restatement of the tests computes, whichever form ran it.
#include "nif_internal.h"

#pragma clang fp contract(off)

namespace {

// Lion (dense apply :682-703): c = b1 m + (1-b1) g; theta -= lr (sign(c) + wd theta); m = b2 m + (1-b2) g from the OLD m.
// sign as tf.math.sign: 0 for +-0 (returned as is: with wd = 0 such a theta does not move), NaN stays NaN.
__device__ __forceinline__ void lion_1(float& th, float g, float& m, const OptArgs& a) {
  const float c = m * a.b1 + g * (1.0f - a.b1);
  const float s = c > 0.f ? 1.f : (c < 0.f ? -1.f : c);
  th = th - a.lr * (s + th * a.wd);
  m = m * a.b2 + g * (1.0f - a.b2);
}

// AdaBelief (dense apply :456-530): m = b1 m + (1-b1) g; v = b2 v + (1-b2) (g - m)^2 + eps (the NEW m); amsgrad: vhat = max(vhat, v);
// u = r m^ / (sqrt(v'/bc2) + eps), or m^ below the rectification threshold (div = 0); u += wd theta (old theta) when wd != 0
template <bool AMS>
__device__ __forceinline__ void adab_1(float& th, float g, float& m, float& v, float& vh, const OptArgs& a) {
  const float mi = a.b1 * m + (1.0f - a.b1) * g;
  const float d = g - mi;
  const float vi = (a.b2 * v + (1.0f - a.b2) * (d * d)) + a.eps;
  m = mi; v = vi;
  float vv = vi;
  if (AMS) { vv = vh >= vi ? vh : vi; vh = vv; }
  const float mh = mi / a.bc1;
  float u = mh;
  if (a.div) u = (a.r * mh) / (sqrtf(vv / a.bc2) + a.eps);
  if (a.wd != 0.f) u = u + a.wd * th;
  th = th - a.lr * u;
}

// KIND = OPT_LION: slot m; OPT_ADABELIEF: m, v (+ vhat with AMS).  n4 = P / 4 when every buffer is 16-byte aligned, else 0 (all scalar)
template <int KIND, bool AMS>
__device__ __forceinline__ void opt_stream(float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, float* __restrict__ vh, long P, long n4, const OptArgs& a) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long q = tid; q < n4; q += stride) {
    f32x4 t4 = reinterpret_cast<const f32x4*>(theta)[q];
    const f32x4 g4 = reinterpret_cast<const f32x4*>(g)[q];
    f32x4 m4 = reinterpret_cast<const f32x4*>(m)[q];
    f32x4 v4 = {0.f, 0.f, 0.f, 0.f}, h4 = {0.f, 0.f, 0.f, 0.f};
    if (KIND == OPT_ADABELIEF) v4 = reinterpret_cast<const f32x4*>(v)[q];
    if (AMS) h4 = reinterpret_cast<const f32x4*>(vh)[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float tj = t4[j], mj = m4[j], vj = v4[j], hj = h4[j];
      if (KIND == OPT_LION) lion_1(tj, g4[j], mj, a);
      else adab_1<AMS>(tj, g4[j], mj, vj, hj, a);
      t4[j] = tj; m4[j] = mj; v4[j] = vj; h4[j] = hj;
    }
    reinterpret_cast<f32x4*>(theta)[q] = t4;
    reinterpret_cast<f32x4*>(m)[q] = m4;
    if (KIND == OPT_ADABELIEF) reinterpret_cast<f32x4*>(v)[q] = v4;
    if (AMS) reinterpret_cast<f32x4*>(vh)[q] = h4;
  }
  for (long i = 4 * n4 + tid; i < P; i += stride) {
    float tj = theta[i], mj = m[i], vj = 0.f, hj = 0.f;
    if (KIND == OPT_ADABELIEF) vj = v[i];
    if (AMS) hj = vh[i];
    if (KIND == OPT_LION) lion_1(tj, g[i], mj, a);
    else adab_1<AMS>(tj, g[i], mj, vj, hj, a);
    theta[i] = tj; m[i] = mj;
    if (KIND == OPT_ADABELIEF) v[i] = vj;
    if (AMS) vh[i] = hj;
  }
}

// k_reduce's body (k_misc.hip), shared by the fused forms: block = 64 columns x 8 row groups, four partial sums per thread, a fixed tree
// over the row groups -- the same order, so the same float.  Returns the column sum on row group 0 (and i < P).
__device__ __forceinline__ float reduce_col(const float* __restrict__ partial, long pstride, int rows, float (*red)[64], int col,
                                            int rg, long i, long P) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < P) {
    const float* p = partial + i;
    int rrow = rg;
    for (; rrow + 24 < rows; rrow += 32) {
      s0 += p[(long)rrow * pstride]; s1 += p[(long)(rrow + 8) * pstride];
      s2 += p[(long)(rrow + 16) * pstride]; s3 += p[(long)(rrow + 24) * pstride];
    }
    for (; rrow < rows; rrow += 8) s0 += p[(long)rrow * pstride];
  }
  red[rg][col] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  return ((red[0][col] + red[1][col]) + (red[2][col] + red[3][col])) + ((red[4][col] + red[5][col]) + (red[6][col] + red[7][col]));
}
// k_reduce's loss sum into g[P] (last block only, every thread of it)
__device__ __forceinline__ void reduce_loss(const float* __restrict__ lossp, int nloss, float (*red)[64], int col, int rg, float* gP) {
  __syncthreads();
  float ls = 0.f;
  for (int b = threadIdx.x; b < nloss; b += 512) ls += lossp[b];
  red[rg][col] = ls;
  __syncthreads();
  if (threadIdx.x < 64) {
    float vv = ((red[0][col] + red[1][col]) + (red[2][col] + red[3][col])) + ((red[4][col] + red[5][col]) + (red[6][col] + red[7][col]));
    for (int off = 32; off > 0; off >>= 1) vv += __shfl_down(vv, off);
    if (threadIdx.x == 0) *gP = vv;
  }
}

__device__ __forceinline__ OptArgs block_args(const OptDev* __restrict__ od) {
  __shared__ OptArgs sa;
  if (threadIdx.x == 0) {
    const OptDev o = *od;
    sa = opt_args(o, opt_scalars(o, o.step + 1));
  }
  __syncthreads();
  return sa;
}

}  // namespace

// ---- standalone updates -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lion(float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ m, long P,
                                              long n4, OptArgs a) {
  opt_stream<OPT_LION, false>(theta, g, m, nullptr, nullptr, P, n4, a);
}
template <bool AMS>
__global__ __launch_bounds__(256) void k_adabelief(float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, float* __restrict__ vh, long P, long n4, OptArgs a) {
  opt_stream<OPT_ADABELIEF, AMS>(theta, g, m, v, vh, P, n4, a);
}

// ---- device-state forms (captured graphs) -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lion_dev(float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ m, long P,
                                                  long n4, const OptDev* __restrict__ od) {
  const OptArgs a = block_args(od);
  opt_stream<OPT_LION, false>(theta, g, m, nullptr, nullptr, P, n4, a);
}
template <bool AMS>
__global__ __launch_bounds__(256) void k_adabelief_dev(float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, float* __restrict__ vh, long P, long n4,
                                                       const OptDev* __restrict__ od) {
  const OptArgs a = block_args(od);
  opt_stream<OPT_ADABELIEF, AMS>(theta, g, m, v, vh, P, n4, a);
}
__global__ void k_opt_step_inc(OptDev* od) { od->step += 1; }

// ---- fused tails: row reduction + update of the column -----------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_reduce_lion(const float* __restrict__ partial, long pstride, int rows,
                                                     const float* __restrict__ lossp, int nloss, float* __restrict__ g, long P,
                                                     float* __restrict__ theta, float* __restrict__ m, OptArgs a) {
  __shared__ float red[8][64];
  const int col = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + col;
  const float gi = reduce_col(partial, pstride, rows, red, col, rg, i, P);
  if (rg == 0 && i < P) {
    g[i] = gi;
    float th = theta[i], mi = m[i];
    lion_1(th, gi, mi, a);
    theta[i] = th; m[i] = mi;
  }
  if (blockIdx.x == gridDim.x - 1) reduce_loss(lossp, nloss, red, col, rg, g + P);
}
template <bool AMS>
__global__ __launch_bounds__(512) void k_reduce_adabelief(const float* __restrict__ partial, long pstride, int rows,
                                                          const float* __restrict__ lossp, int nloss, float* __restrict__ g, long P,
                                                          float* __restrict__ theta, float* __restrict__ m, float* __restrict__ v,
                                                          float* __restrict__ vh, OptArgs a) {
  __shared__ float red[8][64];
  const int col = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + col;
  const float gi = reduce_col(partial, pstride, rows, red, col, rg, i, P);
  if (rg == 0 && i < P) {
    g[i] = gi;
    float th = theta[i], mi = m[i], vi = v[i], hi = AMS ? vh[i] : 0.f;
    adab_1<AMS>(th, gi, mi, vi, hi, a);
    theta[i] = th; m[i] = mi; v[i] = vi;
    if (AMS) vh[i] = hi;
  }
  if (blockIdx.x == gridDim.x - 1) reduce_loss(lossp, nloss, red, col, rg, g + P);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
static bool al16(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }
// n4 and the grid of a stream over P parameters: at most 2048 blocks of 256 threads, the rest grid-strided
static void stream_shape(const float* theta, const float* g, const float* m, const float* v, const float* vh, long P, long* n4,
                         dim3* grid) {
  *n4 = (al16(theta) && al16(g) && al16(m) && al16(v) && al16(vh)) ? P / 4 : 0;
  const long work = *n4 > 0 ? *n4 : P;
  long blocks = (work + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  *grid = dim3((unsigned)blocks);
}

void launch_opt(int kind, bool ams, float* theta, const float* g, float* m, float* v, float* vhat, long P, const OptArgs& a,
                hipStream_t st) {
  long n4; dim3 grid;
  if (kind == OPT_LION) {
    stream_shape(theta, g, m, nullptr, nullptr, P, &n4, &grid);
    hipLaunchKernelGGL(k_lion, grid, dim3(256), 0, st, theta, g, m, P, n4, a);
  } else if (ams) {
    stream_shape(theta, g, m, v, vhat, P, &n4, &grid);
    hipLaunchKernelGGL(k_adabelief<true>, grid, dim3(256), 0, st, theta, g, m, v, vhat, P, n4, a);
  } else {
    stream_shape(theta, g, m, v, nullptr, P, &n4, &grid);
    hipLaunchKernelGGL(k_adabelief<false>, grid, dim3(256), 0, st, theta, g, m, v, (float*)nullptr, P, n4, a);
  }
}

void launch_reduce_opt(int kind, bool ams, const float* partial, long pstride, int rows, const float* loss_partial, int nloss, float* g,
                       long P, float* theta, float* m, float* v, float* vhat, const OptArgs& a, hipStream_t st) {
  dim3 grid((unsigned)((P + 63) / 64)), block(512);
  if (kind == OPT_LION)
    hipLaunchKernelGGL(k_reduce_lion, grid, block, 0, st, partial, pstride, rows, loss_partial, nloss, g, P, theta, m, a);
  else if (ams)
    hipLaunchKernelGGL(k_reduce_adabelief<true>, grid, block, 0, st, partial, pstride, rows, loss_partial, nloss, g, P, theta, m, v, vhat, a);
  else
    hipLaunchKernelGGL(k_reduce_adabelief<false>, grid, block, 0, st, partial, pstride, rows, loss_partial, nloss, g, P, theta, m, v,
                       (float*)nullptr, a);
}

void launch_opt_dev(int kind, bool ams, float* theta, const float* g, float* m, float* v, float* vhat, long P, OptDev* od,
                    hipStream_t st) {
  long n4; dim3 grid;
  if (kind == OPT_LION) {
    stream_shape(theta, g, m, nullptr, nullptr, P, &n4, &grid);
    hipLaunchKernelGGL(k_lion_dev, grid, dim3(256), 0, st, theta, g, m, P, n4, (const OptDev*)od);
  } else if (ams) {
    stream_shape(theta, g, m, v, vhat, P, &n4, &grid);
    hipLaunchKernelGGL(k_adabelief_dev<true>, grid, dim3(256), 0, st, theta, g, m, v, vhat, P, n4, (const OptDev*)od);
  } else {
    stream_shape(theta, g, m, v, nullptr, P, &n4, &grid);
    hipLaunchKernelGGL(k_adabelief_dev<false>, grid, dim3(256), 0, st, theta, g, m, v, (float*)nullptr, P, n4, (const OptDev*)od);
  }
  hipLaunchKernelGGL(k_opt_step_inc, dim3(1), dim3(1), 0, st, od);
}
