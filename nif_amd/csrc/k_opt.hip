// k_opt.hip -- the optimizer updates on the flat parameter vector (gfx950): Keras-2.11 Adam (SURVEY a-11), the reference's Lion and
// AdaBelief (nif/optimizers/external_optimizers.py:631-735, :322-628), Keras 2.11's SGD, RMSprop, Adagrad, Adamax, AdamW and amsgrad Adam
// (formulas restated from Keras 2.11, not pinned by TensorFlow), and the fixed-order row reduction of the gradient (k_reduce), which
// the fused forms share.  Three forms of each update, each one template over (kind, third slot: amsgrad's vhat / centered RMSprop's mean,
// weight average: Keras' use_ema behind the update in the same launch, +4 B read and +4 B written per parameter; ema_1):
//   * k_opt: the update alone over [0, P), behind an all-reduce, a regulariser or a flushed row reduction.  A stream bound by bandwidth:
//     Adam reads theta, g, m, v (16 B) and writes theta, m, v (12 B) per parameter; Lion 12 B / 8 B; AdaBelief as Adam, with amsgrad
//     20 B / 16 B; SGD and Adagrad 12 B / 8 B (slot 0 only), Adamax and RMSprop as Adam (centered RMSprop, amsgrad Adam and AdamW
//     20 B / 16 B).  Every kind but plain Adam four parameters per thread with 16-byte accesses where every buffer is 16-byte
//     aligned, a scalar tail for P % 4; plain Adam one parameter per thread (stream_shape).
//   * k_reduce_opt: k_reduce's row sum of column i (same summation order), g[i] and the loss g[P] still written, then the update of
//     column i behind its sum -- bit-identical to k_reduce followed by the standalone update.
//   * k_opt_dev: hyper-parameters and iteration count from device memory (OptDev) for captured graphs; each block forms the step's
//     scalars in fp64 (opt_scalars / opt_args, the host's own functions), k_opt_step_inc bumps the count behind the update.
// Every form runs the same per-element expressions (adam_1 / lion_1 / adab_1 / sgd_1 / rmsprop_1 / adagrad_1 / adamax_1 / adam_ams_1)
// with contraction off, so that the update is the same float sequence whichever form ran it; Adam's one fused multiply-add is written out.
#include "nif_internal.h"

#pragma clang fp contract(off)

namespace {

// Adam (Keras 2.11): m = m + (g - m)(1-b1); v = v + (g^2 - v)(1-b2) rounded once (fmaf); theta -= lr_t m / (sqrt(v) + eps), where
// a.lr = lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) (opt_args).  The roundings of Adam's earlier kernels, which had contraction on.
__device__ __forceinline__ void adam_1(float& th, float g, float& m, float& v, const OptArgs& a) {
  m = m + (g - m) * (1.0f - a.b1);
  v = fmaf(g * g - v, 1.0f - a.b2, v);
  th = th - a.lr * m / (sqrtf(v) + a.eps);
}

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

// Adam with amsgrad (Keras 2.11): adam_1's m and v, vhat = max(vhat, v), theta -= lr_t m / (sqrt(vhat) + eps)
__device__ __forceinline__ void adam_ams_1(float& th, float g, float& m, float& v, float& vh, const OptArgs& a) {
  m = m + (g - m) * (1.0f - a.b1);
  v = fmaf(g * g - v, 1.0f - a.b2, v);
  vh = vh >= v ? vh : v;
  th = th - a.lr * m / (sqrtf(vh) + a.eps);
}

// SGD (Keras 2.11): theta -= lr g; with momentum m = momentum m - lr g and theta += m, nesterov theta += momentum m - lr g (the new m)
__device__ __forceinline__ void sgd_1(float& th, float g, float& m, const OptArgs& a) {
  const float s = a.lr * g;
  if (a.div == 0) { th = th - s; return; }
  m = a.b1 * m - s;
  th = a.div == 2 ? th + (a.b1 * m - s) : th + m;
}

// RMSprop (Keras 2.11), slots v, mom, a: v = rho v + (1-rho) g^2; centered: a = rho a + (1-rho) g, d = v - a^2 + eps, else d = v + eps;
// inc = lr g / sqrt(d); with momentum mom = momentum mom + inc, theta -= mom, else theta -= inc
template <bool CENTERED>
__device__ __forceinline__ void rmsprop_1(float& th, float g, float& v, float& mom, float& av, const OptArgs& a) {
  v = a.b2 * v + (1.0f - a.b2) * (g * g);
  float d = v;
  if (CENTERED) { av = a.b2 * av + (1.0f - a.b2) * g; d = v - av * av; }
  d = d + a.eps;
  const float inc = a.lr * g / sqrtf(d);
  if (a.div) { mom = a.b1 * mom + inc; th = th - mom; }
  else th = th - inc;
}

// Adagrad (Keras 2.11): acc += g^2 (acc starts at initial_accumulator_value); theta -= lr g / sqrt(acc + eps)
__device__ __forceinline__ void adagrad_1(float& th, float g, float& acc, const OptArgs& a) {
  acc = acc + g * g;
  th = th - a.lr * g / sqrtf(acc + a.eps);
}

// Adamax (Keras 2.11): m += (g - m)(1-b1); u = max(b2 u, |g|); theta -= (lr / (1 - b1^t)) m / (u + eps)   (a.lr carries the correction)
__device__ __forceinline__ void adamax_1(float& th, float g, float& m, float& u, const OptArgs& a) {
  m = m + (g - m) * (1.0f - a.b1);
  u = fmaxf(a.b2 * u, fabsf(g));
  th = th - a.lr * m / (u + a.eps);
}

// the kinds with a second slot (Adam v, AdaBelief v, RMSprop mom, Adamax u); slot 0 is every kind's
template <int KIND> struct Slots { static constexpr bool second = KIND != OPT_LION && KIND != OPT_SGD && KIND != OPT_ADAGRAD; };

// Keras' use_ema behind the update of any kind (Keras 2.11, restated, not pinned by TensorFlow): average = momentum average +
// (1 - momentum) theta with the UPDATED theta; on an overwrite step (ema_overwrite) theta becomes the average
__device__ __forceinline__ void ema_1(float& th, float& av, const OptArgs& a) {
  av = a.ema_mom * av + (1.0f - a.ema_mom) * th;
  if (a.ema_ow) th = av;
}

// one parameter of any kind: slots (m, v, vh) are Adam / AdaBelief m, v, vhat; Lion, SGD m; RMSprop v, mom, a; Adagrad acc; Adamax m, u.
// AMS: the third slot is in use.  AdamW: theta -= lr wd theta with the step's learning rate (no bias correction), then Adam.
// EMA: av is the weight average, updated behind the kind's update (ema_1)
template <int KIND, bool AMS, bool EMA>
__device__ __forceinline__ void opt_1(float& th, float g, float& m, float& v, float& vh, float& av, const OptArgs& a) {
  if (KIND == OPT_ADAM && !AMS) adam_1(th, g, m, v, a);
  else if (KIND == OPT_ADAM) adam_ams_1(th, g, m, v, vh, a);
  else if (KIND == OPT_LION) lion_1(th, g, m, a);
  else if (KIND == OPT_ADABELIEF) adab_1<AMS>(th, g, m, v, vh, a);
  else if (KIND == OPT_SGD) sgd_1(th, g, m, a);
  else if (KIND == OPT_RMSPROP) rmsprop_1<AMS>(th, g, m, v, vh, a);
  else if (KIND == OPT_ADAGRAD) adagrad_1(th, g, m, a);
  else if (KIND == OPT_ADAMAX) adamax_1(th, g, m, v, a);
  else {
    th = th - a.lr0 * a.wd * th;
    if (AMS) adam_ams_1(th, g, m, v, vh, a);
    else adam_1(th, g, m, v, a);
  }
  if (EMA) ema_1(th, av, a);
}

// n4 = P / 4 when every buffer is 16-byte aligned, else 0 (all scalar)
template <int KIND, bool AMS, bool EMA>
__device__ __forceinline__ void opt_stream(float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, float* __restrict__ vh, float* __restrict__ ema, long P, long n4,
                                           const OptArgs& a) {
  constexpr bool S1 = Slots<KIND>::second;
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long q = tid; q < n4; q += stride) {
    f32x4 t4 = reinterpret_cast<const f32x4*>(theta)[q];
    const f32x4 g4 = reinterpret_cast<const f32x4*>(g)[q];
    f32x4 m4 = reinterpret_cast<const f32x4*>(m)[q];
    f32x4 v4 = {0.f, 0.f, 0.f, 0.f}, h4 = {0.f, 0.f, 0.f, 0.f}, e4 = {0.f, 0.f, 0.f, 0.f};
    if (S1) v4 = reinterpret_cast<const f32x4*>(v)[q];
    if (AMS) h4 = reinterpret_cast<const f32x4*>(vh)[q];
    if (EMA) e4 = reinterpret_cast<const f32x4*>(ema)[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float tj = t4[j], mj = m4[j], vj = v4[j], hj = h4[j], ej = e4[j];
      opt_1<KIND, AMS, EMA>(tj, g4[j], mj, vj, hj, ej, a);
      t4[j] = tj; m4[j] = mj; v4[j] = vj; h4[j] = hj; e4[j] = ej;
    }
    reinterpret_cast<f32x4*>(theta)[q] = t4;
    reinterpret_cast<f32x4*>(m)[q] = m4;
    if (S1) reinterpret_cast<f32x4*>(v)[q] = v4;
    if (AMS) reinterpret_cast<f32x4*>(vh)[q] = h4;
    if (EMA) reinterpret_cast<f32x4*>(ema)[q] = e4;
  }
  for (long i = 4 * n4 + tid; i < P; i += stride) {
    float tj = theta[i], mj = m[i], vj = 0.f, hj = 0.f, ej = 0.f;
    if (S1) vj = v[i];
    if (AMS) hj = vh[i];
    if (EMA) ej = ema[i];
    opt_1<KIND, AMS, EMA>(tj, g[i], mj, vj, hj, ej, a);
    theta[i] = tj; m[i] = mj;
    if (S1) v[i] = vj;
    if (AMS) vh[i] = hj;
    if (EMA) ema[i] = ej;
  }
}

// the row sum of k_reduce and the fused forms: block = 64 columns x 8 row groups, four independent partial sums per thread (a latency-
// bound stream of <= 256 rows: more loads in flight, not more bandwidth, is what it needs), a fixed tree over the row groups -- fixed
// order, so deterministic.  Returns the column sum on every row group (stored by row group 0, i < P).
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
// the loss partials into g[P] (last block only, every thread of it): a strided subset per thread in a fixed order, then a fixed tree
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

// the step's scalars from device memory, formed once per block.  od->kind is KIND (a graph is replayed only with the kind it recorded):
// stating it lets the compiler drop the other kinds' scalar code from the block's prologue.  EMA: whether this recorded step overwrites
// theta by the average is decided here, from the count the replay has reached
template <int KIND, bool EMA>
__device__ __forceinline__ OptArgs block_args(const OptDev* __restrict__ od) {
  __shared__ OptArgs sa;
  if (threadIdx.x == 0) {
    OptDev o = *od;
    o.kind = KIND == OPT_ADAMW ? OPT_ADAM : KIND;
    sa = opt_args(o, opt_scalars(o, o.step + 1));
    if (EMA) sa.ema_ow = ema_overwrite(o.step + 1, o.ema_freq) ? 1 : 0;
  }
  __syncthreads();
  return sa;
}

}  // namespace

// ---- gradient rows -> flat gradient (fixed summation order), loss partials -> g[P] ----------------------------------------------
__global__ __launch_bounds__(512) void k_reduce(const float* __restrict__ partial, long pstride, int rows,
                                                const float* __restrict__ lossp, int nloss, float* __restrict__ g, long P) {
  __shared__ float red[8][64];
  const int col = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + col;
  const float gi = reduce_col(partial, pstride, rows, red, col, rg, i, P);
  if (rg == 0 && i < P) g[i] = gi;
  if (blockIdx.x == gridDim.x - 1) reduce_loss(lossp, nloss, red, col, rg, g + P);
}

// ---- the three update forms -------------------------------------------------------------------------------------------------------
// (ema sits behind the arguments the EMA-off instantiations read: theirs keep their places)
template <int KIND, bool AMS, bool EMA>
__global__ __launch_bounds__(256) void k_opt(float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, float* __restrict__ vh, long P, long n4, OptArgs a,
                                             float* __restrict__ ema) {
  opt_stream<KIND, AMS, EMA>(theta, g, m, v, vh, ema, P, n4, a);
}
template <int KIND, bool AMS, bool EMA>
__global__ __launch_bounds__(256) void k_opt_dev(float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, float* __restrict__ vh, long P, long n4,
                                                 const OptDev* __restrict__ od, float* __restrict__ ema) {
  const OptArgs a = block_args<KIND, EMA>(od);
  opt_stream<KIND, AMS, EMA>(theta, g, m, v, vh, ema, P, n4, a);
}
__global__ void k_opt_step_inc(OptDev* od) { od->step += 1; }
template <int KIND, bool AMS, bool EMA>
__global__ __launch_bounds__(512) void k_reduce_opt(const float* __restrict__ partial, long pstride, int rows,
                                                    const float* __restrict__ lossp, int nloss, float* __restrict__ g, long P,
                                                    float* __restrict__ theta, float* __restrict__ m, float* __restrict__ v,
                                                    float* __restrict__ vh, OptArgs a, float* __restrict__ ema) {
  __shared__ float red[8][64];
  const int col = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + col;
  const float gi = reduce_col(partial, pstride, rows, red, col, rg, i, P);
  if (rg == 0 && i < P) {
    g[i] = gi;
    float th = theta[i], mi = m[i], vi = Slots<KIND>::second ? v[i] : 0.f, hi = AMS ? vh[i] : 0.f, ei = EMA ? ema[i] : 0.f;
    opt_1<KIND, AMS, EMA>(th, gi, mi, vi, hi, ei, a);
    theta[i] = th; m[i] = mi;
    if (Slots<KIND>::second) v[i] = vi;
    if (AMS) vh[i] = hi;
    if (EMA) ema[i] = ei;
  }
  if (blockIdx.x == gridDim.x - 1) reduce_loss(lossp, nloss, red, col, rg, g + P);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
void launch_reduce(const float* partial, long pstride, int rows, const float* loss_partial, int nloss, float* g, long P,
                   hipStream_t st) {
  hipLaunchKernelGGL(k_reduce, dim3((unsigned)((P + 63) / 64)), dim3(512), 0, st, partial, pstride, rows, loss_partial, nloss, g, P);
}

static bool al16(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }
// n4 and the grid of a stream over P parameters (v, vh: nullptr where the kind does not use them): at most 2048 blocks of 256 threads,
// the rest grid-strided.  Adam without amsgrad runs one parameter per thread (n4 = 0), the shape of its earlier kernels: four per thread
// serialise four divisions and square roots, and made the captured configs[0] step (P = 6 627, 7 blocks instead of 26) 0.5 us slower
static void stream_shape(int kind, const float* theta, const float* g, const float* m, const float* v, const float* vh,
                         const float* ema, long P, long* n4, dim3* grid) {
  *n4 = (!(kind == OPT_ADAM && vh == nullptr) && al16(theta) && al16(g) && al16(m) && al16(v) && al16(vh) && al16(ema)) ? P / 4 : 0;
  const long work = *n4 > 0 ? *n4 : P;
  long blocks = (work + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  *grid = dim3((unsigned)blocks);
}

// the instantiation of (kernel kind, third slot, weight average): X(KIND, AMS, EMA) is expanded with compile-time arguments
#define OPT_DISPATCH_E(kind, ams, E, X)                                                     \
  switch (kind) {                                                                           \
    case OPT_ADAM: if (ams) { X(OPT_ADAM, true, E); } else { X(OPT_ADAM, false, E); } break; \
    case OPT_LION: X(OPT_LION, false, E); break;                                            \
    case OPT_ADABELIEF: if (ams) { X(OPT_ADABELIEF, true, E); } else { X(OPT_ADABELIEF, false, E); } break; \
    case OPT_SGD: X(OPT_SGD, false, E); break;                                              \
    case OPT_RMSPROP: if (ams) { X(OPT_RMSPROP, true, E); } else { X(OPT_RMSPROP, false, E); } break; \
    case OPT_ADAGRAD: X(OPT_ADAGRAD, false, E); break;                                      \
    case OPT_ADAMAX: X(OPT_ADAMAX, false, E); break;                                        \
    default: if (ams) { X(OPT_ADAMW, true, E); } else { X(OPT_ADAMW, false, E); } break;     \
  }
#define OPT_DISPATCH(kind, ams, ema, X) \
  if (ema) { OPT_DISPATCH_E(kind, ams, true, X) } else { OPT_DISPATCH_E(kind, ams, false, X) }
static bool second_slot(int kind) { return kind != OPT_LION && kind != OPT_SGD && kind != OPT_ADAGRAD; }

// kind: the kernel kind (kernel_kind: OPT_* with OPT_ADAMW), ams: the third slot is in use (third_slot).  The slots a kind does not use
// are not touched (may be null).  ema: the weight average (P floats), null = off
void launch_opt(int kind, bool ams, float* theta, const float* g, float* m, float* v, float* vhat, float* ema, long P, const OptArgs& a,
                hipStream_t st) {
  if (!second_slot(kind)) v = nullptr;
  if (!ams) vhat = nullptr;
  long n4; dim3 grid;
  stream_shape(kind, theta, g, m, v, vhat, ema, P, &n4, &grid);
#define X(K, A, E) hipLaunchKernelGGL((k_opt<K, A, E>), grid, dim3(256), 0, st, theta, g, m, v, vhat, P, n4, a, ema)
  OPT_DISPATCH(kind, ams, ema != nullptr, X)
#undef X
}

void launch_reduce_opt(int kind, bool ams, const float* partial, long pstride, int rows, const float* loss_partial, int nloss, float* g,
                       long P, float* theta, float* m, float* v, float* vhat, float* ema, const OptArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((P + 63) / 64)), block(512);
#define X(K, A, E)                                                                                                                   \
  hipLaunchKernelGGL((k_reduce_opt<K, A, E>), grid, block, 0, st, partial, pstride, rows, loss_partial, nloss, g, P, theta, m, v, vhat, \
                     a, ema)
  OPT_DISPATCH(kind, ams, ema != nullptr, X)
#undef X
}

void launch_opt_dev(int kind, bool ams, float* theta, const float* g, float* m, float* v, float* vhat, float* ema, long P, OptDev* od,
                    hipStream_t st) {
  if (!second_slot(kind)) v = nullptr;
  if (!ams) vhat = nullptr;
  long n4; dim3 grid;
  stream_shape(kind, theta, g, m, v, vhat, ema, P, &n4, &grid);
  const OptDev* o = od;
#define X(K, A, E) hipLaunchKernelGGL((k_opt_dev<K, A, E>), grid, dim3(256), 0, st, theta, g, m, v, vhat, P, n4, o, ema)
  OPT_DISPATCH(kind, ams, ema != nullptr, X)
#undef X
  hipLaunchKernelGGL(k_opt_step_inc, dim3(1), dim3(1), 0, st, od);
}
