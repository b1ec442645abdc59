// k_f64.hip -- the L-BFGS closure in double precision (include/nif_hip.h nif_f64_*; reference nif/optimizers/lbfgs.py:56-88,
// lbfgs_V2.py:57-79, whose fine-tuner switches Keras to float64).  Forward pass, loss and the gradient with respect to every parameter
// of class NIF and NIFMultiScale, all in `double`, on a float64 master copy of the parameters that lives next to the float32 model.
// This is a precision of the fine-tuner, not Keras' float64 policy: fit(), predict() and every other entry point stay float32.
//
// Plane formulation: h . W(p) = sum_k zt_k (h . M_k), zt = (z_1 .. z_r, 1); the [B, po] hypernetwork output never exists.
//
// BOUNDED WORKSPACE: the batch is walked in chunks of F64_CHUNK = 4096 points.  Every tape (layer inputs, pre-activations, dL/da) is a
// [row][F64_CHUNK] double array that is reused by the next chunk, so the workspace does not grow with B.
// DETERMINISTIC: no floating-point atomics.  Inside a chunk the K = batch weight-gradient sums are split into `S` fixed point segments
// whose partial rows are added in segment order; the chunks' sums are added to [grad | loss] in chunk order (kernels of one stream).
//
// Kernels, per chunk (runtime dimensions, one generic family; feature counts are padded to the 16 x 16 MFMA tile by zero operands):
//   k64_pnet_fwd / k64_pnet_bwd   ParameterNet and its reverse sweep, one thread per point, plain FMAs
//   k64_snet_first / k64_snet_last / k64_act_back   first and last ShapeNet layer (1-16 inputs / outputs), loss, dL/da: plain FMAs
//   k64_hidden_fwd / k64_hidden_bwd   the hidden n x n products, forward and in the adjoint, on v_mfma_f64_16x16x4_f64
//   k64_wgrad                         every weight / bias gradient, dM_k += sum_b zt_k[b] h[b] (x) ga[b], as GEMMs with K = batch on the
//                                     same MFMA (one launch over a job table)
//   k64_reduce / k64_loss_reduce      segment rows and per-point losses into [grad | loss], fixed order
// v_mfma_f64_16x16x4_f64 operand maps: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15], one double per lane;
// C/D: col = lane & 15, row = (lane >> 4) + 4 reg.  Here D rows are features and D columns are points, so per-point scalars (zt_k) are
// per-lane values and every tape row is read and written as 16 consecutive doubles.
// Transcendentals are the device library's double sin / cos / exp / tanh / erf / log1p / expm1.
#include "nif_ctx.h"
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#define F64_CHUNK 4096      // points per chunk
#define F64_SEGS 8          // point segments of a chunk in the weight-gradient sums (fewer for very large parameter vectors)
static const long CH = F64_CHUNK;

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct F64Args {
  const double* theta;
  const double* xin; int ncol;
  int Bc, Bp;                       // points of this chunk, and padded to a multiple of 16
  int pi, nst, lst, r, p_act, p_res; double p_om;
  long first_w, first_b, hid_w[NIF_MAX_HID], hid_b[NIF_MAX_HID], hid_w2[NIF_MAX_HID], hid_b2[NIF_MAX_HID], bott_w, bott_b, last_w, last_b;
  int si, so, n, nh, s_act, s_res, nif_skip; double s_om; long po;
  int loss_kind; const double* y; const double* sw; double inv_bg; double* u_out;
  // tapes, [row][F64_CHUNK]
  double *PP, *PA0, *PH, *PA1, *PT, *PA2, *PGA0, *PGA1, *PGA2, *PGH;
  double *ZT, *GZT, *GZTP, *X, *A0, *H, *A, *GA0, *GA, *GU, *GH, *LOSSP;
};
struct F64Job { const double* IN; const double* DA; const double* ZT; int nin, nout, K, wave0; MatRef W; double scale; };

struct NifF64 {
  DevBuf<double> theta, g, stash, part;
  DevBuf<F64Job> jobs; int njobs = 0, job_waves = 0;
  int S = F64_SEGS, seglen = F64_CHUNK / F64_SEGS; long pstride = 0;
  bool have_params = false, have_grad = false;
  F64Args a;
};

__host__ __device__ inline long f64_w1(const F64Args& a) { return 0; }
__host__ __device__ inline long f64_wh(const F64Args& a, int j) { return (long)a.si * a.n + (long)j * a.n * a.n; }
__host__ __device__ inline long f64_wl(const F64Args& a) { return (long)a.si * a.n + (long)a.nh * a.n * a.n; }
__host__ __device__ inline long f64_b1(const F64Args& a) { return f64_wl(a) + (long)a.n * a.so; }
__host__ __device__ inline long f64_bh(const F64Args& a, int j) { return f64_b1(a) + a.n + (long)j * a.n; }
__host__ __device__ inline long f64_bl(const F64Args& a) { return f64_b1(a) + a.n + (long)a.nh * a.n; }
// plane k of the hypernetwork's affine map at pnet_output offset `off`: row k of the hyper kernel, k = r: the hyper bias
__device__ __forceinline__ const double* f64_plane(const F64Args& a, int k) {
  return a.theta + (k < a.r ? a.last_w + (long)k * a.po : a.last_b);
}

// h = f(a), d = f'(a) for the Keras activation ids of nif_internal.h
__device__ __forceinline__ void act64(int act, double a, double* h, double* d) {
  switch (act) {
    case ACT_SINE: *h = sin(a); *d = cos(a); break;
    case ACT_SWISH: { const double s = 1.0 / (1.0 + exp(-a)); *h = a * s; *d = s * (1.0 + a * (1.0 - s)); } break;
    case ACT_TANH: { const double t = tanh(a); *h = t; *d = 1.0 - t * t; } break;
    case ACT_RELU: *h = a > 0.0 ? a : 0.0; *d = a > 0.0 ? 1.0 : 0.0; break;
    case ACT_SIGMOID: { const double s = 1.0 / (1.0 + exp(-a)); *h = s; *d = s * (1.0 - s); } break;
    case ACT_ELU: *h = a > 0.0 ? a : expm1(fmin(a, 0.0)); *d = a > 0.0 ? 1.0 : exp(fmin(a, 0.0)); break;
    case ACT_SOFTPLUS: *h = fmax(a, 0.0) + log1p(exp(-fabs(a))); *d = 1.0 / (1.0 + exp(-a)); break;
    case ACT_GELU: {
      const double cdf = 0.5 * (1.0 + erf(a * 0.70710678118654752440));
      *h = a * cdf; *d = cdf + a * 0.39894228040143267794 * exp(-0.5 * a * a);
    } break;
    case ACT_SELU: {
      const double al = 1.6732632423543772, sc = 1.0507009873554805;
      *h = sc * (a > 0.0 ? a : al * expm1(fmin(a, 0.0))); *d = sc * (a > 0.0 ? 1.0 : al * exp(fmin(a, 0.0)));
    } break;
    case ACT_SOFTSIGN: { const double q = 1.0 / (1.0 + fabs(a)); *h = a * q; *d = q * q; } break;
    case ACT_EXPONENTIAL: { const double e = exp(a); *h = e; *d = e; } break;
    case ACT_HARD_SIGMOID: { const double t = 0.2 * a + 0.5; *h = fmin(fmax(t, 0.0), 1.0); *d = (t > 0.0 && t < 1.0) ? 0.2 : 0.0; } break;
    default: *h = a; *d = 1.0; break;
  }
}
// per-element Keras regression loss of e = prediction - target: value and derivative
__device__ __forceinline__ void loss64(int kind, double e, double* v, double* d) {
  if (kind == NIF_LOSS_MAE) { *v = fabs(e); *d = e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0); }
  else if (kind == NIF_LOSS_HUBER) { const double a = fabs(e); *v = a <= 1.0 ? 0.5 * e * e : a - 0.5; *d = fmin(fmax(e, -1.0), 1.0); }
  else if (kind == NIF_LOSS_LOGCOSH) { const double a = fabs(e); *v = a + log1p(exp(-2.0 * a)) - 0.69314718055994530942; *d = tanh(e); }
  else { *v = e * e; *d = 2.0 * e; }
}

// ---- ParameterNet, one thread per point -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k64_pnet_fwd(F64Args A) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= A.Bp) return;
  const double* th = A.theta;
  const int nst = A.nst;
  const bool real = b < A.Bc;
  for (int d = 0; d < A.pi; ++d) A.PP[d * CH + b] = real ? A.xin[(long)b * A.ncol + d] : 0.0;
  for (int d = 0; d < A.si; ++d) A.X[d * CH + b] = real ? A.xin[(long)b * A.ncol + A.pi + d] : 0.0;
  for (int j = 0; j < nst; ++j) {
    double s = 0.0;
    for (int d = 0; d < A.pi; ++d) s = fma(A.PP[d * CH + b], th[A.first_w + (long)d * nst + j], s);
    const double a = A.p_om * s + th[A.first_b + j];
    double h, dd; act64(A.p_act, a, &h, &dd);
    A.PA0[j * CH + b] = a; A.PH[j * CH + b] = h;
  }
  for (int l = 0; l < A.lst; ++l) {
    const double* hin = A.PH + (long)l * nst * CH;
    double* hout = A.PH + (long)(l + 1) * nst * CH;
    double* a1r = A.PA1 + (long)l * nst * CH;
    double* tr = A.PT + (long)l * nst * CH;
    double* a2r = A.PA2 + (long)l * nst * CH;
    const double* W = th + A.hid_w[l]; const double* bv = th + A.hid_b[l];
    for (int j = 0; j < nst; ++j) {
      double s = 0.0;
      for (int i = 0; i < nst; ++i) s = fma(hin[i * CH + b], W[(long)i * nst + j], s);
      const double a1 = A.p_om * s + bv[j];
      double h, dd; act64(A.p_act, a1, &h, &dd);
      a1r[j * CH + b] = a1;
      if (A.p_res) tr[j * CH + b] = h;
      else hout[j * CH + b] = A.p_act == ACT_SINE ? h : hin[j * CH + b] + h;       // SIREN: sin(a); MLP_SimpleShortCut: x + act(a)
    }
    if (A.p_res) {
      const double* W2 = th + A.hid_w2[l]; const double* b2 = th + A.hid_b2[l];
      for (int j = 0; j < nst; ++j) {
        double s = 0.0;
        for (int i = 0; i < nst; ++i) s = fma(tr[i * CH + b], W2[(long)i * nst + j], s);
        double a2, h, dd;
        if (A.p_act == ACT_SINE) { a2 = A.p_om * s + b2[j]; act64(ACT_SINE, a2, &h, &dd); hout[j * CH + b] = 0.5 * (hin[j * CH + b] + h); }   // SIREN_ResNet
        else { a2 = hin[j * CH + b] + (s + b2[j]); act64(A.p_act, a2, &h, &dd); hout[j * CH + b] = h; }                                      // MLP_ResNet
        a2r[j * CH + b] = a2;
      }
    }
  }
  const double* hL = A.PH + (long)A.lst * nst * CH;
  for (int c = 0; c < A.r; ++c) {
    double s = 0.0;
    for (int i = 0; i < nst; ++i) s = fma(hL[i * CH + b], th[A.bott_w + (long)i * A.r + c], s);
    A.ZT[c * CH + b] = s + th[A.bott_b + c];
  }
  A.ZT[A.r * CH + b] = 1.0;
}

__global__ __launch_bounds__(64) void k64_pnet_bwd(F64Args A) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= A.Bc) return;
  const double* th = A.theta;
  const int nst = A.nst;
  const bool siren = A.p_act == ACT_SINE;
  double* gh = A.PGH; double* gn = A.PGH + (long)nst * CH;
  for (int i = 0; i < nst; ++i) {
    double s = 0.0;
    for (int c = 0; c < A.r; ++c) s = fma(A.GZT[c * CH + b], th[A.bott_w + (long)i * A.r + c], s);
    gh[i * CH + b] = s;
  }
  for (int l = A.lst - 1; l >= 0; --l) {
    const double* a1r = A.PA1 + (long)l * nst * CH;
    const double* a2r = A.PA2 + (long)l * nst * CH;
    double* ga1 = A.PGA1 + (long)l * nst * CH;
    double* ga2 = A.PGA2 + (long)l * nst * CH;
    const double* W = th + A.hid_w[l];
    if (A.p_res) {
      const double* W2 = th + A.hid_w2[l];
      for (int j = 0; j < nst; ++j) {
        double h, dd; act64(A.p_act, a2r[j * CH + b], &h, &dd);
        ga2[j * CH + b] = (siren ? 0.5 : 1.0) * gh[j * CH + b] * dd;
      }
      for (int i = 0; i < nst; ++i) {
        double s = 0.0;
        for (int j = 0; j < nst; ++j) s = fma(ga2[j * CH + b], W2[(long)i * nst + j], s);
        double h, dd; act64(A.p_act, a1r[i * CH + b], &h, &dd);
        ga1[i * CH + b] = A.p_om * s * dd;
      }
      for (int i = 0; i < nst; ++i) {
        double s = 0.0;
        for (int j = 0; j < nst; ++j) s = fma(ga1[j * CH + b], W[(long)i * nst + j], s);
        gn[i * CH + b] = siren ? 0.5 * gh[i * CH + b] + A.p_om * s : ga2[i * CH + b] + s;
      }
    } else {
      for (int j = 0; j < nst; ++j) {
        double h, dd; act64(A.p_act, a1r[j * CH + b], &h, &dd);
        ga1[j * CH + b] = gh[j * CH + b] * dd;
      }
      for (int i = 0; i < nst; ++i) {
        double s = 0.0;
        for (int j = 0; j < nst; ++j) s = fma(ga1[j * CH + b], W[(long)i * nst + j], s);
        gn[i * CH + b] = siren ? A.p_om * s : gh[i * CH + b] + s;
      }
    }
    double* t = gh; gh = gn; gn = t;
  }
  for (int j = 0; j < nst; ++j) {
    double h, dd; act64(A.p_act, A.PA0[j * CH + b], &h, &dd);
    A.PGA0[j * CH + b] = gh[j * CH + b] * dd;
  }
}

// ---- ShapeNet: first layer, last layer + loss, dL/da ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k64_snet_first(F64Args A) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= A.Bp) return;
  const int n = A.n, K = A.r + 1;
  const long w1 = f64_w1(A), b1 = f64_b1(A);
  for (int j = 0; j < n; ++j) {
    double s = 0.0, bias = 0.0;
    for (int k = 0; k < K; ++k) {
      const double* Mk = f64_plane(A, k);
      const double zt = A.ZT[k * CH + b];
      double t = 0.0;
      for (int d = 0; d < A.si; ++d) t = fma(A.X[d * CH + b], Mk[w1 + (long)d * n + j], t);
      s = fma(zt, t, s);
      bias = fma(zt, Mk[b1 + j], bias);
    }
    const double a0 = A.s_om * s + bias;
    double h, dd; act64(A.s_act, a0, &h, &dd);
    A.A0[j * CH + b] = a0; A.H[j * CH + b] = h;
  }
}

// out = u . W_l + b_l, loss, dL/du, and (training) the last layer's data adjoint: dL/dh -> GH buffer 0, dL/dzt -> GZT
__global__ __launch_bounds__(64) void k64_snet_last(F64Args A) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= A.Bp) return;
  const int n = A.n, K = A.r + 1, so = A.so;
  const bool real = b < A.Bc;
  const long wl = f64_wl(A), bl = f64_bl(A);
  const double* u = A.H + (long)A.nh * n * CH;
  const double w = (real && A.sw) ? A.sw[b] : 1.0;
  double per = 0.0;
  for (int s = 0; s < so; ++s) {
    double acc = 0.0, bias = 0.0;
    for (int k = 0; k < K; ++k) {
      const double* Mk = f64_plane(A, k);
      const double zt = A.ZT[k * CH + b];
      double t = 0.0;
      for (int i = 0; i < n; ++i) t = fma(u[i * CH + b], Mk[wl + (long)i * so + s], t);
      acc = fma(zt, t, acc);
      bias = fma(zt, Mk[bl + s], bias);
    }
    const double out = acc + bias;
    if (A.u_out && real) A.u_out[(long)b * so + s] = out;
    if (A.y) {
      double v = 0.0, d = 0.0;
      if (real) loss64(A.loss_kind, out - A.y[(long)b * so + s], &v, &d);
      per += v;
      A.GU[s * CH + b] = real ? d * w * A.inv_bg / (double)so : 0.0;
    }
  }
  if (!A.y) return;
  A.LOSSP[b] = real ? (per / (double)so) * w * A.inv_bg : 0.0;
  for (int i = 0; i < n; ++i) A.GH[i * CH + b] = 0.0;
  for (int k = 0; k < K; ++k) {
    const double* Mk = f64_plane(A, k);
    const double zt = A.ZT[k * CH + b];
    double gz = 0.0;
    for (int s = 0; s < so; ++s) gz = fma(A.GU[s * CH + b], Mk[bl + s], gz);
    for (int i = 0; i < n; ++i) {
      double t = 0.0;
      for (int s = 0; s < so; ++s) t = fma(A.GU[s * CH + b], Mk[wl + (long)i * so + s], t);
      A.GH[i * CH + b] = fma(zt, t, A.GH[i * CH + b]);
      gz = fma(u[i * CH + b], t, gz);
    }
    A.GZT[k * CH + b] = gz;
  }
}

// dL/da of hidden matrix m (m = -1: the first layer) = scale * dL/dh * f'(a); dL/dzt gets the partial rows of the hidden adjoint that
// ran before (npart tiles), the bias planes' term, and for the first layer the term through its matrix
__global__ __launch_bounds__(64) void k64_act_back(F64Args A, int m, const double* GHin, double scale, int npart) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= A.Bp) return;
  const int n = A.n, K = A.r + 1;
  const double* ar = m < 0 ? A.A0 : A.A + (long)m * n * CH;
  double* ga = m < 0 ? A.GA0 : A.GA + (long)m * n * CH;
  const long boff = m < 0 ? f64_b1(A) : f64_bh(A, m);
  for (int j = 0; j < n; ++j) {
    double h, dd; act64(A.s_act, ar[j * CH + b], &h, &dd);
    ga[j * CH + b] = scale * GHin[j * CH + b] * dd;
  }
  for (int k = 0; k < K; ++k) {
    const double* Mk = f64_plane(A, k);
    double s = A.GZT[k * CH + b];
    for (int t = 0; t < npart; ++t) s += A.GZTP[((long)t * K + k) * CH + b];
    for (int j = 0; j < n; ++j) s = fma(ga[j * CH + b], Mk[boff + j], s);
    if (m < 0) {
      const long w1 = f64_w1(A);
      double q = 0.0;
      for (int d = 0; d < A.si; ++d) {
        double t = 0.0;
        for (int j = 0; j < n; ++j) t = fma(ga[j * CH + b], Mk[w1 + (long)d * n + j], t);
        q = fma(A.X[d * CH + b], t, q);
      }
      s = fma(A.s_om, q, s);
    }
    A.GZT[k * CH + b] = s;
  }
}

// ---- hidden n x n products on v_mfma_f64_16x16x4_f64: one wave per (16 points, 16 features) tile -------------------------------------
// a[j][b] = om sum_{k,i} M_k[i][j] (zt_k[b] h_in[i][b]) + sum_k zt_k[b] bias_k[j];  H[m+1] = c1 f(a) + c2 RES
__global__ __launch_bounds__(256) void k64_hidden_fwd(F64Args A, int m, double c1, double c2, const double* RES) {
  const int lane = threadIdx.x & 63, wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n = A.n, njt = (n + 15) >> 4;
  const int pt = wv / njt, jt = wv - pt * njt;
  if (pt * 16 >= A.Bp) return;
  const int c = lane & 15, q = lane >> 4;
  const int b = pt * 16 + c, jA = jt * 16 + c;
  const double* hin = A.H + (long)m * n * CH;
  const long slot = f64_wh(A, m);
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k <= A.r; ++k) {
    const double ztk = A.ZT[k * CH + b];
    const double* Wk = f64_plane(A, k) + slot;
    for (int i0 = 0; i0 < n; i0 += 4) {
      const int i = i0 + q;
      const bool ok = i < n;
      const double av = (ok && jA < n) ? Wk[(long)i * n + jA] : 0.0;
      const double bv = ok ? ztk * hin[(long)i * CH + b] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
  }
  const long boff = f64_bh(A, m);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int j = jt * 16 + q + 4 * reg;
    if (j < n) {
      double bias = 0.0;
      for (int k = 0; k <= A.r; ++k) bias = fma(A.ZT[k * CH + b], f64_plane(A, k)[boff + j], bias);
      const double a = A.s_om * acc[reg] + bias;
      double h, dd; act64(A.s_act, a, &h, &dd);
      A.A[((long)m * n + j) * CH + b] = a;
      A.H[((long)(m + 1) * n + j) * CH + b] = c1 * h + (RES ? c2 * RES[(long)j * CH + b] : 0.0);
    }
  }
}

// U_k[i][b] = sum_j M_k[i][j] ga[j][b] per plane;  GHout = om sum_k zt_k U_k + cres GHres;  GZTP[it][k][b] = om sum_{i in tile} h_in[i][b] U_k[i][b]
__global__ __launch_bounds__(256) void k64_hidden_bwd(F64Args A, int m, const double* GHres, double cres, double* GHout) {
  const int lane = threadIdx.x & 63, wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n = A.n, nit = (n + 15) >> 4, K = A.r + 1;
  const int pt = wv / nit, it = wv - pt * nit;
  if (pt * 16 >= A.Bp) return;
  const int c = lane & 15, q = lane >> 4;
  const int b = pt * 16 + c, iA = it * 16 + c;
  const double* hin = A.H + (long)m * n * CH;
  const double* ga = A.GA + (long)m * n * CH;
  const long slot = f64_wh(A, m);
  f64x4 gacc = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < K; ++k) {
    const double* Wk = f64_plane(A, k) + slot;
    f64x4 U = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < n; j0 += 4) {
      const int j = j0 + q;
      const bool ok = j < n;
      const double av = (ok && iA < n) ? Wk[(long)iA * n + j] : 0.0;
      const double bv = ok ? ga[(long)j * CH + b] : 0.0;
      U = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, U, 0, 0, 0);
    }
    const double ztk = A.ZT[k * CH + b];
    double s = 0.0;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = it * 16 + q + 4 * reg;
      if (i < n) s = fma(hin[(long)i * CH + b], U[reg], s);
      gacc[reg] = fma(ztk, U[reg], gacc[reg]);
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (q == 0) A.GZTP[((long)it * K + k) * CH + b] = A.s_om * s;
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int i = it * 16 + q + 4 * reg;
    if (i < n) GHout[(long)i * CH + b] = A.s_om * gacc[reg] + (GHres ? cres * GHres[(long)i * CH + b] : 0.0);
  }
}

// ---- every weight / bias gradient of a chunk: D[i][j] = scale sum_b (zt_k[b] IN[i][b]) DA[j][b], K = batch ---------------------------
// one wave per (segment, plane, 16 x 16 tile) of a job; IN == null: ones (bias rows); ZT == null: dense matrix.  Writes its tile of the
// segment's partial row (every parameter belongs to exactly one job, so every row is fully rewritten by every launch)
__global__ __launch_bounds__(256) void k64_wgrad(const F64Job* __restrict__ jobs, int njobs, int waves_per_seg, double* part, long pstride,
                                                  int S, int seglen, int Bc) {
  const int lane = threadIdx.x & 63, wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= waves_per_seg * S) return;
  const int seg = wv / waves_per_seg;
  int w = wv - seg * waves_per_seg;
  int ji = 0;
  while (ji + 1 < njobs && jobs[ji + 1].wave0 <= w) ++ji;
  const F64Job J = jobs[ji];
  w -= J.wave0;
  const int nit = (J.nin + 15) >> 4, njt = (J.nout + 15) >> 4;
  const int k = w / (nit * njt); w -= k * nit * njt;
  const int it = w / njt, jt = w - it * njt;
  const int c = lane & 15, q = lane >> 4;
  const int iA = it * 16 + c, jB = jt * 16 + c;
  const int b_lo = seg * seglen;
  int b_hi = b_lo + seglen; if (b_hi > Bc) b_hi = Bc;
  const double* zt = J.ZT ? J.ZT + (long)k * CH : nullptr;
  const double* in = (J.IN && iA < J.nin) ? J.IN + (long)iA * CH : nullptr;
  const double* da = J.DA + (long)(jB < J.nout ? jB : 0) * CH;
  const bool okA = iA < J.nin, okB = jB < J.nout;
  f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  for (int b0 = b_lo; b0 < b_hi; b0 += 8) {
    const int ba = b0 + q, bb = b0 + 4 + q;
    const bool oa = ba < b_hi, ob = bb < b_hi;
    const double av0 = (oa && okA) ? (in ? in[ba] : 1.0) * (zt ? zt[ba] : 1.0) : 0.0;
    const double bv0 = (oa && okB) ? da[ba] : 0.0;
    const double av1 = (ob && okA) ? (in ? in[bb] : 1.0) * (zt ? zt[bb] : 1.0) : 0.0;
    const double bv1 = (ob && okB) ? da[bb] : 0.0;
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av0, bv0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av1, bv1, acc1, 0, 0, 0);
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int i = it * 16 + q + 4 * reg;
    if (i < J.nin && okB) part[(long)seg * pstride + matref_index(J.W, k, i, jB)] = J.scale * (acc0[reg] + acc1[reg]);
  }
}

__global__ __launch_bounds__(256) void k64_reduce(const double* __restrict__ part, long pstride, int S, double* g, long P) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P) return;
  double s = 0.0;
  for (int t = 0; t < S; ++t) s += part[(long)t * pstride + idx];
  g[idx] += s;
}
__global__ __launch_bounds__(256) void k64_loss_reduce(const double* __restrict__ lossp, int Bc, double* gl) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int b = threadIdx.x; b < Bc; b += 256) s += lossp[b];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *gl += sh[0];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static int f64_supported(nif_ctx* c, const char* who) {
  if (c->kind == NIF_KIND_LASTLAYER)
    return fail(NIF_ERR_INVALID, std::string(who) + ": the double-precision path is built for class NIF and NIFMultiScale, not for NIFMultiScaleLastLayerParameterized");
  if (c->cfg.mixed_policy != NIF_POLICY_FLOAT32)
    return fail(NIF_ERR_INVALID, std::string(who) + ": the double-precision path is built for models of policy float32, not for a mixed policy");
  if (c->capturing) return fail(NIF_ERR_STATE, std::string(who) + ": not capturable (inside nif_graph_begin / nif_graph_end)");
  return NIF_OK;
}

static void f64_add_job(std::vector<F64Job>& jobs, int& waves, const double* IN, const double* DA, const double* ZT, int nin, int nout,
                        int K, const MatRef& W, double scale) {
  F64Job j; memset(&j, 0, sizeof(j));
  j.IN = IN; j.DA = DA; j.ZT = ZT; j.nin = nin; j.nout = nout; j.K = K; j.W = W; j.scale = scale; j.wave0 = waves;
  waves += K * ((nin + 15) / 16) * ((nout + 15) / 16);
  jobs.push_back(j);
}
static MatRef f64_dense(long off, int nin, int nout) { MatRef m; m.r = 0; m.base_k = 0; m.kstride = 0; m.base_last = off; m.ld = nout; m.nin = nin; m.nout = nout; return m; }
static MatRef f64_vec(long off, int nout) { MatRef m = f64_dense(off, 1, nout); m.ld = 0; return m; }
static MatRef f64_hyper(const nif_ctx* c, long slot, int ld, int nin, int nout) {
  MatRef m; m.r = c->r; m.base_k = c->last_w + slot; m.kstride = c->po; m.base_last = c->last_b + slot; m.ld = ld; m.nin = nin; m.nout = nout; return m;
}

static int f64_ensure(nif_ctx* c) {
  if (c->f64) return NIF_OK;
  std::unique_ptr<NifF64> own(new NifF64());      // joins the context after the last step that can fail
  NifF64* f = own.get();
  F64Args& a = f->a;
  memset(&a, 0, sizeof(a));
  a.ncol = c->pi + c->si;
  a.pi = c->pi; a.nst = c->nst; a.lst = c->lst; a.r = c->r; a.p_act = c->cfg.p_act; a.p_res = c->cfg.p_resblock;
  a.p_om = c->cfg.p_act == NIF_ACT_SINE ? (double)c->cfg.p_omega0 : 1.0;
  a.first_w = c->first_w; a.first_b = c->first_b;
  for (int i = 0; i < c->lst; ++i) { a.hid_w[i] = c->hid_w[i]; a.hid_b[i] = c->hid_b[i]; a.hid_w2[i] = c->hid_w2[i]; a.hid_b2[i] = c->hid_b2[i]; }
  a.bott_w = c->bott_w; a.bott_b = c->bott_b; a.last_w = c->last_w; a.last_b = c->last_b;
  a.si = c->si; a.so = c->so; a.n = c->n; a.nh = c->nh; a.po = c->po;
  a.nif_skip = c->kind == NIF_KIND_NIF; a.s_res = c->cfg.s_resblock;
  a.s_act = a.nif_skip ? c->cfg.s_act : NIF_ACT_SINE;
  a.s_om = a.nif_skip ? 1.0 : (double)c->cfg.s_omega0;
  const long P = c->P;
  const int n = c->n, nst = c->nst, lst = c->lst, nh = c->nh, K = c->r + 1, nit = (n + 15) / 16;
  // the segment rows hold a whole gradient each: fewer of them for very large parameter vectors (fixed per context: still deterministic)
  f->S = F64_SEGS;
  while (f->S > 1 && (double)f->S * (double)P > 3.3e7) f->S >>= 1;
  f->seglen = F64_CHUNK / f->S;
  f->pstride = (P + 1 + 15) / 16 * 16;
  const long rows = c->pi + nst + (long)(lst + 1) * nst + 3L * lst * nst + nst + 2L * lst * nst + 2L * nst + K + K + (long)nit * K + c->si + n +
                    (long)(nh + 1) * n + (long)nh * n + n + (long)nh * n + c->so + 3L * n + 1;
  int rc = f->theta.alloc(P); if (rc) return rc;
  rc = f->g.alloc(P + 1); if (rc) return rc;
  rc = f->stash.alloc(rows * CH); if (rc) return rc;
  rc = f->part.alloc(f->pstride * f->S); if (rc) return rc;
  HIPCHK(hipMemsetAsync(f->stash, 0, sizeof(double) * (size_t)rows * CH, c->st));
  HIPCHK(hipMemsetAsync(f->part, 0, sizeof(double) * (size_t)f->pstride * f->S, c->st));
  HIPCHK(hipMemsetAsync(f->g, 0, sizeof(double) * (size_t)(P + 1), c->st));
  double* p = f->stash;
  auto take = [&](long nrows) { double* q = p; p += nrows * CH; return q; };
  a.PP = take(c->pi); a.PA0 = take(nst); a.PH = take((long)(lst + 1) * nst); a.PA1 = take((long)lst * nst); a.PT = take((long)lst * nst);
  a.PA2 = take((long)lst * nst); a.PGA0 = take(nst); a.PGA1 = take((long)lst * nst); a.PGA2 = take((long)lst * nst); a.PGH = take(2L * nst);
  a.ZT = take(K); a.GZT = take(K); a.GZTP = take((long)nit * K); a.X = take(c->si); a.A0 = take(n); a.H = take((long)(nh + 1) * n);
  a.A = take((long)nh * n); a.GA0 = take(n); a.GA = take((long)nh * n); a.GU = take(c->so); a.GH = take(3L * n); a.LOSSP = take(1);
  a.theta = f->theta;
  // the weight-gradient job table: together the jobs cover every parameter exactly once
  std::vector<F64Job> jobs; int waves = 0;
  const double pom = a.p_om, som = a.s_om;
  f64_add_job(jobs, waves, a.PP, a.PGA0, nullptr, c->pi, nst, 1, f64_dense(c->first_w, c->pi, nst), pom);
  f64_add_job(jobs, waves, nullptr, a.PGA0, nullptr, 1, nst, 1, f64_vec(c->first_b, nst), 1.0);
  for (int l = 0; l < lst; ++l) {
    f64_add_job(jobs, waves, a.PH + (long)l * nst * CH, a.PGA1 + (long)l * nst * CH, nullptr, nst, nst, 1, f64_dense(c->hid_w[l], nst, nst), pom);
    f64_add_job(jobs, waves, nullptr, a.PGA1 + (long)l * nst * CH, nullptr, 1, nst, 1, f64_vec(c->hid_b[l], nst), 1.0);
    if (a.p_res) {
      f64_add_job(jobs, waves, a.PT + (long)l * nst * CH, a.PGA2 + (long)l * nst * CH, nullptr, nst, nst, 1, f64_dense(c->hid_w2[l], nst, nst), pom);
      f64_add_job(jobs, waves, nullptr, a.PGA2 + (long)l * nst * CH, nullptr, 1, nst, 1, f64_vec(c->hid_b2[l], nst), 1.0);
    }
  }
  f64_add_job(jobs, waves, a.PH + (long)lst * nst * CH, a.GZT, nullptr, nst, c->r, 1, f64_dense(c->bott_w, nst, c->r), 1.0);
  f64_add_job(jobs, waves, nullptr, a.GZT, nullptr, 1, c->r, 1, f64_vec(c->bott_b, c->r), 1.0);
  f64_add_job(jobs, waves, a.X, a.GA0, a.ZT, c->si, n, K, f64_hyper(c, f64_w1(a), n, c->si, n), som);
  f64_add_job(jobs, waves, nullptr, a.GA0, a.ZT, 1, n, K, f64_hyper(c, f64_b1(a), 0, 1, n), 1.0);
  for (int m = 0; m < nh; ++m) {
    f64_add_job(jobs, waves, a.H + (long)m * n * CH, a.GA + (long)m * n * CH, a.ZT, n, n, K, f64_hyper(c, f64_wh(a, m), n, n, n), som);
    f64_add_job(jobs, waves, nullptr, a.GA + (long)m * n * CH, a.ZT, 1, n, K, f64_hyper(c, f64_bh(a, m), 0, 1, n), 1.0);
  }
  f64_add_job(jobs, waves, a.H + (long)nh * n * CH, a.GU, a.ZT, n, c->so, K, f64_hyper(c, f64_wl(a), c->so, n, c->so), 1.0);
  f64_add_job(jobs, waves, nullptr, a.GU, a.ZT, 1, c->so, K, f64_hyper(c, f64_bl(a), 0, 1, c->so), 1.0);
  f->njobs = (int)jobs.size(); f->job_waves = waves;
  rc = f->jobs.alloc((long)jobs.size()); if (rc) return rc;
  HIPCHK(hipMemcpyAsync(f->jobs, jobs.data(), sizeof(F64Job) * jobs.size(), hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));      // (the host table goes out of scope)
  c->f64 = own.release();
  return NIF_OK;
}

void nif_f64_release(nif_ctx* c) { delete c->f64; c->f64 = nullptr; }

// The C-ABI of the path (include/nif_hip.h nif_f64_*).  NIF_FLUSH_NONE throughout: a float64 master vector, [grad | loss] buffer and
// workspace of their own -- theta, grad, the optimizer slots and a pending row reduction of the float32 path are neither read nor written
extern "C" int nif_f64_set_params(nif_ctx* c, const double* host, int64_t n) {
  if (!c || !host) return fail(NIF_ERR_INVALID, "null");
  int rc = f64_supported(c, "nif_f64_set_params"); if (rc) return rc;
  if (n != c->P) return fail(NIF_ERR_INVALID, "parameter count mismatch");
  NIF_ENTER(c, NIF_FLUSH_NONE)
  rc = f64_ensure(c); if (rc) return rc;
  HIPCHK(hipMemcpyAsync(c->f64->theta, host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  c->f64->have_params = true;
  return NIF_OK;
}
extern "C" int nif_f64_get_params(nif_ctx* c, double* host, int64_t n) {
  if (!c || !host) return fail(NIF_ERR_INVALID, "null");
  int rc = f64_supported(c, "nif_f64_get_params"); if (rc) return rc;
  if (n != c->P) return fail(NIF_ERR_INVALID, "parameter count mismatch");
  if (!c->f64 || !c->f64->have_params) return fail(NIF_ERR_STATE, "nif_f64_get_params before nif_f64_set_params");
  NIF_ENTER(c, NIF_FLUSH_NONE)
  HIPCHK(hipMemcpyAsync(host, c->f64->theta, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

// forward (and, with y, loss + adjoint + weight gradients) of every chunk, in chunk order on the context's stream
static int f64_run(nif_ctx* c, const double* xin, const double* y, const double* sw, long B, long Bg, double* u_out) {
  NifF64* f = c->f64;
  const bool train = y != nullptr;
  const int n = c->n, nh = c->nh, nit = (n + 15) / 16;
  const bool nif = c->kind == NIF_KIND_NIF, res = c->cfg.s_resblock != 0;
  hipStream_t st = c->st;
  if (train) HIPCHK(hipMemsetAsync(f->g, 0, sizeof(double) * (size_t)(c->P + 1), st));
  for (long off = 0; off < B; off += CH) {
    F64Args a = f->a;
    a.Bc = (int)(B - off < CH ? B - off : CH);
    a.Bp = (a.Bc + 15) / 16 * 16;
    a.xin = xin + off * a.ncol;
    a.y = train ? y + off * c->so : nullptr;
    a.sw = (train && sw) ? sw + off : nullptr;
    a.inv_bg = 1.0 / (double)Bg;
    a.loss_kind = c->loss_kind;
    a.u_out = u_out ? u_out + off * c->so : nullptr;
    const int pblk = (a.Bp + 63) / 64;
    const int mblk = ((a.Bp / 16) * nit + 3) / 4;
    k64_pnet_fwd<<<pblk, 64, 0, st>>>(a);
    k64_snet_first<<<pblk, 64, 0, st>>>(a);
    for (int m = 0; m < nh; ++m) {
      // class NIF: u = f(a) + u;  SIREN: sin(a);  SIREN resblock: t = sin(a1), then u = 0.5 (u + sin(a2))
      double c1 = 1.0, c2 = 0.0; const double* RES = nullptr;
      if (nif) { c2 = 1.0; RES = a.H + (long)m * n * CH; }
      else if (res && (m & 1)) { c1 = 0.5; c2 = 0.5; RES = a.H + (long)(m - 1) * n * CH; }
      k64_hidden_fwd<<<mblk, 256, 0, st>>>(a, m, c1, c2, RES);
    }
    k64_snet_last<<<pblk, 64, 0, st>>>(a);
    if (train) {
      // dL/dh rotates through three buffers: cur (input of this step), and for resblocks the block's incoming gradient is kept
      double* GH[3] = {a.GH, a.GH + (long)n * CH, a.GH + 2L * n * CH};
      int cur = 0, blk = 0, npart = 0;
      for (int m = nh - 1; m >= 0; --m) {
        const bool odd = res && (m & 1);
        if (odd) blk = cur;
        k64_act_back<<<pblk, 64, 0, st>>>(a, m, GH[cur], odd ? 0.5 : 1.0, npart);
        int out = 0;
        while (out == cur || (res && out == blk)) ++out;
        const double* R = nullptr; double cres = 0.0;
        if (nif) { R = GH[cur]; cres = 1.0; }
        else if (res && !(m & 1)) { R = GH[blk]; cres = 0.5; }
        k64_hidden_bwd<<<mblk, 256, 0, st>>>(a, m, R, cres, GH[out]);
        cur = out; npart = nit;
      }
      k64_act_back<<<pblk, 64, 0, st>>>(a, -1, GH[cur], 1.0, npart);
      k64_pnet_bwd<<<(a.Bc + 63) / 64, 64, 0, st>>>(a);
      const int wv = f->job_waves * f->S;
      k64_wgrad<<<(wv + 3) / 4, 256, 0, st>>>(f->jobs, f->njobs, f->job_waves, f->part, f->pstride, f->S, f->seglen, a.Bc);
      k64_reduce<<<(int)((c->P + 255) / 256), 256, 0, st>>>(f->part, f->pstride, f->S, f->g, c->P);
      k64_loss_reduce<<<1, 256, 0, st>>>(a.LOSSP, a.Bc, f->g + c->P);
    }
    HIPCHK(hipGetLastError());
  }
  return NIF_OK;
}

extern "C" int nif_f64_forward_dev(nif_ctx* c, const double* xin, int64_t B, double* u) {
  if (!c || !xin || !u || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  int rc = f64_supported(c, "nif_f64_forward_dev"); if (rc) return rc;
  if (!c->f64 || !c->f64->have_params) return fail(NIF_ERR_STATE, "nif_f64_forward_dev before nif_f64_set_params");
  NIF_ENTER(c, NIF_FLUSH_NONE)
  return f64_run(c, xin, nullptr, nullptr, B, B, u);
}
extern "C" int nif_f64_loss_grad_dev(nif_ctx* c, const double* xin, const double* y, const double* sw, int64_t B, int64_t Bg) {
  if (!c || !xin || !y || B <= 0 || Bg < B) return fail(NIF_ERR_INVALID, "bad argument");
  int rc = f64_supported(c, "nif_f64_loss_grad_dev"); if (rc) return rc;
  if (!c->f64 || !c->f64->have_params) return fail(NIF_ERR_STATE, "nif_f64_loss_grad_dev before nif_f64_set_params");
  NIF_ENTER(c, NIF_FLUSH_NONE)
  rc = f64_run(c, xin, y, sw, B, Bg, nullptr); if (rc) return rc;
  c->f64->have_grad = true;
  return NIF_OK;
}
extern "C" int nif_f64_grad_read(nif_ctx* c, double* loss, double* grad) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  int rc = f64_supported(c, "nif_f64_grad_read"); if (rc) return rc;
  if (!c->f64 || !c->f64->have_grad) return fail(NIF_ERR_STATE, "nif_f64_grad_read before nif_f64_loss_grad_dev");
  NIF_ENTER(c, NIF_FLUSH_NONE)
  if (grad) HIPCHK(hipMemcpyAsync(grad, c->f64->g, sizeof(double) * (size_t)c->P, hipMemcpyDeviceToHost, c->st));
  if (loss) HIPCHK(hipMemcpyAsync(loss, c->f64->g + c->P, sizeof(double), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}
