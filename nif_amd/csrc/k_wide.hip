// k_wide.hip -- workgroup-tiled dense layers of the last-layer class's shared SIREN ShapeNet at 129..512 units.
//
// Every kernel of the library that runs this class below 129 units keeps a tile of points x ALL features in the registers of one wave;
// at 256 units that is 400..500 VGPRs.  Here a layer is one launch and a WORKGROUP owns an output tile of WT_F = 128 rows x WT_P = 64
// columns: its four waves take 32 rows each and both 32-column halves (two f32x16 accumulators, v_mfma_f32_32x32x2_f32), the reduction
// index is walked in chunks of WT_K = 32 through the LDS.  One tile program (wide_mma) serves three roles; they differ in what the rows,
// the columns and the reduction index ARE, i.e. in how a chunk is brought into the LDS and where the accumulators go:
//
//   role      rows (A side)              columns (B side)     reduction        epilogue
//   forward   output features f          points of 2 tiles    input features   sin(omega acc + b) -> OUT, cos -> COS (training)
//   adjoint   input features k           points of 2 tiles    output features  COS(k, p) scale acc -> OUT = dL/da of the layer below
//   gradient  input features k, + bias   output features f    points of a tile partial[row][W(k, f)] = scale acc, partial[row][b(f)]
//
// Activations, stashes and adjoints are [tile][feature][32 points] fp32 with exactly `feature count` rows per tile -- the layout of
// PHI / DPHI (LLArgs), so the bottleneck's output IS c->PHI and its adjoint reads c->DPHI as k_ll_out wrote it.  W is read row-major
// straight from theta: there is no packed image of a wide matrix, hence nothing a weight update could leave stale.
//
// Bounds: every LDS element is written by a guarded load (row < rows, reduction index < K, tile < ntiles, point < B where the role
// sums over points) and zero otherwise, so the MFMA loop needs no guard; every global store is guarded by row < nrow, column < ncol /
// tile < ntiles.  LDS: (129 + 65) x 32 floats = 24.8 KB, static.
#include "nif_internal.h"

#define WT_F 128      // rows of a workgroup tile (4 waves x 32)
#define WT_P 64       // columns
#define WT_K 32       // reduction chunk
#define WT_AS (WT_F + 1)      // LDS row strides: odd, so that the transposing fills (32 consecutive reduction indices of one row) hit 32 banks
#define WT_BS (WT_P + 1)

enum { WIDE_FWD = 0, WIDE_ADJ = 1, WIDE_GW = 2 };

// acc[c] += A(rows 32 w ..) x B(columns 32 c ..) over one LDS chunk of kk reduction steps (kk even)
__device__ __forceinline__ void wide_mma(const float* As, const float* Bs, int kk, int wave, int lane, f32x16 (&acc)[2]) {
  const int p = lane & 31, hf = lane >> 5;
  const float* a = As + hf * WT_AS + 32 * wave + p;
  const float* b = Bs + hf * WT_BS + p;
  for (int k = 0; k < kk; k += 2) {
    const float av = a[k * WT_AS], b0 = b[k * WT_BS], b1 = b[k * WT_BS + 32];
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
  }
}

// A chunk travels global -> registers (fetch) -> LDS (deposit): the fetch of chunk i + 1 is issued in front of the MFMAs of chunk i, so
// its latency runs under them.  Per thread and chunk: WT_NA elements of the A side, WT_NB of the B side
#define WT_NA (WT_K * WT_F / 256)
#define WT_NB (WT_K * WT_P / 256)

// A side of the two point roles.  Forward: As[k][i] = W[k0 + k][r0 + i], rows of W, coalesced along i; adjoint: As[k][i] =
// W[r0 + i][k0 + k], the transpose, coalesced along k
template <int ROLE>
__device__ __forceinline__ void wide_fetch_w(float (&va)[WT_NA], const float* __restrict__ W, int ld, int K, int nrow, int k0, int r0, int tid) {
  // element q of a thread: forward (k, i) = (tid / 128 + 2 q, tid % 128), adjoint (tid % 32, tid / 32 + 8 q): one base, one stride
  const int k = ROLE == WIDE_FWD ? tid >> 7 : tid & 31, i = ROLE == WIDE_FWD ? tid & 127 : tid >> 5;
  const float* ptr = ROLE == WIDE_FWD ? W + (long)(k0 + k) * ld + r0 + i : W + (long)(r0 + i) * ld + k0 + k;
  const long step = (ROLE == WIDE_FWD ? 2L : 8L) * ld;
#pragma unroll
  for (int q = 0; q < WT_NA; ++q, ptr += step) {
    const bool ok = ROLE == WIDE_FWD ? (k0 + k + 2 * q < K && r0 + i < nrow) : (k0 + k < K && r0 + i + 8 * q < nrow);
    va[q] = 0.f;
    if (ok) va[q] = *ptr;
  }
}
template <int ROLE>
__device__ __forceinline__ void wide_deposit_w(float* As, const float (&va)[WT_NA], int tid) {
#pragma unroll
  for (int q = 0; q < WT_NA; ++q) {
    const int e = tid + 256 * q;
    const int k = ROLE == WIDE_FWD ? e >> 7 : e & 31, i = ROLE == WIDE_FWD ? e & 127 : e >> 5;
    As[k * WT_AS + i] = va[q];
  }
}
// B side of the two point roles: Bs[k][j] = SRC[tile t0 + j / 32][k0 + k][j % 32], or the first layer's coordinates
__device__ __forceinline__ void wide_fetch_points(float (&vb)[WT_NB], const WideArgs& A, const float* __restrict__ src, int K, int k0, long t0, int tid) {
  // element q of a thread: (k, j) = (tid / 64 + 4 q, tid % 64): one tile and point per thread, the feature moves
  const int j = tid & 63, kg = k0 + (tid >> 6);
  const long t = t0 + (j >> 5), pt = t * 32 + (j & 31);
  const bool ok = t < A.ntiles && (src || pt < A.B);
  const float* ptr = src ? src + (t * K + kg) * 32 + (j & 31) : A.xin + pt * A.ncol + A.col0 + kg;
  const int step = src ? 4 * 32 : 4;
#pragma unroll
  for (int q = 0; q < WT_NB; ++q, ptr += step) {
    vb[q] = 0.f;
    if (ok && kg + 4 * q < K) vb[q] = *ptr;
  }
}
__device__ __forceinline__ void wide_deposit_points(float* Bs, const float (&vb)[WT_NB], int tid) {
#pragma unroll
  for (int q = 0; q < WT_NB; ++q) {
    const int e = tid + 256 * q;
    Bs[(e >> 6) * WT_BS + (e & 63)] = vb[q];
  }
}

// forward (rows = output features) and adjoint (rows = input features): persistent over (point block, row block) items
template <int ROLE>
__global__ __launch_bounds__(256) void k_wide_layer(WideArgs A) {
  __shared__ float As[WT_K * WT_AS];
  __shared__ float Bs[WT_K * WT_BS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 31, hf = lane >> 5;
  const int nrow = ROLE == WIDE_FWD ? A.nout : A.nin;      // rows of the output
  const int K = ROLE == WIDE_FWD ? A.nin : A.nout;         // reduction length
  const long nrb = (nrow + WT_F - 1) / WT_F, npb = (A.ntiles + 1) / 2;
  const float* __restrict__ W = A.theta + A.w_off;
  const float* __restrict__ src = ROLE == WIDE_FWD ? A.IN : A.DA;
  for (long item = blockIdx.x; item < nrb * npb; item += gridDim.x) {
    const int r0 = (int)(item % nrb) * WT_F;
    const long t0 = (item / nrb) * 2;
    f32x16 acc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[c][v] = 0.f;
    float va[WT_NA], vb[WT_NB];
    wide_fetch_w<ROLE>(va, W, A.ld, K, nrow, 0, r0, tid);
    wide_fetch_points(vb, A, src, K, 0, t0, tid);
    for (int k0 = 0; k0 < K; k0 += WT_K) {
      __syncthreads();      // the previous chunk (or item) has been consumed
      wide_deposit_w<ROLE>(As, va, tid);
      wide_deposit_points(Bs, vb, tid);
      __syncthreads();
      if (k0 + WT_K < K) {
        wide_fetch_w<ROLE>(va, W, A.ld, K, nrow, k0 + WT_K, r0, tid);
        wide_fetch_points(vb, A, src, K, k0 + WT_K, t0, tid);
      }
      const int kk = K - k0 < WT_K ? (K - k0 + 1) & ~1 : WT_K;
      wide_mma(As, Bs, kk, wave, lane, acc);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const long t = t0 + c;
      if (t >= A.ntiles) continue;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int f = r0 + 32 * wave + fmap(v, hf);
        if (f >= nrow) continue;
        const long o = (t * nrow + f) * 32 + p;
        if (ROLE == WIDE_FWD) {
          const float ph = fmaf(A.scale, acc[c][v], A.theta[A.b_off + f]);
          if (A.sine) {
            float s, co; nif_sincosf(ph, &s, &co);
            A.OUT[o] = s;
            if (A.COS) A.COS[o] = co;
          } else A.OUT[o] = ph;
        } else {
          A.OUT[o] = A.COS[o] * (A.scale * acc[c][v]);
        }
      }
    }
  }
}

// the gradient role's chunk = one tile of points: As[q][i] = IN[t][r0 + i][q] (q = point), 1 in the bias row, Bs[q][j] = DA[t][c0 + j][q];
// a point >= B adds nothing
__device__ __forceinline__ void wide_fetch_gw(float (&va)[WT_NA], float (&vb)[WT_NB], const WideArgs& A, long t, int r0, int c0, int tid) {
  // element s of a thread: point q = tid % 32, row / column tid / 32 + 8 s
  const int q = tid & 31, i0 = tid >> 5, k = r0 + i0;
  const long pt = t * 32 + q;
  const bool live = pt < A.B;
  const float* pa = A.IN ? A.IN + (t * A.nin + k) * 32 + q : A.xin + pt * A.ncol + A.col0 + k;
  const int sa = A.IN ? 8 * 32 : 8;
#pragma unroll
  for (int s = 0; s < WT_NA; ++s, pa += sa) {
    va[s] = (live && k + 8 * s == A.nin) ? 1.0f : 0.f;
    if (live && k + 8 * s < A.nin) va[s] = *pa;
  }
  const float* pb = A.DA + (t * A.nout + c0 + i0) * 32 + q;
#pragma unroll
  for (int s = 0; s < WT_NB; ++s, pb += 8 * 32) {
    vb[s] = 0.f;
    if (live && c0 + i0 + 8 * s < A.nout) vb[s] = *pb;
  }
}
// weight and bias gradient of one layer: grid (rows, row blocks x column blocks).  Workgroup (x, y) sums the tiles x, x + gridDim.x, ..
// in that order into its 128 x 64 block of [IN | 1]^T DA and writes it into partial row x: the order is fixed, k_reduce sums the rows
__global__ __launch_bounds__(256) void k_wide_gw(WideArgs A) {
  __shared__ float As[WT_K * WT_AS];
  __shared__ float Bs[WT_K * WT_BS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 31, hf = lane >> 5;
  const int ncb = (A.nout + WT_P - 1) / WT_P;      // (rows: nin + 1, row nin the ones row, i.e. the bias gradient)
  const int r0 = ((int)blockIdx.y / ncb) * WT_F, c0 = ((int)blockIdx.y % ncb) * WT_P;
  f32x16 acc[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[c][v] = 0.f;
  float va[WT_NA], vb[WT_NB];
  if ((long)blockIdx.x < A.ntiles) wide_fetch_gw(va, vb, A, blockIdx.x, r0, c0, tid);
  for (long t = blockIdx.x; t < A.ntiles; t += gridDim.x) {
    __syncthreads();
#pragma unroll
    for (int s = 0; s < WT_NA; ++s) { const int e = tid + 256 * s; As[(e & 31) * WT_AS + (e >> 5)] = va[s]; }
#pragma unroll
    for (int s = 0; s < WT_NB; ++s) { const int e = tid + 256 * s; Bs[(e & 31) * WT_BS + (e >> 5)] = vb[s]; }
    __syncthreads();
    if (t + gridDim.x < A.ntiles) wide_fetch_gw(va, vb, A, t + gridDim.x, r0, c0, tid);
    wide_mma(As, Bs, WT_K, wave, lane, acc);
  }
  float* prow = A.partial + (long)blockIdx.x * A.pstride;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int f = c0 + 32 * c + p;
    if (f >= A.nout) continue;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int k = r0 + 32 * wave + fmap(v, hf);
      if (k < A.nin) prow[A.w_off + (long)k * A.ld + f] = A.scale * acc[c][v];
      else if (k == A.nin) prow[A.b_off + f] = acc[c][v];
    }
  }
}

static unsigned wide_grid(const WideArgs& a, int nrow) {
  const long items = (long)((nrow + WT_F - 1) / WT_F) * ((a.ntiles + 1) / 2);
  const long cap = 256 * 4;      // four workgroups of 25 KB LDS and 256 threads per CU: the loop wraps beyond
  return (unsigned)(items < cap ? (items < 1 ? 1 : items) : cap);
}
void launch_wide_fwd(const WideArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((k_wide_layer<WIDE_FWD>), dim3(wide_grid(a, a.nout)), dim3(256), 0, st, a);
}
void launch_wide_adj(const WideArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((k_wide_layer<WIDE_ADJ>), dim3(wide_grid(a, a.nin)), dim3(256), 0, st, a);
}
void launch_wide_gw(const WideArgs& a, int rows, hipStream_t st) {
  const int nrb = (a.nin + 1 + WT_F - 1) / WT_F, ncb = (a.nout + WT_P - 1) / WT_P;
  hipLaunchKernelGGL(k_wide_gw, dim3((unsigned)rows, (unsigned)(nrb * ncb)), dim3(256), 0, st, a);
}
