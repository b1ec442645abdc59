// k_prune.hip -- low-magnitude pruning of the flat parameter vector (nif_prune_*; tfmot.sparsity.keras semantics, nif_amd/sparsity.py).
//   * select: the exact k-th largest |w| of every pruned tensor (segment) in one set of launches, by radix select on the bits of |w|.
//     With the sign bit cleared a float's bits are a 31-bit unsigned key whose order is the order of the magnitudes (zeros, denormals
//     and infinities included; -0 and +0 share key 0).  Three digit passes of 11 / 10 / 10 bits, each two kernels:
//       k_prune_hist: per-block LDS histograms of the pass's digit among the keys that carry the prefix selected so far -- one
//         sub-histogram per wave, because weights crowd into a few exponents (the first digit holds the exponent) and a single LDS
//         histogram would serialise four waves on the same bins -- then one integer global atomic per nonzero bin per block;
//       k_prune_pick: one workgroup per segment scans its histogram from the top bin down, takes the bin that holds the k-th largest,
//         appends it to the prefix, subtracts the keys above it from the rank, and clears the histogram for the next pass.
//     Integer counts: the result does not depend on the order the atomics land in, and ranks of a data-parallel run that hold the
//     same weights select the same thresholds without talking to each other.
//   * mask: mask[i] = key(w[i]) >= key(thr) (ties keep more than k entries, as TF-MOT's `abs(w) >= threshold` does).
//   * apply: theta[i] = mask[i] ? theta[i] : theta[i] * 0 (TF-MOT's `weight * mask`, signed zeros included) as one 16-byte stream over
//     the span of the segments; outside the segments the byte mask holds 1, so those floats are stored back unchanged.
#include "nif_internal.h"

namespace {

__device__ __forceinline__ unsigned mag_key(float w) { return __float_as_uint(w) & 0x7fffffffu; }

// the segment that owns flattened block b: the last one whose first block is <= b
__device__ __forceinline__ int seg_of_block(const PruneSeg* __restrict__ segs, int nseg, long b) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// digit (key >> SHIFT) & (2^WIDTH - 1) among the keys whose bits above SHIFT + WIDTH equal the selected prefix's
template <int SHIFT, int WIDTH, bool FIRST>
__global__ __launch_bounds__(256) void k_prune_hist(const float* __restrict__ theta, const PruneSeg* __restrict__ segs, int nseg,
                                                    const PruneSel* __restrict__ sel, unsigned* __restrict__ hist) {
  constexpr int NB = 1 << WIDTH;
  __shared__ unsigned h[4][NB];
  const int s = seg_of_block(segs, nseg, blockIdx.x);
  const PruneSeg sg = segs[s];
  const int wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * NB; i += 256) (&h[0][0])[i] = 0u;
  __syncthreads();
  const unsigned want = FIRST ? 0u : (sel[s].prefix >> (SHIFT + WIDTH));      // (SHIFT + WIDTH = 31 in the first pass: every key)
  const long base = (blockIdx.x - sg.blk0) * (long)PRUNE_CHUNK;
  const float* __restrict__ w = theta + sg.off;
#pragma unroll
  for (int j = 0; j < PRUNE_CHUNK / 256; ++j) {
    const long i = base + j * 256 + threadIdx.x;
    if (i < sg.size) {
      const unsigned key = mag_key(w[i]);
      if ((key >> (SHIFT + WIDTH)) == want) atomicAdd(&h[wave][(key >> SHIFT) & (NB - 1)], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < NB; b += 256) {
    const unsigned c = h[0][b] + h[1][b] + h[2][b] + h[3][b];
    if (c) atomicAdd(&hist[(long)s * PRUNE_BINS + b], c);
  }
}

// thread t owns the bins NB-1-t*PER down to NB-(t+1)*PER; an inclusive scan of the per-thread totals from the top gives every thread
// the count of keys above its bins, and the one thread whose range holds rank krem walks its bins
template <int SHIFT, int WIDTH, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void k_prune_pick(const PruneSeg* __restrict__ segs, PruneSel* __restrict__ sel,
                                                    unsigned* __restrict__ hist, float* __restrict__ thr) {
  constexpr int NB = 1 << WIDTH, PER = NB / 256;
  __shared__ unsigned scan[256];
  const int s = blockIdx.x, t = threadIdx.x;
  unsigned* __restrict__ hs = hist + (long)s * PRUNE_BINS;
  const unsigned krem = FIRST ? (unsigned)segs[s].k : sel[s].krem;
  const unsigned prefix = FIRST ? 0u : sel[s].prefix;
  const int top = NB - 1 - t * PER;
  unsigned c[PER], tot = 0u;
#pragma unroll
  for (int j = 0; j < PER; ++j) { c[j] = hs[top - j]; tot += c[j]; }
  scan[t] = tot;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned v = t >= d ? scan[t - d] : 0u;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const unsigned above = scan[t] - tot;
  if (above < krem && krem <= above + tot) {
    unsigned acc = above;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (acc + c[j] >= krem) {
        const unsigned p = prefix | ((unsigned)(top - j) << SHIFT);
        sel[s].prefix = p;
        sel[s].krem = krem - acc;
        if (LAST) thr[s] = __uint_as_float(p);
        break;
      }
      acc += c[j];
    }
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) hs[top - j] = 0u;      // (each thread read only its own bins)
}

__global__ __launch_bounds__(256) void k_prune_mask(const float* __restrict__ theta, const PruneSeg* __restrict__ segs, int nseg,
                                                    const float* __restrict__ thr, unsigned char* __restrict__ mask) {
  const int s = seg_of_block(segs, nseg, blockIdx.x);
  const PruneSeg sg = segs[s];
  const unsigned tk = mag_key(thr[s]);
  const long base = (blockIdx.x - sg.blk0) * (long)PRUNE_CHUNK;
#pragma unroll
  for (int j = 0; j < PRUNE_CHUNK / 256; ++j) {
    const long i = base + j * 256 + threadIdx.x;
    if (i < sg.size) mask[sg.off + i] = mag_key(theta[sg.off + i]) >= tk ? 1 : 0;
  }
}

__device__ __forceinline__ float masked(float t, unsigned char m) { return m ? t : t * 0.0f; }

// quads [q0, q1) of theta; a quad that runs past P is done element by element
__global__ __launch_bounds__(256) void k_prune_apply(float* __restrict__ theta, const unsigned char* __restrict__ mask, long q0, long q1,
                                                     long P) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long q = q0 + (long)blockIdx.x * blockDim.x + threadIdx.x; q < q1; q += stride) {
    if (4 * q + 4 <= P) {
      f32x4 t4 = reinterpret_cast<const f32x4*>(theta)[q];
      const uchar4 m4 = reinterpret_cast<const uchar4*>(mask)[q];
      t4[0] = masked(t4[0], m4.x); t4[1] = masked(t4[1], m4.y); t4[2] = masked(t4[2], m4.z); t4[3] = masked(t4[3], m4.w);
      reinterpret_cast<f32x4*>(theta)[q] = t4;
    } else {
      for (long i = 4 * q; i < P; ++i) theta[i] = masked(theta[i], mask[i]);
    }
  }
}

}  // namespace

void launch_prune_update(const float* theta, const PruneSeg* segs, int nseg, long nblk, unsigned* hist, PruneSel* sel, float* thr,
                         unsigned char* mask, hipStream_t st) {
  const dim3 gb((unsigned)nblk), gs((unsigned)nseg), blk(256);
  hipLaunchKernelGGL((k_prune_hist<20, 11, true>), gb, blk, 0, st, theta, segs, nseg, (const PruneSel*)sel, hist);
  hipLaunchKernelGGL((k_prune_pick<20, 11, true, false>), gs, blk, 0, st, segs, sel, hist, thr);
  hipLaunchKernelGGL((k_prune_hist<10, 10, false>), gb, blk, 0, st, theta, segs, nseg, (const PruneSel*)sel, hist);
  hipLaunchKernelGGL((k_prune_pick<10, 10, false, false>), gs, blk, 0, st, segs, sel, hist, thr);
  hipLaunchKernelGGL((k_prune_hist<0, 10, false>), gb, blk, 0, st, theta, segs, nseg, (const PruneSel*)sel, hist);
  hipLaunchKernelGGL((k_prune_pick<0, 10, false, true>), gs, blk, 0, st, segs, sel, hist, thr);
  hipLaunchKernelGGL(k_prune_mask, gb, blk, 0, st, theta, segs, nseg, (const float*)thr, mask);
}

void launch_prune_apply(float* theta, const unsigned char* mask, long lo, long hi, long P, hipStream_t st) {
  const long q0 = lo / 4, q1 = (hi + 3) / 4;
  long blocks = (q1 - q0 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_prune_apply, dim3((unsigned)blocks), dim3(256), 0, st, theta, mask, q0, q1, P);
}
