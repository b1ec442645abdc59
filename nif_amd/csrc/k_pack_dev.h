// k_pack_dev.h -- the weight-plane contract.  Every matrix kernel reads theta through PACKED PLANE IMAGES written by k_pack.hip; their
// layout is stated HERE once: the packers build the images from these functions, nif_api.hip sizes and offsets its buffers with them,
// and every consumer pins its own stride constants to them with a static_assert next to the constant.
//
// 16-bit sets (A operands of v_mfma_f32_16x16x32_bf16 / _f16): a plane (one k of one matrix) is NCH = NBL / 2 K-step chunks; a chunk
// holds, per 16-row block, `splits` groups of 64 lanes x one 16-byte unit (8 elements): unit ((blk splits + s) 64 + lane), element t =
// split s of M[in][out], slot = 16 (2 ks + (t >> 2)) + 4 (lane >> 4) + (t & 3) (exactly what a lane of the previous layer's C/D tile
// holds in blocks 2ks, 2ks+1), row = 16 blk + (lane & 15); forward (in, out) = (slot, row), adjoint (row, slot); outside the matrix: 0
//   split    3 / 2 splits, bf16          x = x0 + x1 + x2 exactly (8 + 8 + 8 significand bits)
//   compact  1 / 1, bf16 or half         the policies' set: bf16(x) (mixed_bfloat16) or half(x), RNE, saturated (mixed_float16)
//   half     2 / 2, half                 hi + lo of s x, s the plane's power of two (plane_scale_shift); both directions in the ADJOINT geometry
//   phi      3 / 2, bf16                 dense [n][sop <= 32] of the last-layer class: forward chunks of its TWO output blocks, ONE adjoint chunk
// fp32 sets (f32-input MFMAs), one f32x4 per (block pair, lane); the adjoint image swaps ib / ob and in / out:
//   tiles16  ((ob NBL + ib) 64 + lane) 4 + v : M[in = 16ib + 4(lane>>4) + v][out = 16ob + (lane&15)]
//   tiles32  block (ob,ib), quad vq, lane, c : M[in = 32ib + fmap(4vq+c, lane>>5)][out = 32ob + (lane&31)]
#pragma once
#include "nif_internal.h"

enum PlaneSet { PLANES_SPLIT, PLANES_COMPACT, PLANES_HALF, PLANES_PHI, PLANES_T16, PLANES_T32 };
enum PlaneDir { PLANE_FWD, PLANE_BWD };
#define PLANE_UNIT_BYTES 16
#define NIF_PLANE_FN constexpr __host__ __device__ inline

// 16-row blocks of an n-wide layer, padded to a supported count
NIF_PLANE_FN int plane_nbl(int n) { return (n + 15) / 16 <= 4 ? (n + 15) / 16 : ((n + 15) / 16 <= 6 ? 6 : 8); }
NIF_PLANE_FN int plane_elem_bytes(PlaneSet s) { return s == PLANES_T16 || s == PLANES_T32 ? 4 : 2; }
NIF_PLANE_FN int plane_splits(PlaneSet s, PlaneDir d) {
  return s == PLANES_COMPACT ? 1 : ((s == PLANES_HALF || d == PLANE_BWD) ? 2 : 3);
}
// blocks and 16-byte units of one chunk, chunks of one plane (16-bit sets)
NIF_PLANE_FN int plane_chunk_blocks(PlaneSet s, PlaneDir d, int NBL) { return s == PLANES_PHI && d == PLANE_FWD ? 2 : NBL; }
NIF_PLANE_FN int plane_chunk_units(PlaneSet s, PlaneDir d, int NBL) { return plane_chunk_blocks(s, d, NBL) * plane_splits(s, d) * 64; }
NIF_PLANE_FN int plane_chunks(PlaneSet s, PlaneDir d, int NBL) { return s == PLANES_PHI && d == PLANE_BWD ? 1 : NBL / 2; }
// elements of one plane; NBL = blocks per side (16-row blocks; 32-row blocks for tiles32)
NIF_PLANE_FN long plane_elems(PlaneSet s, PlaneDir d, int NBL) {
  return s == PLANES_T16 ? (long)NBL * NBL * 256
       : s == PLANES_T32 ? (long)NBL * NBL * 1024
       : (long)plane_chunks(s, d, NBL) * plane_chunk_units(s, d, NBL) * (PLANE_UNIT_BYTES / plane_elem_bytes(s));
}
// elements / bytes of the r + 1 planes of ONE n x n matrix (the sets in 16-row blocks)
NIF_PLANE_FN long plane_mat_elems(PlaneSet s, PlaneDir d, int n, int r) { return plane_elems(s, d, plane_nbl(n)) * (r + 1); }
NIF_PLANE_FN long plane_mat_bytes(PlaneSet s, PlaneDir d, int n, int r) { return plane_mat_elems(s, d, n, r) * plane_elem_bytes(s); }

// ---- what every packer shares --------------------------------------------------------------------
// element `rem` of a 16-bit plane whose chunks hold `nblk` blocks of `ns` splits -> its split, K slot and row
__device__ __forceinline__ void pack_decode(long rem, int ns, int nblk, int& s, int& slot, int& row) {
  const int t = rem & 7; rem >>= 3;
  const int lane = rem & 63; rem >>= 6;
  s = (int)(rem % ns); rem /= ns;
  const int blk = (int)(rem % nblk), ks = (int)(rem / nblk);
  slot = 16 * (2 * ks + (t >> 2)) + 4 * (lane >> 4) + (t & 3);
  row = 16 * blk + (lane & 15);
}
// scale * M^(k)[in][out], zero outside the matrix (the padded rows / columns of every plane)
__device__ __forceinline__ float pack_theta(const float* __restrict__ theta, const MatRef& m, int k, int in, int out, float scale) {
  return (in < m.nin && out < m.nout) ? scale * theta[matref_index(m, k, in, out)] : 0.f;
}
// split s of x = x0 + x1 + x2 in bf16 (s = 0 alone: the compact bf16 plane)
__device__ __forceinline__ __bf16 pack_split_bf16(float x, int s) {
  const __bf16 x0 = (__bf16)x;
  const float r1 = x - (float)x0;
  const __bf16 x1 = (__bf16)r1;
  return s == 0 ? x0 : (s == 1 ? x1 : (__bf16)(r1 - (float)x1));
}
// half(x), RNE, saturated at the largest finite half; split s of x = hi + lo on it (11 + 11 significand bits: |x - hi - lo| <= 2^-24 |x|)
__device__ __forceinline__ _Float16 pack_sat_half(float x) { return (_Float16)__builtin_amdgcn_fmed3f(x, -65504.0f, 65504.0f); }
__device__ __forceinline__ _Float16 pack_split_half(float x, int s) {
  const _Float16 h0 = pack_sat_half(x);
  return s == 0 ? h0 : (_Float16)(x - (float)h0);
}
// max |scale M^(k)| over a workgroup of 256 threads, returned to all of them (red: 256 floats of LDS; the leading barrier lets a caller use it again)
__device__ __forceinline__ float plane_absmax(const float* __restrict__ theta, const MatRef& m, int k, float scale, float* red) {
  float mx = 0.f;
  for (int q = threadIdx.x; q < m.nin * m.nout; q += 256) {
    const int in = q / m.nout, out = q - in * m.nout;
    mx = fmaxf(mx, fabsf(scale * theta[matref_index(m, k, in, out)]));
  }
  __syncthreads();
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  return red[0];
}
// the half planes' power of two 2^sh for a plane of largest entry mx = f 2^ex, f in [0.5, 1): max |2^sh x| in [2^13, 2^14); an
// all-zero or non-finite plane takes 1, and |sh| <= 60 (the scaled constants of sine16_tag_sc stay normal numbers)
__device__ __forceinline__ int plane_scale_shift(float mx) {
  int ex = 0;
  if (mx > 0.f && mx < 3.0e38f) (void)frexpf(mx, &ex); else ex = 14;
  const int sh = 14 - ex;
  return sh > 60 ? 60 : (sh < -60 ? -60 : sh);
}
// where a scale table holds [s | 1 / s] of plane k of batch matrix `mat`
__device__ __forceinline__ long plane_scale_index(int mat, int r, int k) { return ((long)mat * (r + 1) + k) * 2; }

// ---- host side (k_pack.hip) ------------------------------------------------------------------------
struct PlanePair { void* F = nullptr; void* B = nullptr; };      // forward / adjoint image of one plane set; null: not written
// One packing job over the 16-bit sets: `nmat` equally shaped matrices `mstride` slots apart in `theta`, the first one m0, scaled by
// `scale` (omega_0 of the SIREN layer, folded into the planes so that no consumer multiplies by it per element).  Batch entry y goes
// to matrix mat0 + y * dstep of every image given, and to rows y (m0.r + 1) .. of `pscale` [matrix][plane][s | 1 / s].
struct PackJob {
  const float* theta; MatRef m0; long mstride; int nmat;
  int NBL; float scale;
  int mat0 = 0, dstep = 1;
  PlanePair split, half, compact;
  int compact_half = 0;           // the compact set's element: bf16 (mixed_bfloat16) or half (mixed_float16)
  float* pscale = nullptr;
};
// split + half: k_pack16b_dual (the scales found in the kernel).  half alone: k_plane_scales, k_pack16b.  split alone: k_pack16b.
// compact: a k_pack16b launch of its own, last
void launch_pack_planes(const PackJob& job, hipStream_t st);
void launch_pack_phi(const float* theta, long w_off, int n, int sop, void* WPF, void* WPB, hipStream_t st);
void launch_pack16(const float* theta, const MatRef& m, int NBL, f32x4* WF, f32x4* WB, hipStream_t st);
// forward image alone of matrix m of `nbatch` (<= 65535) parameter vectors `tstride` floats apart: entry y -> WF + y dstride_f32x4
void launch_pack16_fwd_batch(const float* theta, const MatRef& m, long tstride, int nbatch, int NBL, f32x4* WF, long dstride_f32x4,
                             hipStream_t st);
void launch_pack(const float* theta, const MatRef& m, int NBI, int NBO, f32x4* WF, f32x4* WB, hipStream_t st);
