// k_pack.hip -- the packers: theta -> the plane images of k_pack_dev.h (layouts, split rules and the scale rule are stated there).
//   k_pack16b        one 16-bit set of a batch of matrices.  mode 0: the split groups; 1 / 2 (the policies' COMPACT set, late r4): bf16(x) /
//                    half(x), a third / half of the split planes' bytes; 3 (r5): the EXACT-PRODUCT HALF planes on k_plane_scales' powers of
//                    two.  hi.hi + hi.lo + lo.hi then carry an fp32 product: measured on MI355X 2.8e-8 rms / 2.1e-7 max of sum|a_k b_k| at
//                    K = 64 (the bf16 6-product form: 2.7e-8 / 2.9e-7, the f32-input MFMA: 3.9e-8 / 4.0e-7; tools/exp/f16_split_mfma.hip,
//                    profiles/r05_f16_probe.txt) at HALF the matrix work and two thirds of the plane bytes
//   k_plane_scales   the half planes' powers of two, one workgroup per (plane, matrix): the snapshot path
//   k_pack16b_dual   modes 0 and 3 of a batch in ONE launch, the scales found in the kernel: the training step's packer
//   k_pack_phi       the phi layer of the last-layer class;   k_pack16, k_pack: the fp32 planes, packed on demand
// blockIdx.y = matrix j of a batch of equally shaped matrices `mstride` slots apart (the hidden hyper-matrices).
#include "k_pack_dev.h"

// element e of direction `fwd` of a 16-bit set with ns splits: its value before the split, and the split it takes
__device__ __forceinline__ float pack16b_elem(const float* __restrict__ theta, const MatRef& m, long e, long per_plane, int ns, int NBL,
                                              bool fwd, float scale, int& k, int& s) {
  k = (int)(e / per_plane);
  int slot, row;
  pack_decode(e - (long)k * per_plane, ns, NBL, s, slot, row);
  return pack_theta(theta, m, k, fwd ? slot : row, fwd ? row : slot, scale);
}

__global__ void k_pack16b(const float* __restrict__ theta, MatRef m, long mstride, int NBL, __bf16* __restrict__ WF,
                          __bf16* __restrict__ WB, long fstride, long bstride, float scale, int mode, const float* __restrict__ pscale) {
  m.base_k += (long)blockIdx.y * mstride; m.base_last += (long)blockIdx.y * mstride;
  WF += (long)blockIdx.y * fstride; WB += (long)blockIdx.y * bstride;
  const PlaneSet set = mode == 3 ? PLANES_HALF : (mode ? PLANES_COMPACT : PLANES_SPLIT);
  const long fwd_plane = plane_elems(set, PLANE_FWD, NBL), bwd_plane = plane_elems(set, PLANE_BWD, NBL);
  const long total_f = fwd_plane * (m.r + 1), total_b = bwd_plane * (m.r + 1);
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total_f + total_b; idx += (long)gridDim.x * blockDim.x) {
    const bool fwd = idx < total_f;
    const long e = fwd ? idx : idx - total_f;
    int k, s;
    float x = pack16b_elem(theta, m, e, fwd ? fwd_plane : bwd_plane, plane_splits(set, fwd ? PLANE_FWD : PLANE_BWD), NBL, fwd, scale, k, s);
    if (mode == 3) x *= pscale[plane_scale_index(blockIdx.y, m.r, k)];
    if (mode >= 2) reinterpret_cast<_Float16*>(fwd ? WF : WB)[e] = mode == 3 ? pack_split_half(x, s) : pack_sat_half(x);
    else (fwd ? WF : WB)[e] = pack_split_bf16(x, s);
  }
}
__global__ void k_plane_scales(const float* __restrict__ theta, MatRef m, long mstride, float scale, float* __restrict__ pscale) {
  m.base_k += (long)blockIdx.y * mstride; m.base_last += (long)blockIdx.y * mstride;
  __shared__ float red[256];
  const int sh = plane_scale_shift(plane_absmax(theta, m, blockIdx.x, scale, red));
  if (threadIdx.x == 0) {
    float* ps = pscale + plane_scale_index(blockIdx.y, m.r, blockIdx.x);
    ps[0] = ldexpf(1.0f, sh); ps[1] = ldexpf(1.0f, -sh);
  }
}
// r5: every workgroup of a half plane takes the maximum over its plane itself -- <= 16 K cached words -- instead of waiting for a
// k_plane_scales launch; all of them arrive at the same power of two, the thread holding the plane's first forward unit writes it for
// the consumers: three launches of ~5 us per training step -> one.  Index space [split elements | half elements], both multiples of
// the workgroup's 256 elements, so a workgroup's elements of one loop trip lie in ONE part and ONE plane.
__global__ __launch_bounds__(256) void k_pack16b_dual(const float* __restrict__ theta, MatRef m, long mstride, int NBL,
                                                     __bf16* __restrict__ WF, __bf16* __restrict__ WB, long fstride, long bstride,
                                                     _Float16* __restrict__ WFx, _Float16* __restrict__ WBx, long fxstride, long bxstride,
                                                     float scale, float* __restrict__ pscale) {
  m.base_k += (long)blockIdx.y * mstride; m.base_last += (long)blockIdx.y * mstride;
  WF += (long)blockIdx.y * fstride; WB += (long)blockIdx.y * bstride;
  WFx += (long)blockIdx.y * fxstride; WBx += (long)blockIdx.y * bxstride;
  const long fwd0 = plane_elems(PLANES_SPLIT, PLANE_FWD, NBL), bwd0 = plane_elems(PLANES_SPLIT, PLANE_BWD, NBL);
  const long px = plane_elems(PLANES_HALF, PLANE_FWD, NBL);       // (either direction)
  const long tot0 = (fwd0 + bwd0) * (m.r + 1), totx = 2 * px * (m.r + 1);
  __shared__ float red[256];
  int k_have = -1;
  float s_have = 1.0f;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < tot0 + totx; idx += (long)gridDim.x * blockDim.x) {
    const bool half = idx >= tot0;
    const long i2 = half ? idx - tot0 : idx;
    const long tf = half ? px * (m.r + 1) : fwd0 * (m.r + 1);
    const bool fwd = i2 < tf;
    const long e = fwd ? i2 : i2 - tf;
    const PlaneSet set = half ? PLANES_HALF : PLANES_SPLIT;
    const long per_plane = half ? px : (fwd ? fwd0 : bwd0);
    int k, s;
    float x = pack16b_elem(theta, m, e, per_plane, plane_splits(set, fwd ? PLANE_FWD : PLANE_BWD), NBL, fwd, scale, k, s);
    if (half) {
      if (k != k_have) {        // (uniform over the workgroup: see above)
        const int sh = plane_scale_shift(plane_absmax(theta, m, k, scale, red));
        s_have = ldexpf(1.0f, sh); k_have = k;
        if (fwd && e == (long)k * per_plane && pscale) {
          float* ps = pscale + plane_scale_index(blockIdx.y, m.r, k);
          ps[0] = s_have; ps[1] = ldexpf(1.0f, -sh);
        }
      }
      (fwd ? WFx : WBx)[e] = pack_split_half(x * s_have, s);
    } else (fwd ? WF : WB)[e] = pack_split_bf16(x, s);
  }
}
// phi layer of the last-layer class: dense W[n][sop], sop <= 32 (two 16-output blocks)
__global__ void k_pack_phi(const float* __restrict__ theta, long w_off, int n, int sop, int NBL, __bf16* __restrict__ WPF,
                           __bf16* __restrict__ WPB) {
  const MatRef m = {0, 0, 0, w_off, sop, n, sop};
  const long total_f = plane_elems(PLANES_PHI, PLANE_FWD, NBL), total_b = plane_elems(PLANES_PHI, PLANE_BWD, NBL);
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total_f + total_b; idx += (long)gridDim.x * blockDim.x) {
    const bool fwd = idx < total_f;
    const PlaneDir d = fwd ? PLANE_FWD : PLANE_BWD;
    const long e = fwd ? idx : idx - total_f;
    int s, slot, row;
    pack_decode(e, plane_splits(PLANES_PHI, d), plane_chunk_blocks(PLANES_PHI, d, NBL), s, slot, row);
    (fwd ? WPF : WPB)[e] = pack_split_bf16(pack_theta(theta, m, 0, fwd ? slot : row, fwd ? row : slot, 1.0f), s);
  }
}
// the fp32 planes: one loop for both tile sizes.  T32 = false: 16-row blocks (k_snet3, k_jac, k_sob); true: 32-row blocks (k_snet, k_pnet)
// element idx of the forward (fwd) or adjoint image of all r + 1 planes
template <bool T32>
__device__ __forceinline__ float pack_f32_elem(const float* __restrict__ theta, const MatRef& m, int NBI, int NBO, long idx, bool fwd) {
  const long per_plane = (long)NBI * NBO * (T32 ? 1024 : 256);
  const int k = (int)(idx / per_plane);
  const long rem = idx - (long)k * per_plane;
  const int lane = (rem >> 2) & 63, blk = (int)(rem >> (T32 ? 10 : 8));
  const int v = T32 ? 4 * (int)((rem >> 8) & 3) + (int)(rem & 3) : (int)(rem & 3);
  const int kk = T32 ? fmap(v, lane >> 5) : 4 * (lane >> 4) + v, rr = T32 ? lane & 31 : lane & 15, W = T32 ? 32 : 16;
  if (fwd) {  // forward plane: blk = ob*NBI + ib
    const int ob = blk / NBI, ib = blk % NBI;
    return pack_theta(theta, m, k, W * ib + kk, W * ob + rr, 1.0f);
  }
  // adjoint plane: blk = ib*NBO + ob   (output blocks of U are the in-feature blocks)
  const int ib = blk / NBO, ob = blk % NBO;
  return pack_theta(theta, m, k, W * ib + rr, W * ob + kk, 1.0f);
}
template <bool T32>
__device__ __forceinline__ void pack_f32(const float* __restrict__ theta, const MatRef& m, int NBI, int NBO, float* __restrict__ WF,
                                         float* __restrict__ WB) {
  const long total = (long)NBI * NBO * (T32 ? 1024 : 256) * (m.r + 1);
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    WF[idx] = pack_f32_elem<T32>(theta, m, NBI, NBO, idx, true);
    WB[idx] = pack_f32_elem<T32>(theta, m, NBI, NBO, idx, false);
  }
}
// The forward tiles16 image alone of matrix m of gridDim.y parameter vectors `tstride` floats apart (the combined nets of k_jac_snap:
// slot vectors w_t, m dense): entry y -> WF + y dstride floats
__global__ void k_pack16_fwd_batch(const float* __restrict__ theta, MatRef m, long tstride, int NBL, float* __restrict__ WF, long dstride) {
  const float* th = theta + (long)blockIdx.y * tstride;
  float* wf = WF + (long)blockIdx.y * dstride;
  const long total = plane_elems(PLANES_T16, PLANE_FWD, NBL) * (m.r + 1);
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x)
    wf[idx] = pack_f32_elem<false>(th, m, NBL, NBL, idx, true);
}
__global__ void k_pack16(const float* __restrict__ theta, MatRef m, int NBL, float* __restrict__ WF, float* __restrict__ WB) {
  pack_f32<false>(theta, m, NBL, NBL, WF, WB);
}
__global__ void k_pack(const float* __restrict__ theta, MatRef m, int NBI, int NBO, float* __restrict__ WF, float* __restrict__ WB) {
  pack_f32<true>(theta, m, NBI, NBO, WF, WB);
}

// ---- launchers -----------------------------------------------------------------------------------
static int pack_grid(long total, int cap) { const long g = (total + 255) / 256; return (int)(g < cap ? g : cap); }
void launch_pack_planes(const PackJob& j, hipStream_t st) {
  const int np = j.m0.r + 1;
  auto mat = [&](PlaneSet s, PlaneDir d) { return plane_elems(s, d, j.NBL) * np; };                // elements per matrix
  auto stride = [&](PlaneSet s, PlaneDir d) { return j.dstep * mat(s, d); };        // ... between batch entries
  auto at = [&](void* base, PlaneSet s, PlaneDir d) { return (char*)base + (size_t)j.mat0 * mat(s, d) * plane_elem_bytes(s); };
  const long split_all = mat(PLANES_SPLIT, PLANE_FWD) + mat(PLANES_SPLIT, PLANE_BWD);
  // (one grid size for every mode of k_pack16b: the split set's)
  auto pack16b = [&](const PlanePair& p, PlaneSet s, int mode) {
    hipLaunchKernelGGL(k_pack16b, dim3(pack_grid(split_all, 4096), j.nmat), dim3(256), 0, st, j.theta, j.m0, j.mstride, j.NBL,
                       (__bf16*)at(p.F, s, PLANE_FWD), (__bf16*)at(p.B, s, PLANE_BWD), stride(s, PLANE_FWD), stride(s, PLANE_BWD), j.scale,
                       mode, j.pscale);
  };
  if (j.split.F && j.half.F)
    hipLaunchKernelGGL(k_pack16b_dual, dim3(pack_grid(split_all + mat(PLANES_HALF, PLANE_FWD) + mat(PLANES_HALF, PLANE_BWD), 4096), j.nmat),
                       dim3(256), 0, st, j.theta, j.m0, j.mstride, j.NBL, (__bf16*)at(j.split.F, PLANES_SPLIT, PLANE_FWD),
                       (__bf16*)at(j.split.B, PLANES_SPLIT, PLANE_BWD), stride(PLANES_SPLIT, PLANE_FWD), stride(PLANES_SPLIT, PLANE_BWD),
                       (_Float16*)at(j.half.F, PLANES_HALF, PLANE_FWD), (_Float16*)at(j.half.B, PLANES_HALF, PLANE_BWD),
                       stride(PLANES_HALF, PLANE_FWD), stride(PLANES_HALF, PLANE_BWD), j.scale, j.pscale);
  else if (j.half.F) {
    hipLaunchKernelGGL(k_plane_scales, dim3(np, j.nmat), dim3(256), 0, st, j.theta, j.m0, j.mstride, j.scale, j.pscale);
    pack16b(j.half, PLANES_HALF, 3);
  } else if (j.split.F) pack16b(j.split, PLANES_SPLIT, 0);
  if (j.compact.F) pack16b(j.compact, PLANES_COMPACT, j.compact_half ? 2 : 1);
}
void launch_pack_phi(const float* theta, long w_off, int n, int sop, void* WPF, void* WPB, hipStream_t st) {
  hipLaunchKernelGGL(k_pack_phi, dim3(64), dim3(256), 0, st, theta, w_off, n, sop, plane_nbl(n), (__bf16*)WPF, (__bf16*)WPB);
}
void launch_pack16(const float* theta, const MatRef& m, int NBL, f32x4* WF, f32x4* WB, hipStream_t st) {
  const int grid = pack_grid(plane_elems(PLANES_T16, PLANE_FWD, NBL) * (m.r + 1), 2048);
  hipLaunchKernelGGL(k_pack16, dim3(grid), dim3(256), 0, st, theta, m, NBL, (float*)WF, (float*)WB);
}
void launch_pack16_fwd_batch(const float* theta, const MatRef& m, long tstride, int nbatch, int NBL, f32x4* WF, long dstride_f32x4,
                             hipStream_t st) {
  const int grid = pack_grid(plane_elems(PLANES_T16, PLANE_FWD, NBL) * (m.r + 1), 64);
  hipLaunchKernelGGL(k_pack16_fwd_batch, dim3(grid, nbatch), dim3(256), 0, st, theta, m, tstride, NBL, (float*)WF, dstride_f32x4 * 4);
}
void launch_pack(const float* theta, const MatRef& m, int NBI, int NBO, f32x4* WF, f32x4* WB, hipStream_t st) {
  const int grid = pack_grid((long)NBI * NBO * 1024 * (m.r + 1), 2048);
  hipLaunchKernelGGL(k_pack, dim3(grid), dim3(256), 0, st, theta, m, NBI, NBO, (float*)WF, (float*)WB);
}
