// k_snet4.hip -- k_snet3 with every n x n product on the BF16 matrix cores at fp32 accuracy.
//
// gfx950 runs v_mfma_f32_16x16x32_bf16 at 16x the rate of the f32-input MFMAs (1024 vs 64 FLOP/clk/SIMD).
// An fp32 number is EXACTLY the sum of three bf16 numbers (8 + 8 + 8 significand bits, same exponent range):
//     x = x0 + x1 + x2 ,  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)
// and bf16 x bf16 products are exact in the fp32 accumulator, so
//     a.b  =  a0b0 + (a0b1 + a1b0) + (a0b2 + a2b0 + a1b1) + O(2^-24 |a||b|)
// Six MFMAs (small terms first) reproduce the fp32 product to 4.2e-8 rms / 4.3e-7 max of sum|a_k b_k| at K = 64 --
// slightly BETTER than v_mfma_f32_16x16x4_f32 itself (6.1e-8 / 5.9e-7; tools/exp/bf16_split_mfma.hip, measured
// on MI355X) -- in 6 x 16 = 96 matrix-pipe cycles per 16x16x32 block instead of 8 x 32 = 256.  The forward pass
// (predictions and loss, 1e-5 bar) uses the 6-product form; the data adjoint, whose bar is the gradient
// tolerance, the 3-product form (a0b0 + a0b1 + a1b0, 1.9e-6 rms) in 48 cycles.
//
// Weight planes are pre-split at pack time (k_pack.hip, layout in k_pack_dev.h) into bf16 A operands; the activation tile (B operand) is
// split once per layer in registers and shared by all r+1 planes: the per-point latent factor zt_k is applied
// to the PRODUCT (column scaling commutes with the GEMM).  Planes stream L2 -> LDS by DMA in K-step chunks
// (32 input features x all outputs: NBL x 3 KiB forward, NBL x 2 KiB adjoint), double buffered, one barrier per
// chunk -> 24 KiB of plane LDS per workgroup for the 64-wide net.
//
// Everything else (tiles, stashes, ring, first / last layer, loss, modes) is k_snet3's; see there.
#include "k_snet4_dev.h"

// ---- host side ---------------------------------------------------------------------------------
// floats per k of the LDS small-vector image (last-layer class: + last_layer_bias and the rl x rl map)
int snet4_nsm_ll(int si, int sop, int nh, int n, int sou, int rl) {
  return snet3_nsm(si, sop, nh, n) + ((sou + 3) & ~3) + ((rl * rl + 3) & ~3);
}
__global__ void k_ll_slots(const float* __restrict__ theta, LLSlotMap m, float* __restrict__ slots) {
  for (int sgi = blockIdx.y; sgi < m.nseg; sgi += gridDim.y)
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < m.seg[sgi].len; e += (long)gridDim.x * blockDim.x)
      slots[m.seg[sgi].dst + e] = theta[m.seg[sgi].src + e];
}
void launch_ll_slots(const float* theta, const LLSlotMap& m, float* slots, hipStream_t st) {
  hipLaunchKernelGGL(k_ll_slots, dim3(16, m.nseg), dim3(256), 0, st, theta, m, slots);
}
bool snet4_supported(const SNetArgs& a) {
  const int NBL = snet3_nbl(a.n);
  if (a.n > 128 || (NBL & 1) || a.nh < 1) return false;
  if (a.ll && a.so > 32) return false;          // the phi layer runs as two 16-output MFMA blocks
  return snet4_shmem(a, NBL) <= 160u * 1024u;
}
// plain SIREN: the act'(a) ring is not needed (the cosine's sign rides in the stashed sine, any depth / width)
bool snet4_sign_ring(const SNetArgs& a) { return !a.nif_skip; }
// does the training launch of `a` write its hidden-layer dL/da stash rows in bf16?  The kernel's own condition (`PR && NBL != 6 &&
// A.da_bf16` at the store), stated once next to it: the host derives the consumers' GwArgs.da_bf16 from THIS, not from a second copy
// of the dispatch predicate
bool snet4_writes_da_bf16(const SNetArgs& a) { return a.da_bf16 != 0 && a.prec == 1 && snet3_nbl(a.n) != 6; }
// ... and the hidden matrices' INPUT rows as 16-bit phases: the kernel's PHC condition (plain tagged-sine training form, PR = 1, NBL = 8)
bool snet4_writes_h_ph16(const SNetArgs& a) { return a.h_ph16 != 0 && a.prec == 1 && snet3_nbl(a.n) == 8 && !a.res && !a.nif_skip; }
int launch_snet4(const SNetArgs& a, bool train, bool query_only, hipStream_t st) {
  const int NBL = snet3_nbl(a.n);
  const long nt16 = 2 * ((a.B + 31) / 32);
  const long ngroups = (nt16 + 3) / 4;
  long cap = NBL <= 4 ? 256 * NIF_S4_OCC : 256 * NIF_S4_OCC_WIDE;
  if (NBL == 8 && a.ll && train && !a.res) cap = 256 * NIF_S4_OCC_LL8;
  if (a.wg_cap > 0 && a.wg_cap < cap) cap = a.wg_cap;
  const int nblk = (int)(ngroups < cap ? ngroups : cap);
  if (query_only) return nblk;
  dim3 grid(nblk), block(256);
  const size_t shm = snet4_shmem(a, NBL);
  SNetArgs h = a;
  const int pr = snet4_pr(a);
  if (a.prec != 0) { h.WF4 = a.WF4h; h.WB4 = a.WB4h; }      // the policies' compact plane set (k_pack16b mode 1 / 2)
  if (pr == 2) {      // mixed_float16: the PR = 2 instantiations (k_snet4_f16.hip)
    launch_snet4_f16(h, train, nblk, shm, st);
    return nblk;
  }
  if (pr == 3) {      // r5: fp32-exact products on half pairs -- every SIREN form (k_snet4_x16.hip); the bf16-split forms below are class NIF's
    h.WF4 = a.WF4x; h.WB4 = a.WB4x;
    launch_snet4_x16(h, train, nblk, shm, st);
    return nblk;
  }
#define S4L(NBL_, TR_, ACT_, MODE_, SGN_, LL_, PR_)                                                                    \
  {                                                                                                                 \
    if (shm > 48 * 1024)                                                                                            \
      (void)hipFuncSetAttribute((const void*)k_snet4<NBL_, TR_, ACT_, MODE_, SGN_, LL_, PR_>,                            \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);                              \
    hipLaunchKernelGGL((k_snet4<NBL_, TR_, ACT_, MODE_, SGN_, LL_, PR_>), grid, block, shm, st, h);                      \
  }
// PR_: the mixed_bfloat16 policy (ONE bf16 product per n x n operand pair); plain SIREN training always takes the tagged-sine form
#define S4M(NBL_, LL_, PR_)                                                                                         \
  if (a.nif_skip) { if (train) S4L(NBL_, true, -1, 2, false, LL_, PR_) else S4L(NBL_, false, -1, 2, false, LL_, PR_) }    \
  else if (a.res) { if (train) S4L(NBL_, true, ACT_SINE, 1, true, LL_, PR_) else S4L(NBL_, false, ACT_SINE, 1, false, LL_, PR_) } \
  else if (train) S4L(NBL_, true, ACT_SINE, 0, true, LL_, PR_)                                                      \
  else S4L(NBL_, false, ACT_SINE, 0, false, LL_, PR_)
#define S4N(NBL_, LL_, PR_)   /* last-layer class: no NIF skip form */                                              \
  if (a.res) { if (train) S4L(NBL_, true, ACT_SINE, 1, true, LL_, PR_) else S4L(NBL_, false, ACT_SINE, 1, false, LL_, PR_) } \
  else if (train) S4L(NBL_, true, ACT_SINE, 0, true, LL_, PR_)                                                      \
  else S4L(NBL_, false, ACT_SINE, 0, false, LL_, PR_)
// (PR = 0, the exact bf16 splits: class NIF alone since r5 -- its activations are not bounded, the half pairs of the SIREN forms need |h| <= 1;
//  a SIREN net reaches this point with PR = 0 only when the half planes are not packed, which nif_api never does: refused below)
#define S4(NBL_)                                                            \
  if (a.ll && a.prec == 1) { S4N(NBL_, true, true) }                        \
  else if (a.prec == 1) { S4M(NBL_, false, true) }                          \
  else if (a.nif_skip) { if (train) S4L(NBL_, true, -1, 2, false, false, false) else S4L(NBL_, false, -1, 2, false, false, false) } \
  else return -1;
#ifdef NIF_S4_DEV      // ISA work (tools/isa_hist.py): only the benchmark shape's training / inference instantiations
  if (train) S4L(4, true, ACT_SINE, 0, true, false, false) else S4L(4, false, ACT_SINE, 0, false, false, false)
#else
  switch (NBL) {
    case 2: S4(2) break;
    case 4: S4(4) break;
    case 6: S4(6) break;
    default: S4(8) break;
  }
#endif
#undef S4
#undef S4N
#undef S4M
#undef S4L
  return nblk;
}
