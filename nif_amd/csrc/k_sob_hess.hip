// k_sob_hess.hip -- the Sobolev step kernel (k_sob_dev.h) in its second-order form (HESS): one coordinate pair (j, k) of
// HessianLayer as a trained output (reference nif/layers/gradient.py:130-180, :234-261).  Training only (predict() takes k_jac<HESS>),
// fp32 policy, NIFMultiScale with or without resblocks and the last-layer class (LL); the general 3-seed form: 1 + 3 streams, the
// act'(a) ring of cos / sin (no sign-bit register), the LDS and register budget of the first-order 3-seed step.
#include "k_sob_dev.h"

void launch_sob_hess(const SobArgs& J, bool bf, int nblk, size_t shm, hipStream_t st) {
  const SNetArgs& a = J.s;
  const int NBL = snet3_nbl(a.n);
  dim3 grid(nblk), block(256);
#define SHL(NBL_, MODE_, BF_, LL_)                                                                                      \
  {                                                                                                                     \
    if (shm > 48 * 1024)                                                                                                \
      (void)hipFuncSetAttribute((const void*)k_sob<NBL_, MODE_, true, BF_, false, NIF_SOB_MAXSEED, false, LL_, true>,   \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);                                  \
    hipLaunchKernelGGL((k_sob<NBL_, MODE_, true, BF_, false, NIF_SOB_MAXSEED, false, LL_, true>), grid, block, shm, st, J); \
  }
#define SHK(NBL_, BF_)                                                                  \
  if (a.ll) { if (a.res) SHL(NBL_, 1, BF_, true) else SHL(NBL_, 0, BF_, true) }          \
  else { if (a.res) SHL(NBL_, 1, BF_, false) else SHL(NBL_, 0, BF_, false) }
  switch (NBL) {
    case 1: SHK(1, 0) break;
    case 3: SHK(3, 0) break;
    case 2: if (bf) { SHK(2, 1) } else { SHK(2, 0) } break;
    case 4: if (bf) { SHK(4, 1) } else { SHK(4, 0) } break;
    case 6: if (bf) { SHK(6, 1) } else { SHK(6, 0) } break;
    default: SHK(8, 0) break;
  }
#undef SHK
#undef SHL
}
