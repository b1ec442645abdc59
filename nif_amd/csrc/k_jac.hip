// k_jac.hip -- JacobianLayer / HessianLayer for the hypernetwork classes: the point-wise launches of the tangent kernel (k_jac_dev.h)
#include "k_jac_dev.h"

static void launch_jac_impl(JacArgs& J, bool hess, hipStream_t st);
void launch_jac(const SNetArgs& a, int ns, const int* seeds, const float* const* zd, int nx_total, int x0, float* dydx,
                hipStream_t st) {
  JacArgs J;
  J.s = a; J.ns = ns; J.nx_total = nx_total; J.x0 = x0; J.dydx = dydx; J.hj = J.hk = 0; J.d2ydx2 = nullptr;
  for (int d = 0; d < NIF_JAC_MAXSEED; ++d) { J.seed[d] = d < ns ? seeds[d] : 0; J.ZD[d] = d < ns ? zd[d] : nullptr; }
  launch_jac_impl(J, false, st);
}
// one coordinate pair (seed_j at x position hj, seed_k at hk) of the Hessian: fills columns hj, hk of dydx and the entries
// (hj, hk), (hk, hj) of d2ydx2 [B][so][nx][nx]
void launch_hess(const SNetArgs& a, int seed_j, int seed_k, int hj, int hk, int nx_total, float* dydx, float* d2ydx2, hipStream_t st,
                 const float* zd_j, const float* zd_k, const float* zdd) {
  JacArgs J;
  J.s = a; J.ns = 3; J.nx_total = nx_total; J.x0 = 0; J.dydx = dydx; J.hj = hj; J.hk = hk; J.d2ydx2 = d2ydx2;
  J.seed[0] = seed_j; J.seed[1] = seed_k;
  J.seed[2] = zdd ? -1 : 0;          // stream 2 carries z'' like a parameter seed carries z' (bias / partial-product terms)
  J.ZD[0] = seed_j < 0 ? zd_j : nullptr; J.ZD[1] = seed_k < 0 ? zd_k : nullptr; J.ZD[2] = zdd;
  launch_jac_impl(J, true, st);
}
// shapes the Jacobian / Hessian kernels take: one 16-point-tile plane (and the small hyper-vectors) must fit the LDS
bool jac_supported(const SNetArgs& a) {
  if (a.n > 128) return false;
  const int NBL = snet3_nbl(a.n);
  const size_t plane = (size_t)NBL * NBL * 256;
  const size_t sm_tot = (((size_t)(a.r + 1) * a.nsm) + 3) & ~(size_t)3;
  return (plane + sm_tot + 4 * (size_t)(1 + NIF_JAC_MAXSEED) * a.r * 16 + 8) * sizeof(float) <= 160u * 1024u;
}
static void launch_jac_impl(JacArgs& J, bool hess, hipStream_t st) {
  const SNetArgs& a = J.s;
  const int NBL = snet3_nbl(a.n);
  const long nt16 = 2 * ((a.B + 31) / 32);
  const long ngroups = (nt16 + 3) / 4;
  const long cap = NBL <= 4 ? 512 : 256;
  dim3 grid((unsigned)(ngroups < cap ? ngroups : cap)), block(256);
  const size_t shm = jac_shmem(a, &J.one_buf);
#define JL(NBL_, ACT_, MODE_)                                                                                        \
  {                                                                                                                  \
    if (hess) {                                                                                                      \
      if (shm > 48 * 1024)                                                                                           \
        (void)hipFuncSetAttribute((const void*)k_jac<NBL_, ACT_, MODE_, true>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                  (int)shm);                                                                         \
      hipLaunchKernelGGL((k_jac<NBL_, ACT_, MODE_, true>), grid, block, shm, st, J);                                 \
    } else {                                                                                                         \
      if (shm > 48 * 1024)                                                                                           \
        (void)hipFuncSetAttribute((const void*)k_jac<NBL_, ACT_, MODE_>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                  (int)shm);                                                                         \
      hipLaunchKernelGGL((k_jac<NBL_, ACT_, MODE_>), grid, block, shm, st, J);                                       \
    }                                                                                                                \
  }
#define JK(NBL_)                                                      \
  if (a.nif_skip) JL(NBL_, -1, 2) else if (a.res) JL(NBL_, ACT_SINE, 1) else JL(NBL_, ACT_SINE, 0)
  switch (NBL) {
    case 1: JK(1) break;
    case 2: JK(2) break;
    case 3: JK(3) break;
    case 4: JK(4) break;
    case 6: JK(6) break;
    default: JK(8) break;
  }
#undef JK
#undef JL
}
