// k_jac_snap.hip -- the snapshot forms of the tangent kernel (k_jac<.., SNAP>, k_jac_dev.h; nif_snapshot_derivatives*):
// T <= 65535 combined r = 0 nets in one launch, blockIdx.y the snapshot.  `a` is the net of the first snapshot (theta + off_bh = the
// slot vectors [T][po], WF = the planes [T][nh], snap_off / snap_M / snap_wstride set), a.B the longest snapshot's points; the
// device's workgroups are shared by the T snapshots.  Outputs are indexed by the call's point numbering, as the point-wise launches
// index them.
#include "k_jac_dev.h"

static void launch_jac_snap_impl(JacArgs& J, bool hess, long T, hipStream_t st) {
  const SNetArgs& a = J.s;
  const int NBL = snet3_nbl(a.n);
  const long ngroups = (2 * ((a.B + 31) / 32) + 3) / 4;
  const long cap = NBL <= 4 ? 512 : 256;
  long per = (cap + T - 1) / T;
  if (per > ngroups) per = ngroups;
  dim3 grid((unsigned)(per < 1 ? 1 : per), (unsigned)T), block(256);
  const size_t shm = jac_shmem(a, &J.one_buf);
#define JLK(K_)                                                                                                            \
  {                                                                                                                        \
    if (shm > 48 * 1024) (void)hipFuncSetAttribute((const void*)K_, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm); \
    hipLaunchKernelGGL(K_, grid, block, shm, st, J);                                                                       \
  }
#define JL(NBL_, ACT_, MODE_) \
  { if (hess) JLK((k_jac<NBL_, ACT_, MODE_, true, true>)) else JLK((k_jac<NBL_, ACT_, MODE_, false, true>)) }
#define JK(NBL_) \
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
#undef JLK
}
// ns coordinate seeds (order 1): columns x0 .. x0 + ns of dydx [n][so][nx_total]
void launch_jac_snap(const SNetArgs& a, long T, int ns, const int* seeds, int nx_total, int x0, float* dydx, hipStream_t st) {
  JacArgs J;
  J.s = a; J.ns = ns; J.nx_total = nx_total; J.x0 = x0; J.dydx = dydx; J.hj = J.hk = 0; J.d2ydx2 = nullptr;
  for (int d = 0; d < NIF_JAC_MAXSEED; ++d) { J.seed[d] = d < ns ? seeds[d] : 0; J.ZD[d] = nullptr; }
  launch_jac_snap_impl(J, false, T, st);
}
// the coordinate pair (seed_j at x position hj, seed_k at hk) of the Hessian, as launch_hess
void launch_hess_snap(const SNetArgs& a, long T, int seed_j, int seed_k, int hj, int hk, int nx_total, float* dydx, float* d2ydx2,
                      hipStream_t st) {
  JacArgs J;
  J.s = a; J.ns = 3; J.nx_total = nx_total; J.x0 = 0; J.dydx = dydx; J.hj = hj; J.hk = hk; J.d2ydx2 = d2ydx2;
  J.seed[0] = seed_j; J.seed[1] = seed_k; J.seed[2] = 0;
  J.ZD[0] = J.ZD[1] = J.ZD[2] = nullptr;
  launch_jac_snap_impl(J, true, T, st);
}
