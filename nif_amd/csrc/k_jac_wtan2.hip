// k_jac_wtan2.hip -- the second-order weight-tangent kernel of nif_snapshot_param_second_derivatives* (DESIGN 2.10): a sibling of
// k_jac_wt (k_jac_wtan.hip) in a translation unit of its own, so that every k_jac and k_jac_wt instantiation keeps the code it has.
//
// Over a snapshot t the latent z_t, two directions delta_a, delta_b in latent space and a second direction dd_ab are constant.  The
// snapshot's net is the dense r = 0 net of w_t; its first tangents are carried by the slot vectors wd_a = sum_k
// delta_a,k M^(k), wd_b, and the second tangent of the pair by ONE more, wdd = sum_k dd_ab,k M^(k).  One launch is one
// pair; the streams are h, h'_a, h'_b, h'' -- the accumulator set of k_jac<.., HESS>:
//
//   first layer   a'_d = w0 x W1'_d + b1'_d          a'' = w0 x W1'' + b1''
//                 coordinate seed j: a'_x = w0 W1[j,:],  a''_ax = w0 W1'_a[j,:]
//   hidden j      a'_d = w0 (h'_d W + h W'_d) + b'_d
//                 a''  = w0 (h'' W + h'_a W'_b + h'_b W'_a + h W'') + b''
//                 h''  = f'(a) a'' + f''(a) a'_a a'_b, then the layer's MODE rule as k_jac<HESS> applies it to its second-order stream
//   last          u''  = h'' Wl + h'_a Wl'_b + h'_b Wl'_a + h Wl'' + bl''
//
// FORM (compile time) is the plane set of a pair, so that no form multiplies a plane of zeros:
//   WT2_GEN   a < b          planes W, W'_a, W'_b (, W'')    4 + 2 + 2 (+ 1) products per hidden layer
//   WT2_DIAG  a = b          planes W, W'_a (, W'')          streams h, h', h'': 3 + 2 (+ 1), the cross term as (2 h') W'
//   WT2_MIX   a x coordinate planes W, W'_a                  4 + 2: a coordinate moves no weight, so there is no W'_x and no W''
// has_dd (wave-uniform launch argument): the pair has a second direction; a latent call without d2latent has no W'' plane at all.
// The image of a snapshot holds `pstride` planes per hidden layer; pl[] names the ones this pair walks, in the order above.  The
// small-vector LDS image holds four vectors [w | wd_a | wd_b | wdd] under k_jac_wt's rule at three streams.  A pair's arithmetic
// depends on nothing but its own operands: not on the other directions of the call, nor on the snapshot's place in the launch.
#include "k_jac_dev.h"

enum { WT2_GEN = 0, WT2_DIAG = 1, WT2_MIX = 2 };

struct JacWt2Args {
  SNetArgs s;               // as launch_jac_wt: theta + off_bh = the slot vectors w_t [T][po], WF = the plane images, snap_* set
  const float* wd[3];       // tangent slot vectors [T][po]: wd_a, wd_b (WT2_GEN), wdd (has_dd)
  int pl[4];                // planes of a hidden layer this pair walks: W, W'_a, then W'_b (WT2_GEN), then W'' (has_dd)
  int npl;                  // how many of them
  int pstride;              // planes per hidden layer in the image
  int has_dd;
  int seed;                 // WT2_MIX: the coordinate
  int row, i0, i1;          // out [n][so][row]: the pair's value goes to columns i0 and i1 of its row (one value, both places)
  float* out;
  int one_buf;              // as JacArgs::one_buf
};

template <int NBL, int ACT, int MODE, int FORM>
__global__ __launch_bounds__(256, (NBL <= 4 ? 2 : 1)) void k_jac_wt2(JacWt2Args J) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const SNetArgs& A = J.s;
  constexpr int NT = 256, WAVES = 4;
  constexpr int PLANE = NBL * NBL * 256;
  static_assert(PLANE == plane_elems(PLANES_T16, PLANE_FWD, NBL), "k_pack_dev.h");
  constexpr int PF4 = (PLANE / 4 + NT - 1) / NT;
  constexpr bool PEXACT = (PLANE / 4) % NT == 0;
  constexpr int NP = 16 * NBL;
  constexpr bool GEN = FORM == WT2_GEN, DIAG = FORM == WT2_DIAG, MIX = FORM == WT2_MIX;
  // the snapshot of this workgroup, exactly as k_jac_wt rebases onto it
  const long ts = blockIdx.y;
  const long p0 = A.snap_off ? A.snap_off[ts] : ts * A.snap_M;
  const long NB = A.snap_off ? A.snap_off[ts + 1] - p0 : A.snap_M;
  if ((long)blockIdx.x >= (2 * ((NB + 31) / 32) + 3) / 4) return;      // no tile group of this snapshot for this slot (whole workgroup)
  const float* xin = A.snap_off ? A.xin + p0 * A.ncol : A.xin;
  const f32x4* WF = A.WF + ts * A.snap_wstride;
  float* out = J.out + p0 * A.so * J.row;

  const int tid = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, p = lane & 15, g = lane >> 4;
  const int n = A.n, nh = A.nh, si = A.si, so = A.so, nsm = A.nsm, npl = J.npl, pstride = J.pstride;
  const bool has_dd = !MIX && J.has_dd != 0;
  const long nt16 = 2 * ((NB + 31) / 32);
  const long ngroups = (nt16 + WAVES - 1) / WAVES;

  f32x4* planes = reinterpret_cast<f32x4*>(smem);
  const int one_buf = J.one_buf;
  float* sm = smem + (one_buf ? 1 : 2) * PLANE;      // [4][nsm]: w_t, wd_a, wd_b, wdd (an image the form does not read stays unwritten)
  const float* sm_a = sm + nsm;
  const float* sm_b = sm + 2 * nsm;
  const float* sm_dd = sm + 3 * nsm;
  const int o_w1 = 0, o_wl = si * NP, o_b1 = o_wl + so * NP, o_bh = o_b1 + NP, o_bl = o_bh + nh * NP;

  {
    const long s_wl = (long)si * n + (long)nh * n * n;
    const long s_b1 = s_wl + (long)n * so, s_bh = s_b1 + n, s_bl = s_bh + (long)nh * n;
    for (int idx = tid; idx < 4 * nsm; idx += NT) {
      const int k = idx / nsm, e = idx - k * nsm;
      if ((k == 2 && !GEN) || (k == 3 && !has_dd)) continue;
      const float* src = (k == 0 ? A.theta + A.off_bh : J.wd[k - 1]) + ts * A.po;
      float v = 0.f;
      if (e < o_wl) { const int dd = e / NP, f = e - dd * NP; if (f < n) v = src[(long)dd * n + f]; }
      else if (e < o_b1) { const int o = (e - o_wl) / NP, f = (e - o_wl) - o * NP; if (f < n) v = src[s_wl + (long)f * so + o]; }
      else if (e < o_bh) { const int f = e - o_b1; if (f < n) v = src[s_b1 + f]; }
      else if (e < o_bl) { const int j = (e - o_bh) / NP, f = (e - o_bh) - j * NP; if (f < n) v = src[s_bh + (long)j * n + f]; }
      else if (e < o_bl + so) v = src[s_bl + (e - o_bl)];
      sm[idx] = v;
    }
    if (nh > 0) {
      const f32x4* src = WF + (long)J.pl[0] * (PLANE / 4);
#pragma unroll
      for (int q = 0; q < PF4; ++q)
        if (PEXACT || tid + NT * q < PLANE / 4) planes[tid + NT * q] = src[tid + NT * q];
    }
  }
  __syncthreads();
  int gpar = 0;

  for (long tg = blockIdx.x; tg < ngroups; tg += gridDim.x) {
    const bool last_group = tg + gridDim.x >= ngroups;
    const long t16_raw = tg * WAVES + wid;
    const bool active = t16_raw < nt16;
    const long t16 = active ? t16_raw : nt16 - 1;
    const long pt = t16 * 16 + p;
    const bool valid = active && pt < NB;
    const long ptc = pt < NB ? pt : NB - 1;
    const float* xrow = xin + ptc * A.ncol + A.col0;

    // streams: h (primal), ha = h'_a, hb = h'_b (the coordinate's tangent in WT2_MIX; dead on the diagonal), h2 = h''
    f32x4 h[NBL], acc[NBL], ha[NBL], acca[NBL], hb[NBL], accb[NBL], h2[NBL], acc2[NBL];
    // ---- first layer ------------------------------------------------------------------------------------------------
    {
      const float* s0 = sm + 4 * g;
#pragma unroll
      for (int b = 0; b < NBL; ++b) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, sa = {0.f, 0.f, 0.f, 0.f};
        for (int dd = 0; dd < si; ++dd) {
          s += xrow[dd] * *reinterpret_cast<const f32x4*>(s0 + o_w1 + dd * NP + 16 * b);
          sa += xrow[dd] * *reinterpret_cast<const f32x4*>(sm_a + 4 * g + o_w1 + dd * NP + 16 * b);
        }
        acc[b] = A.omega * s + *reinterpret_cast<const f32x4*>(s0 + o_b1 + 16 * b);
        acca[b] = A.omega * sa + *reinterpret_cast<const f32x4*>(sm_a + 4 * g + o_b1 + 16 * b);
        if (GEN) {
          f32x4 sb = {0.f, 0.f, 0.f, 0.f};
          for (int dd = 0; dd < si; ++dd) sb += xrow[dd] * *reinterpret_cast<const f32x4*>(sm_b + 4 * g + o_w1 + dd * NP + 16 * b);
          accb[b] = A.omega * sb + *reinterpret_cast<const f32x4*>(sm_b + 4 * g + o_b1 + 16 * b);
        }
        if (MIX) {
          accb[b] = A.omega * *reinterpret_cast<const f32x4*>(s0 + o_w1 + J.seed * NP + 16 * b);
          acc2[b] = A.omega * *reinterpret_cast<const f32x4*>(sm_a + 4 * g + o_w1 + J.seed * NP + 16 * b);
        } else {
          f32x4 s2 = {0.f, 0.f, 0.f, 0.f};
          if (has_dd) {
            for (int dd = 0; dd < si; ++dd) s2 += xrow[dd] * *reinterpret_cast<const f32x4*>(sm_dd + 4 * g + o_w1 + dd * NP + 16 * b);
            s2 = A.omega * s2 + *reinterpret_cast<const f32x4*>(sm_dd + 4 * g + o_b1 + 16 * b);
          }
          acc2[b] = s2;
        }
      }
      f32x4 dv[NBL];
#pragma unroll
      for (int b = 0; b < NBL; ++b) {
        f32x4 d2;
#pragma unroll
        for (int v = 0; v < 4; ++v) d2[v] = act_d2<ACT>(A.act, acc[b][v]);
        h2[b] = d2 * acca[b] * (DIAG ? acca[b] : accb[b]);      // f''(a) a'_a a'_b; f'(a) a'' joins behind act16
      }
      act16<NBL, ACT>(A.act, acc, h, dv, n, g);
#pragma unroll
      for (int b = 0; b < NBL; ++b) {
        ha[b] = dv[b] * acca[b];
        if (!DIAG) hb[b] = dv[b] * accb[b];
        h2[b] = dv[b] * acc2[b] + h2[b];
      }
    }
    // ---- hidden layers: the pair's planes of each layer, in pl[]'s order ------------------------------------------------
    f32x4 ublk[MODE == 1 ? NBL : 1], ublka[MODE == 1 ? NBL : 1], ublkb[MODE == 1 ? NBL : 1], ublk2[MODE == 1 ? NBL : 1];
    for (int j = 0; j < nh; ++j) {
#pragma unroll
      for (int b = 0; b < NBL; ++b) {
        acc[b][0] = 0.f; acc[b][1] = 0.f; acc[b][2] = 0.f; acc[b][3] = 0.f;
        acca[b][0] = 0.f; acca[b][1] = 0.f; acca[b][2] = 0.f; acca[b][3] = 0.f;
        acc2[b][0] = 0.f; acc2[b][1] = 0.f; acc2[b][2] = 0.f; acc2[b][3] = 0.f;
        if (!DIAG) { accb[b][0] = 0.f; accb[b][1] = 0.f; accb[b][2] = 0.f; accb[b][3] = 0.f; }
      }
      for (int q = 0; q < npl; ++q) {
        // the plane after this one: the layer's next, the next layer's first, or (next tile group) the image's first again
        const bool wrap = q + 1 == npl && j + 1 == nh;
        const bool has_next = !wrap || !last_group;
        f32x4 pre[PF4];
        if (has_next) {
          const long nxt = wrap ? J.pl[0] : (q + 1 < npl ? (long)j * pstride + J.pl[q + 1] : (long)(j + 1) * pstride + J.pl[0]);
          const f32x4* src = WF + nxt * (PLANE / 4);
#pragma unroll
          for (int v = 0; v < PF4; ++v)
            if (PEXACT || tid + NT * v < PLANE / 4) pre[v] = src[tid + NT * v];
        }
        const f32x4* cur = planes + (one_buf ? 0 : (gpar & 1)) * (PLANE / 4);
        if (q == 0) {             // W: every stream
          mfma16<NBL, true>(cur, h, acc, lane);
          mfma16<NBL, true>(cur, ha, acca, lane);
          if constexpr (!DIAG) mfma16<NBL, true>(cur, hb, accb, lane);
          mfma16<NBL, true>(cur, h2, acc2, lane);
        } else if (q == 1) {      // W'_a: h into a'_a, the other tangent into a''
          mfma16<NBL, true>(cur, h, acca, lane);
          if constexpr (DIAG) {
            f32x4 t2[NBL];
#pragma unroll
            for (int b = 0; b < NBL; ++b) t2[b] = 2.0f * ha[b];
            mfma16<NBL, true>(cur, t2, acc2, lane);
          } else mfma16<NBL, true>(cur, hb, acc2, lane);
        } else if (GEN && q == 2) {      // W'_b: h into a'_b, h'_a into a''
          if constexpr (GEN) {
            mfma16<NBL, true>(cur, h, accb, lane);
            mfma16<NBL, true>(cur, ha, acc2, lane);
          }
        } else {                  // W'': h into a''
          mfma16<NBL, true>(cur, h, acc2, lane);
        }
        if (has_next) {
          if (one_buf) __syncthreads();     // every wave is done with the plane that is about to be overwritten
          f32x4* dst = planes + (one_buf ? 0 : ((gpar + 1) & 1)) * (PLANE / 4);
#pragma unroll
          for (int v = 0; v < PF4; ++v)
            if (PEXACT || tid + NT * v < PLANE / 4) dst[tid + NT * v] = pre[v];
        }
        __syncthreads();
        ++gpar;
      }
      {
        const int ob = o_bh + j * NP + 4 * g;
#pragma unroll
        for (int b = 0; b < NBL; ++b) {
          acc[b] = A.omega * acc[b] + *reinterpret_cast<const f32x4*>(sm + ob + 16 * b);
          acca[b] = A.omega * acca[b] + *reinterpret_cast<const f32x4*>(sm_a + ob + 16 * b);
          if (GEN) accb[b] = A.omega * accb[b] + *reinterpret_cast<const f32x4*>(sm_b + ob + 16 * b);
          if (MIX) accb[b] = A.omega * accb[b];
          acc2[b] = A.omega * acc2[b];
          if (has_dd) acc2[b] += *reinterpret_cast<const f32x4*>(sm_dd + ob + 16 * b);
        }
      }
      f32x4 dv[NBL], sec[NBL];
#pragma unroll
      for (int b = 0; b < NBL; ++b) {
        f32x4 d2;
#pragma unroll
        for (int v = 0; v < 4; ++v) d2[v] = act_d2<ACT>(A.act, acc[b][v]);
        sec[b] = d2 * acca[b] * (DIAG ? acca[b] : accb[b]);
      }
      act16<NBL, ACT>(A.act, acc, acc, dv, n, g);
#pragma unroll
      for (int b = 0; b < NBL; ++b) {
        const f32x4 ta = dv[b] * acca[b];
        const f32x4 t2 = dv[b] * acc2[b] + sec[b];
        f32x4 tb = {0.f, 0.f, 0.f, 0.f};
        if (!DIAG) tb = dv[b] * accb[b];
        if (MODE == 0) {
          ha[b] = ta; h2[b] = t2; h[b] = acc[b];
          if (!DIAG) hb[b] = tb;
        } else if (MODE == 2) {
          ha[b] += ta; h2[b] += t2; h[b] += acc[b];
          if (!DIAG) hb[b] += tb;
        } else {
          if (!(j & 1)) {
            ublka[b] = ha[b]; ha[b] = ta;
            ublk2[b] = h2[b]; h2[b] = t2;
            ublk[b] = h[b]; h[b] = acc[b];
            if (!DIAG) { ublkb[b] = hb[b]; hb[b] = tb; }
          } else {
            ha[b] = 0.5f * (ublka[b] + ta);
            h2[b] = 0.5f * (ublk2[b] + t2);
            h[b] = 0.5f * (ublk[b] + acc[b]);
            if (!DIAG) hb[b] = 0.5f * (ublkb[b] + tb);
          }
        }
      }
    }
    // ---- last layer: u'' = h'' Wl + h'_a Wl'_b + h'_b Wl'_a + h Wl'' + bl'' -----------------------------------------------
    for (int o = 0; o < so; ++o) {
      float p2 = 0.f, px = 0.f;      // px: the cross products (doubled on the diagonal)
#pragma unroll
      for (int b = 0; b < NBL; ++b) {
        const int ow = o_wl + o * NP + 16 * b + 4 * g;
        const f32x4 w = *reinterpret_cast<const f32x4*>(sm + ow);
        const f32x4 wa = *reinterpret_cast<const f32x4*>(sm_a + ow);
        p2 += (h2[b][0] * w[0] + h2[b][1] * w[1]) + (h2[b][2] * w[2] + h2[b][3] * w[3]);
        if (DIAG) px += (ha[b][0] * wa[0] + ha[b][1] * wa[1]) + (ha[b][2] * wa[2] + ha[b][3] * wa[3]);
        else px += (hb[b][0] * wa[0] + hb[b][1] * wa[1]) + (hb[b][2] * wa[2] + hb[b][3] * wa[3]);
        if (GEN) {
          const f32x4 wb = *reinterpret_cast<const f32x4*>(sm_b + ow);
          px += (ha[b][0] * wb[0] + ha[b][1] * wb[1]) + (ha[b][2] * wb[2] + ha[b][3] * wb[3]);
        }
        if (has_dd) {
          const f32x4 wdd = *reinterpret_cast<const f32x4*>(sm_dd + ow);
          p2 += (h[b][0] * wdd[0] + h[b][1] * wdd[1]) + (h[b][2] * wdd[2] + h[b][3] * wdd[3]);
        }
      }
      p2 += DIAG ? 2.0f * px : px;
      if (has_dd && g == 0) p2 += sm_dd[o_bl + o];      // the bias' second tangent once per point (p2 is summed over g)
      p2 += __shfl_xor(p2, 16);
      p2 += __shfl_xor(p2, 32);
      if (valid && g == 0) {
        out[(pt * so + o) * J.row + J.i0] = p2;
        out[(pt * so + o) * J.row + J.i1] = p2;
      }
    }
  }
}

// LDS of a launch: one or two plane buffers and four small-vector images -- k_jac_wt's rule at three streams, so that the shapes
// jac_wt_supported takes are the shapes this kernel takes
static size_t jac_wt2_shmem(const SNetArgs& a, int* one_buf) {
  const int NBL = snet3_nbl(a.n);
  const size_t plane = (size_t)NBL * NBL * 256;
  const size_t rest = ((((size_t)4 * a.nsm) + 3) & ~(size_t)3) + 8;
  *one_buf = (2 * plane + rest) * sizeof(float) > 160u * 1024u ? 1 : 0;
  return ((*one_buf ? 1 : 2) * plane + rest) * sizeof(float);
}

// One pair on T combined nets (`a` as launch_jac_wt takes it; a.B = the longest snapshot's points).  form: WT2_GEN / WT2_DIAG /
// WT2_MIX; wd_a, wd_b, wdd: the tangent slot vectors [T][po] (wd_b: WT2_GEN only; wdd null: no second direction); pl_*: their planes'
// places among the pstride planes of a hidden layer in the image at a.WF (W itself at 0); seed: WT2_MIX's coordinate.  The pair's value
// lands in columns i0 and i1 of out [n][so][row].
void launch_jac_wt2(const SNetArgs& a, long T, int form, const float* wd_a, const float* wd_b, const float* wdd, int pl_a, int pl_b,
                    int pl_dd, int pstride, int seed, int row, int i0, int i1, float* out, hipStream_t st) {
  JacWt2Args J;
  J.s = a; J.pstride = pstride; J.seed = seed; J.row = row; J.i0 = i0; J.i1 = i1; J.out = out;
  J.has_dd = (form != WT2_MIX && wdd) ? 1 : 0;
  J.wd[0] = wd_a; J.wd[1] = form == WT2_GEN ? wd_b : nullptr; J.wd[2] = J.has_dd ? wdd : nullptr;
  int q = 0;
  J.pl[q++] = 0; J.pl[q++] = pl_a;
  if (form == WT2_GEN) J.pl[q++] = pl_b;
  if (J.has_dd) J.pl[q++] = pl_dd;
  J.npl = q;
  for (; q < 4; ++q) J.pl[q] = 0;
  const int NBL = snet3_nbl(a.n);
  const long ngroups = (2 * ((a.B + 31) / 32) + 3) / 4;
  const long cap = NBL <= 4 ? 512 : 256;
  long per = (cap + T - 1) / T;
  if (per > ngroups) per = ngroups;
  dim3 grid((unsigned)(per < 1 ? 1 : per), (unsigned)T), block(256);
  const size_t shm = jac_wt2_shmem(a, &J.one_buf);
#define JL(NBL_, ACT_, MODE_, FORM_)                                                                                                     \
  {                                                                                                                                      \
    if (shm > 48 * 1024)                                                                                                                 \
      (void)hipFuncSetAttribute((const void*)k_jac_wt2<NBL_, ACT_, MODE_, FORM_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm); \
    hipLaunchKernelGGL((k_jac_wt2<NBL_, ACT_, MODE_, FORM_>), grid, block, shm, st, J);                                                  \
  }
#define JF(NBL_, ACT_, MODE_)                                 \
  {                                                           \
    if (form == WT2_GEN) JL(NBL_, ACT_, MODE_, WT2_GEN)       \
    else if (form == WT2_DIAG) JL(NBL_, ACT_, MODE_, WT2_DIAG) \
    else JL(NBL_, ACT_, MODE_, WT2_MIX)                       \
  }
#define JK(NBL_) \
  if (a.nif_skip) JF(NBL_, -1, 2) else if (a.res) JF(NBL_, ACT_SINE, 1) else JF(NBL_, ACT_SINE, 0)
  switch (NBL) {
    case 1: JK(1) break;
    case 2: JK(2) break;
    case 3: JK(3) break;
    case 4: JK(4) break;
    case 6: JK(6) break;
    default: JK(8) break;
  }
#undef JK
#undef JF
#undef JL
}
