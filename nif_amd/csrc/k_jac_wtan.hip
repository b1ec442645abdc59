// k_jac_wtan.hip -- the weight-tangent form of the snapshot tangent kernel (nif_snapshot_param_derivatives*): a sibling of
// k_jac<.., SNAP> (k_jac_dev.h) in a translation unit of its own, so that every k_jac instantiation keeps the code it has.
//
// Over a snapshot t the latent z_t is constant, and so is a direction delta_t,d in latent space (dz/dp_c (p_t), or one the caller
// gives).  The snapshot's net is the dense r = 0 net of the combined slot vector w_t = b + sum_k z_t,k M^(k), and the
// tangent of that net along direction d is carried by ONE more slot vector per direction, wd_t,d = sum_k delta_t,d,k M^(k) (no b):
//
//   first layer   a   = w0 x W1 + b1                a'_d = w0 x W1'_d + b1'_d                      (x fixed)
//   hidden j      a   = w0 h W_j + b_j              a'_d = w0 (h'_d W_j + h W'_d,j) + b'_d,j ;     h'_d = f'(a) a'_d, then the layer's
//                                                   MODE rule as k_jac applies it to any tangent
//   last          u   = h Wl + bl                   u'_d = h'_d Wl + h Wl'_d + bl'_d
//
// Up to NIF_JAC_MAXSEED directions per launch.  The plane image of a snapshot holds, per hidden layer, `pstride` planes
// [W_j | W'_0,j | W'_1,j | W'_2,j]; a launch of ns streams walks the first 1 + ns of each layer through k_jac's double buffer (or its
// one-buffer fallback): on W_j every stream and the primal multiply, on W'_d,j only stream d does -- 1 + 2 ns plane products per
// hidden layer where the point-wise kernel runs (r + 1)(1 + ns).  The small-vector LDS image holds (1 + ns) nsm floats: w_t's
// vectors, then each wd_t,d's.  A stream's arithmetic does not depend on ns nor on its position in the launch.
#include "k_jac_dev.h"

struct JacWtArgs {
  SNetArgs s;                           // as launch_jac_snap: theta + off_bh = the slot vectors w_t [T][po], WF = the plane images, snap_* set
  int ns;                               // direction streams of this launch (<= NIF_JAC_MAXSEED)
  const float* wd[NIF_JAC_MAXSEED];     // stream d's tangent slot vectors [T][po]
  int pstride;                          // planes per hidden layer in the image (>= 1 + ns)
  int nd_total, d0;                     // row stride of dudp (directions of the call) and first column of this launch
  float* dudp;                          // [n][so][nd_total]
  int one_buf;                          // as JacArgs::one_buf
};

template <int NBL, int ACT, int MODE>
__global__ __launch_bounds__(256, (NBL <= 4 ? 2 : 1)) void k_jac_wt(JacWtArgs J) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const SNetArgs& A = J.s;
  constexpr int NT = 256, WAVES = 4, NS = NIF_JAC_MAXSEED;
  constexpr int PLANE = NBL * NBL * 256;
  static_assert(PLANE == plane_elems(PLANES_T16, PLANE_FWD, NBL), "k_pack_dev.h");
  constexpr int PF4 = (PLANE / 4 + NT - 1) / NT;
  constexpr bool PEXACT = (PLANE / 4) % NT == 0;
  constexpr int NP = 16 * NBL;
  // the snapshot of this workgroup, exactly as k_jac<.., SNAP> rebases onto it
  const long ts = blockIdx.y;
  const long p0 = A.snap_off ? A.snap_off[ts] : ts * A.snap_M;
  const long NB = A.snap_off ? A.snap_off[ts + 1] - p0 : A.snap_M;
  if ((long)blockIdx.x >= (2 * ((NB + 31) / 32) + 3) / 4) return;      // no tile group of this snapshot for this slot (whole workgroup)
  const float* xin = A.snap_off ? A.xin + p0 * A.ncol : A.xin;
  const f32x4* WF = A.WF + ts * A.snap_wstride;
  float* u_out = A.u_out ? A.u_out + p0 * A.so : nullptr;
  float* dudp = J.dudp + p0 * A.so * J.nd_total;

  const int tid = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, p = lane & 15, g = lane >> 4;
  const int n = A.n, nh = A.nh, si = A.si, so = A.so, nsm = A.nsm, ns = J.ns, pstride = J.pstride;
  const long nt16 = 2 * ((NB + 31) / 32);
  const long ngroups = (nt16 + WAVES - 1) / WAVES;

  f32x4* planes = reinterpret_cast<f32x4*>(smem);
  const int one_buf = J.one_buf;
  float* sm = smem + (one_buf ? 1 : 2) * PLANE;      // [1 + ns][nsm]: image 0 = w_t, image 1 + d = wd_t,d
  const int o_w1 = 0, o_wl = si * NP, o_b1 = o_wl + so * NP, o_bh = o_b1 + NP, o_bl = o_bh + nh * NP;

  {
    const long s_wl = (long)si * n + (long)nh * n * n;
    const long s_b1 = s_wl + (long)n * so, s_bh = s_b1 + n, s_bl = s_bh + (long)nh * n;
    for (int idx = tid; idx < (1 + ns) * nsm; idx += NT) {
      const int k = idx / nsm, e = idx - k * nsm;
      const float* src = (k == 0 ? A.theta + A.off_bh : (k == 1 ? J.wd[0] : (k == 2 ? J.wd[1] : J.wd[2]))) + ts * A.po;
      float v = 0.f;
      if (e < o_wl) { const int dd = e / NP, f = e - dd * NP; if (f < n) v = src[(long)dd * n + f]; }
      else if (e < o_b1) { const int o = (e - o_wl) / NP, f = (e - o_wl) - o * NP; if (f < n) v = src[s_wl + (long)f * so + o]; }
      else if (e < o_bh) { const int f = e - o_b1; if (f < n) v = src[s_b1 + f]; }
      else if (e < o_bl) { const int j = (e - o_bh) / NP, f = (e - o_bh) - j * NP; if (f < n) v = src[s_bh + (long)j * n + f]; }
      else if (e < o_bl + so) v = src[s_bl + (e - o_bl)];
      sm[idx] = v;
    }
    if (nh > 0) {
#pragma unroll
      for (int q = 0; q < PF4; ++q)
        if (PEXACT || tid + NT * q < PLANE / 4) planes[tid + NT * q] = WF[tid + NT * q];
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

    f32x4 h[NBL], acc[NBL], hd[NS][NBL], accd[NS][NBL];
    // ---- first layer: the layer's expression on w_t, and again on each wd_t,d ----------------------------------
    {
      const float* s0 = sm + 4 * g;
#pragma unroll
      for (int b = 0; b < NBL; ++b) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int dd = 0; dd < si; ++dd) s += xrow[dd] * *reinterpret_cast<const f32x4*>(s0 + o_w1 + dd * NP + 16 * b);
        acc[b] = A.omega * s + *reinterpret_cast<const f32x4*>(s0 + o_b1 + 16 * b);
#pragma unroll
        for (int d = 0; d < NS; ++d) {
          f32x4 sd = {0.f, 0.f, 0.f, 0.f};
          if (d < ns) {
            const float* sdv = s0 + (1 + d) * nsm;
            for (int dd = 0; dd < si; ++dd) sd += xrow[dd] * *reinterpret_cast<const f32x4*>(sdv + o_w1 + dd * NP + 16 * b);
            sd = A.omega * sd + *reinterpret_cast<const f32x4*>(sdv + o_b1 + 16 * b);
          }
          accd[d][b] = sd;
        }
      }
      f32x4 dv[NBL];
      act16<NBL, ACT>(A.act, acc, h, dv, n, g);
#pragma unroll
      for (int d = 0; d < NS; ++d)
#pragma unroll
        for (int b = 0; b < NBL; ++b) hd[d][b] = dv[b] * accd[d][b];
    }
    // ---- hidden layers: planes W_j, W'_0,j .. W'_ns-1,j of the image, in that order -----------------------------
    f32x4 ublk[MODE == 1 ? NBL : 1], ublkd[MODE == 1 ? NS : 1][MODE == 1 ? NBL : 1];
    for (int j = 0; j < nh; ++j) {
#pragma unroll
      for (int b = 0; b < NBL; ++b) {
        acc[b][0] = 0.f; acc[b][1] = 0.f; acc[b][2] = 0.f; acc[b][3] = 0.f;
#pragma unroll
        for (int d = 0; d < NS; ++d) { accd[d][b][0] = 0.f; accd[d][b][1] = 0.f; accd[d][b][2] = 0.f; accd[d][b][3] = 0.f; }
      }
      for (int q = 0; q <= ns; ++q) {
        // the plane after this one: the layer's next, the next layer's first, or (next tile group) the image's first again
        const bool wrap = q == ns && j + 1 == nh;
        const bool has_next = !wrap || !last_group;
        f32x4 pre[PF4];
        if (has_next) {
          const long nxt = wrap ? 0 : (q < ns ? (long)j * pstride + q + 1 : (long)(j + 1) * pstride);
          const f32x4* src = WF + nxt * (PLANE / 4);
#pragma unroll
          for (int v = 0; v < PF4; ++v)
            if (PEXACT || tid + NT * v < PLANE / 4) pre[v] = src[tid + NT * v];
        }
        const f32x4* cur = planes + (one_buf ? 0 : (gpar & 1)) * (PLANE / 4);
        if (q == 0) {
          mfma16<NBL, true>(cur, h, acc, lane);
#pragma unroll
          for (int d = 0; d < NS; ++d)
            if (d < ns) mfma16<NBL, true>(cur, hd[d], accd[d], lane);
        } else {
#pragma unroll
          for (int d = 0; d < NS; ++d)
            if (d == q - 1) mfma16<NBL, true>(cur, h, accd[d], lane);
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
        const float* sb = sm + o_bh + j * NP + 4 * g;
#pragma unroll
        for (int b = 0; b < NBL; ++b) acc[b] = A.omega * acc[b] + *reinterpret_cast<const f32x4*>(sb + 16 * b);
#pragma unroll
        for (int d = 0; d < NS; ++d)
          if (d < ns) {
#pragma unroll
            for (int b = 0; b < NBL; ++b)
              accd[d][b] = A.omega * accd[d][b] + *reinterpret_cast<const f32x4*>(sb + (1 + d) * nsm + 16 * b);
          }
      }
      f32x4 dv[NBL];
      act16<NBL, ACT>(A.act, acc, acc, dv, n, g);
#pragma unroll
      for (int d = 0; d < NS; ++d)
#pragma unroll
        for (int b = 0; b < NBL; ++b) {
          const f32x4 t = dv[b] * accd[d][b];
          if (MODE == 0) hd[d][b] = t;
          else if (MODE == 2) hd[d][b] += t;
          else {
            if (!(j & 1)) { ublkd[d][b] = hd[d][b]; hd[d][b] = t; }
            else hd[d][b] = 0.5f * (ublkd[d][b] + t);
          }
        }
      if (MODE == 0) {
#pragma unroll
        for (int b = 0; b < NBL; ++b) h[b] = acc[b];
      } else if (MODE == 2) {
#pragma unroll
        for (int b = 0; b < NBL; ++b) h[b] += acc[b];
      } else {
        if (!(j & 1)) {
#pragma unroll
          for (int b = 0; b < NBL; ++b) { ublk[b] = h[b]; h[b] = acc[b]; }
        } else {
#pragma unroll
          for (int b = 0; b < NBL; ++b) h[b] = 0.5f * (ublk[b] + acc[b]);
        }
      }
    }
    // ---- last layer: u = h Wl + bl,  u'_d = h'_d Wl + h Wl'_d + bl'_d --------------------------------------------
    for (int o = 0; o < so; ++o) {
      float part = 0.f, pd[NS];
#pragma unroll
      for (int d = 0; d < NS; ++d) pd[d] = 0.f;
#pragma unroll
      for (int b = 0; b < NBL; ++b) {
        const float* wp = sm + o_wl + o * NP + 16 * b + 4 * g;
        const f32x4 w = *reinterpret_cast<const f32x4*>(wp);
        part += (h[b][0] * w[0] + h[b][1] * w[1]) + (h[b][2] * w[2] + h[b][3] * w[3]);
#pragma unroll
        for (int d = 0; d < NS; ++d)
          if (d < ns) {
            const f32x4 wt = *reinterpret_cast<const f32x4*>(wp + (1 + d) * nsm);
            pd[d] += (hd[d][b][0] * w[0] + hd[d][b][1] * w[1]) + (hd[d][b][2] * w[2] + hd[d][b][3] * w[3]);
            pd[d] += (h[b][0] * wt[0] + h[b][1] * wt[1]) + (h[b][2] * wt[2] + h[b][3] * wt[3]);
          }
      }
#pragma unroll
      for (int d = 0; d < NS; ++d)
        if (d < ns && g == 0) pd[d] += sm[(1 + d) * nsm + o_bl + o];      // the bias tangent once per point (pd is summed over g)
      part += __shfl_xor(part, 16);
      part += __shfl_xor(part, 32);
#pragma unroll
      for (int d = 0; d < NS; ++d) { pd[d] += __shfl_xor(pd[d], 16); pd[d] += __shfl_xor(pd[d], 32); }
      if (valid && g == 0) {
        if (u_out) u_out[pt * so + o] = part + sm[o_bl + o];
#pragma unroll
        for (int d = 0; d < NS; ++d)
          if (d < ns) dudp[(pt * so + o) * J.nd_total + J.d0 + d] = pd[d];
      }
    }
  }
}

// LDS of a launch of ns streams: one or two plane buffers and the (1 + ns) small-vector images, under k_jac's rule (jac_shmem)
static size_t jac_wt_shmem(const SNetArgs& a, int ns, int* one_buf) {
  const int NBL = snet3_nbl(a.n);
  const size_t plane = (size_t)NBL * NBL * 256;
  const size_t rest = ((((size_t)(1 + ns) * a.nsm) + 3) & ~(size_t)3) + 8;
  *one_buf = (2 * plane + rest) * sizeof(float) > 160u * 1024u ? 1 : 0;
  return ((*one_buf ? 1 : 2) * plane + rest) * sizeof(float);
}
// shapes the weight-tangent form takes: one plane and four small-vector images must fit the LDS (every shape jac_supported takes
// with r >= 3 does; a smaller latent with very many small vectors may not)
bool jac_wt_supported(const SNetArgs& a) {
  if (a.n > 128) return false;
  int one_buf;
  return jac_wt_shmem(a, NIF_JAC_MAXSEED, &one_buf) <= 160u * 1024u;
}

// ns direction streams on T combined nets (`a` as launch_jac_snap takes it; a.B = the longest snapshot's points): columns
// d0 .. d0 + ns of dudp [n][so][nd_total]; wd[d] = the tangent slot vectors [T][po] of stream d; pstride = planes per hidden layer
// in the image at a.WF
void launch_jac_wt(const SNetArgs& a, long T, int ns, const float* const* wd, int pstride, int nd_total, int d0, float* dudp,
                   hipStream_t st) {
  JacWtArgs J;
  J.s = a; J.ns = ns; J.pstride = pstride; J.nd_total = nd_total; J.d0 = d0; J.dudp = dudp;
  for (int d = 0; d < NIF_JAC_MAXSEED; ++d) J.wd[d] = d < ns ? wd[d] : nullptr;
  const int NBL = snet3_nbl(a.n);
  const long ngroups = (2 * ((a.B + 31) / 32) + 3) / 4;
  const long cap = NBL <= 4 ? 512 : 256;
  long per = (cap + T - 1) / T;
  if (per > ngroups) per = ngroups;
  dim3 grid((unsigned)(per < 1 ? 1 : per), (unsigned)T), block(256);
  const size_t shm = jac_wt_shmem(a, ns, &J.one_buf);
#define JL(NBL_, ACT_, MODE_)                                                                                                    \
  {                                                                                                                              \
    if (shm > 48 * 1024)                                                                                                         \
      (void)hipFuncSetAttribute((const void*)k_jac_wt<NBL_, ACT_, MODE_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm); \
    hipLaunchKernelGGL((k_jac_wt<NBL_, ACT_, MODE_>), grid, block, shm, st, J);                                                  \
  }
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
}
