// nif_api.hip -- C-ABI of libnif_hip.so (include/nif_hip.h): context, parameter layout, kernel
// orchestration.  gfx950 only; there is no CPU fallback.
#include "../../include/nif_hip.h"
#include "nif_internal.h"
#include "k_pack_dev.h"
#include <cstdlib>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "nif_ctx.h"
#include "../../include/nif_hip_snapshots.h"
#include "../../include/nif_hip_snapderiv.h"
#include "../../include/nif_hip_snapparam.h"
#include "../../include/nif_hip_snapparam2.h"
#include "../../include/nif_hip_encode.h"
#include "../../include/nif_hip_snapfit.h"
#include "../../include/nif_hip_sensors.h"

#define NIF_ACT_SLABS 32   // point slabs of the activity regulariser's plane pass
static inline bool act_on(const nif_ctx* c) { return c->act_l1 != 0.f || c->act_l2 != 0.f; }
// Scope of the passes of a multi-pass step that run without jac_reg and the activity regulariser (their losses belong to the first
// pass): the coefficients are zero inside and back on every way out
struct RegsOff {
  nif_ctx* c; float jac_l1, act_l1, act_l2;
  RegsOff(nif_ctx* c_, bool on) : c(on ? c_ : nullptr) {
    if (!c) return;
    jac_l1 = c->jac_l1; act_l1 = c->act_l1; act_l2 = c->act_l2;
    c->jac_l1 = 0.f; c->act_l1 = 0.f; c->act_l2 = 0.f;
  }
  ~RegsOff() { if (c) { c->jac_l1 = jac_l1; c->act_l1 = act_l1; c->act_l2 = act_l2; } }
  RegsOff(const RegsOff&) = delete;
  RegsOff& operator=(const RegsOff&) = delete;
};
static int jac_reg_pass(nif_ctx* c, const float* xin, long B, long Bg, const int* mu_blk = nullptr);
// Sobolev streams of one x_index: coordinate seeds first, then the parameter seeds (their pseudo-tiles trail the stashes, so
// that the first-layer reduction simply stops in front of them); gcol = the x_index position (column of dydx) of each stream
struct SobPlan { int ns, nsc; int seeds[3]; int par[3]; int gcol[3]; bool any_par;
                 int gstride, nx_all, ny, no_primal; unsigned ymask;
                 int hess; };      // 1: a second-order pair pass (nif_sobolev2_loss_grad_dev, SobPar::hess)      // r4: one group of the x_index columns / a y_index subset (SobPar)
static int sob_par_pass(nif_ctx* c, const float* xin, long B, long Bg, const SobPlan& sp, const SNetArgs& sa);
static int fill_snet_ll_sob(nif_ctx* c, SNetArgs& sa, const float* xin, long B, bool f32_planes = false);

#ifndef NIF_PIPE_CHUNK_DEFAULT
#define NIF_PIPE_CHUNK_DEFAULT 131072L
#endif

static thread_local std::string g_err;
int nif_fail(int code, const std::string& msg) { g_err = msg; return code; }

extern "C" const char* nif_last_error(void) { return g_err.c_str(); }
extern "C" int nif_abi_version(void) { return NIF_ABI_VERSION; }
extern "C" int nif_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static void add_desc(nif_ctx* c, const char* name, long& off, int rows, int cols) {
  nif_tensor_desc d;
  memset(&d, 0, sizeof(d));
  snprintf(d.name, sizeof(d.name), "%s", name);
  d.offset = off; d.rows = rows; d.cols = cols;
  c->layout.push_back(d);
  off += (long)rows * (cols ? cols : 1);
}

// Keras variable order (nif/model.py:178-231, :591-734, :1162-1215)
static int build_layout(nif_ctx* c) {
  long off = 0;
  char nm[48];
  c->first_w = off; add_desc(c, "pnet_first_w", off, c->pi, c->nst);
  c->first_b = off; add_desc(c, "pnet_first_b", off, c->nst, 0);
  for (int i = 0; i < c->lst; ++i) {
    snprintf(nm, sizeof(nm), "pnet_h%d_w", i); c->hid_w[i] = off; add_desc(c, nm, off, c->nst, c->nst);
    snprintf(nm, sizeof(nm), "pnet_h%d_b", i); c->hid_b[i] = off; add_desc(c, nm, off, c->nst, 0);
    if (c->cfg.p_resblock) {
      snprintf(nm, sizeof(nm), "pnet_h%d_w2", i); c->hid_w2[i] = off; add_desc(c, nm, off, c->nst, c->nst);
      snprintf(nm, sizeof(nm), "pnet_h%d_b2", i); c->hid_b2[i] = off; add_desc(c, nm, off, c->nst, 0);
    }
  }
  c->bott_w = off; add_desc(c, "pnet_bottleneck_w", off, c->nst, c->r);
  c->bott_b = off; add_desc(c, "pnet_bottleneck_b", off, c->r, 0);
  c->last_w = off; add_desc(c, "pnet_last_w", off, c->r, (int)c->po);
  c->last_b = off; add_desc(c, "pnet_last_b", off, (int)c->po, 0);
  if (c->kind == NIF_KIND_LASTLAYER) {
    const int nout = (int)c->po * c->so;
    c->s_first_w = off; add_desc(c, "snet_first_w", off, c->si, c->n);
    c->s_first_b = off; add_desc(c, "snet_first_b", off, c->n, 0);
    for (int i = 0; i < c->L; ++i) {
      snprintf(nm, sizeof(nm), "snet_h%d_w", i); c->s_hid_w[i] = off; add_desc(c, nm, off, c->n, c->n);
      snprintf(nm, sizeof(nm), "snet_h%d_b", i); c->s_hid_b[i] = off; add_desc(c, nm, off, c->n, 0);
      if (c->cfg.s_resblock) {
        snprintf(nm, sizeof(nm), "snet_h%d_w2", i); c->s_hid_w2[i] = off; add_desc(c, nm, off, c->n, c->n);
        snprintf(nm, sizeof(nm), "snet_h%d_b2", i); c->s_hid_b2[i] = off; add_desc(c, nm, off, c->n, 0);
      }
    }
    c->s_bott_w = off; add_desc(c, "snet_bottleneck_w", off, c->n, nout);
    c->s_bott_b = off; add_desc(c, "snet_bottleneck_b", off, nout, 0);
    c->ll_bias = off; add_desc(c, "last_layer_bias", off, c->so, 0);
  }
  c->P = off;
  return 0;
}

// f32x4 of one fp32 plane of `nblk` blocks per side
static long plane_f32x4(PlaneSet s, int nblk) { return plane_elems(s, PLANE_FWD, nblk) / 4; }
// the stream and every buffer whose size the configuration fixes
static int create_buffers(nif_ctx* c) {
  const int nh = c->nh, nm = c->nm;
  HIPCHK(hipSetDevice(c->dev));
  HIPCHK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
  const long pn = c->P + 2;   // [grad | loss | one scratch word of the two-level row reduction]
  for (DevBuf<float>* b : {&c->theta, &c->grad, &c->m, &c->v}) { const int rc = b->alloc(pn); if (rc) return rc; }
  for (float* b : {c->m.p, c->v.p, c->grad.p}) HIPCHK(hipMemset(b, 0, sizeof(float) * (size_t)pn));
  int rc = NIF_OK;
  const long pk_p = (long)(nm > 0 ? nm : 1) * plane_f32x4(PLANES_T32, c->NSTB);
  const long p32 = plane_f32x4(PLANES_T32, c->NB), p16 = plane_f32x4(PLANES_T16, snet3_nbl(c->n));     // one buffer serves either tile size
  // (a wide last-layer net reads its matrices row-major from theta: no plane image of any kind, one element keeps the buffers non-null)
  const long pk_s = c->use_wide ? 1 : (long)(nh > 0 ? nh : 1) * (c->r + 1) * (p16 > p32 ? p16 : p32);
  if (!rc) rc = c->pWF.alloc(pk_p);
  if (!rc) rc = c->pWB.alloc(pk_p);
  if (!rc) rc = c->sWF.alloc(pk_s);
  if (!rc) rc = c->sWB.alloc(pk_s);
  if (nh > 0 && !(snet3_nbl(c->n) & 1) && c->n <= 128) {
    const int rr = c->kind == NIF_KIND_LASTLAYER ? 0 : c->r;   // last-layer class: shared dense weights, one plane
    auto set = [&](DevBuf<char>& f, DevBuf<char>& b, PlaneSet s, int nmat) {       // both images of `nmat` matrices in set s
      if (!rc) rc = f.alloc(nmat * plane_mat_bytes(s, PLANE_FWD, c->n, rr));
      if (!rc) rc = b.alloc(nmat * plane_mat_bytes(s, PLANE_BWD, c->n, rr));
    };
    set(c->sWF4, c->sWB4, PLANES_SPLIT, nh);
    if (c->kind != NIF_KIND_NIF) {   // SIREN nets (r5): the exact-product half planes of k_snet4<.., PR = 3> / k_snet6 (class NIF keeps the bf16 splits)
      set(c->sWF4x, c->sWB4x, PLANES_HALF, nh);
      if (!rc) rc = c->sWscale.alloc((long)nh * (rr + 1) * 2);
    }
    // the policy's compact plane set (k_snet4 / k_snet6<.., PR>), next to the exact splits
    if (c->cfg.mixed_policy != NIF_POLICY_FLOAT32) set(c->sWF4h, c->sWB4h, PLANES_COMPACT, nh);
    if (c->kind == NIF_KIND_LASTLAYER) set(c->ll_wpf, c->ll_wpb, PLANES_PHI, 1);
  }
  // slot-ordered copy of the dense ShapeNet parameters of the last-layer class (k_snet4<LL>, k_sob<LL>, k_jac on the r = 0 arguments)
  if (c->kind == NIF_KIND_LASTLAYER && nh > 0 && c->n <= 128 && !rc)
    rc = c->ll_slots.alloc((long)c->si * c->n + (long)nh * c->n * c->n + (long)c->n * c->so * c->r +
                           c->n + (long)nh * c->n + c->so * c->r + c->so + c->r * c->r + 64);
  const long pk_l = c->use_wide ? 1 : (long)(nh > 0 ? nh : 1) * plane_f32x4(PLANES_T32, c->NB);
  if (!rc && c->kind == NIF_KIND_LASTLAYER) rc = c->lWF.alloc(pk_l);
  if (!rc && c->kind == NIF_KIND_LASTLAYER) rc = c->lWB.alloc(pk_l);
  return rc;
}

extern "C" int nif_create(const nif_cfg* cfg, int device_id, nif_ctx** out) {
  if (!cfg || !out) return fail(NIF_ERR_INVALID, "null argument");
  if (cfg->abi_version != NIF_ABI_VERSION) return fail(NIF_ERR_INVALID, "abi_version mismatch");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(NIF_ERR_NODEVICE, "no HIP device visible: libnif_hip has no CPU fallback");
  if (device_id < 0 || device_id >= ndev) return fail(NIF_ERR_INVALID, "device_id out of range");
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(NIF_ERR_NODEVICE, std::string("device is ") + prop.gcnArchName + ", libnif_hip is built for gfx950 only");
  if (cfg->kind != NIF_KIND_NIF && cfg->kind != NIF_KIND_MULTISCALE && cfg->kind != NIF_KIND_LASTLAYER)
    return fail(NIF_ERR_INVALID, "unknown model kind");
  if (cfg->mixed_policy != NIF_POLICY_FLOAT32 && cfg->mixed_policy != NIF_POLICY_MIXED_BF16 && cfg->mixed_policy != NIF_POLICY_MIXED_F16)
    return fail(NIF_ERR_INVALID, "unknown mixed_policy");
  for (int i = 0; i < 7; ++i) if (cfg->reserved[i] != 0) return fail(NIF_ERR_INVALID, "reserved fields must be zero");
  if (cfg->p_act < 0 || cfg->p_act > NIF_ACT_HARD_SIGMOID || cfg->s_act < 0 || cfg->s_act > NIF_ACT_HARD_SIGMOID)
    return fail(NIF_ERR_INVALID, "unknown activation id (nif_act)");
  if (cfg->kind == NIF_KIND_LASTLAYER && cfg->latent_dim * cfg->so_dim > 64)
    return fail(NIF_ERR_INVALID, "last-layer class: latent_dim * output_dim must be <= 64");
  if (cfg->pi_dim < 1 || cfg->si_dim < 1 || cfg->so_dim < 1 || cfg->latent_dim < 1)
    return fail(NIF_ERR_INVALID, "dims must be >= 1");
  if (cfg->n_sx < 1 || cfg->n_st < 1) return fail(NIF_ERR_INVALID, "units must be >= 1");
  if (cfg->n_st > 128) return fail(NIF_ERR_INVALID, "ParameterNet units must be in [1,128]");
  // ShapeNets wider than 128 units: the last-layer class alone, on the workgroup-tiled layer kernels (k_wide.hip)
  const bool wide = cfg->n_sx > 128;
  if (wide && cfg->kind != NIF_KIND_LASTLAYER)
    return fail(NIF_ERR_INVALID, "ShapeNet units must be in [1,128] for NIF / NIFMultiScale: only the last-layer class goes wider (up to 512)");
  if (cfg->n_sx > 512) return fail(NIF_ERR_INVALID, "ShapeNet units must be in [1,512] for the last-layer class");
  if (wide && cfg->s_resblock)
    return fail(NIF_ERR_INVALID, "ShapeNet wider than 128 units: plain SIREN only, use_resblock stops at 128 units");
  if (wide && cfg->mixed_policy != NIF_POLICY_FLOAT32)
    return fail(NIF_ERR_INVALID, "ShapeNet wider than 128 units: mixed_policy float32 only, the mixed policies stop at 128 units");
  if (cfg->latent_dim > 64) return fail(NIF_ERR_INVALID, "latent_dim must be <= 64");
  if (cfg->pi_dim > 16 || cfg->si_dim > 16 || cfg->so_dim > 16)
    return fail(NIF_ERR_INVALID, "input/output dims must be <= 16");
  const int nh = cfg->l_sx * (cfg->s_resblock ? 2 : 1);
  const int nm = cfg->l_st * (cfg->p_resblock ? 2 : 1);
  if (cfg->l_sx < 0 || nh > NIF_MAX_HID || cfg->l_st < 0 || cfg->l_st > NIF_MAX_HID)
    return fail(NIF_ERR_INVALID, "too many layers");
  if (cfg->kind == NIF_KIND_NIF && (cfg->s_resblock || cfg->p_resblock || cfg->p_act == NIF_ACT_SINE))
    return fail(NIF_ERR_INVALID, "class NIF has no resblock / sine ParameterNet");
  if (cfg->p_resblock && cfg->kind == NIF_KIND_NIF) return fail(NIF_ERR_INVALID, "bad cfg");

  std::unique_ptr<nif_ctx> own(new nif_ctx());      // (a failure below frees the stream and every buffer made so far: ~nif_ctx)
  nif_ctx* c = own.get();
  c->cfg = *cfg;
  { const char* e = getenv("NIF_FP32_MFMA"); c->opt_fp32_mfma = e && e[0] == '1'; }
  { const char* e = getenv("NIF_FUSE_GW"); c->opt_fuse_gw = !(e && e[0] == '0'); }
  { const char* e = getenv("NIF_SMALL_STEP"); c->opt_small_step = !(e && e[0] == '0'); }
  { const char* e = getenv("NIF_FUSE_TAIL"); c->opt_fuse_tail = !(e && e[0] == '0'); }
  { const char* e = getenv("NIF_PIPE_CHUNK"); if (e && e[0]) c->opt_pipe_chunk = atol(e); }
  { const char* e = getenv("NIF_SIDE_PNET"); if (e && e[0]) c->opt_side_pnet = e[0] != '0'; }
  { const char* e = getenv("NIF_PIPE_WGS"); if (e && e[0]) c->opt_pipe_wgs = atoi(e); }
  c->dev = device_id;
  c->kind = cfg->kind; c->pi = cfg->pi_dim; c->si = cfg->si_dim; c->so = cfg->so_dim;
  c->n = cfg->n_sx; c->L = cfg->l_sx; c->nst = cfg->n_st; c->lst = cfg->l_st; c->r = cfg->latent_dim;
  c->nh = nh; c->nm = nm;
  c->use_wide = wide;
  c->NB = c->n <= 32 ? 1 : (c->n <= 64 ? 2 : 4);
  c->NSTB = c->nst <= 32 ? 1 : (c->nst <= 64 ? 2 : 4);
  c->po = (long)nh * c->n * c->n + (long)(c->si + c->so + 1 + nh) * c->n + c->so;
  if (c->kind == NIF_KIND_LASTLAYER) c->po = c->r;   // model.py:583-585
  c->RB = (c->r + 31) / 32;
  build_layout(c);
  c->pstride = (c->P + 1 + 63) / 64 * 64;
  if (create_buffers(c) != NIF_OK) return fail(NIF_ERR_HIP, "nif_create: " + g_err);
  *out = own.release();
  return NIF_OK;
}

nif_ctx::~nif_ctx() {
  (void)hipSetDevice(dev);
  nif_f64_release(this);
  if (comm) (void)nif_comm_destroy(this);
  for (hipStream_t s : {st2, st_copy, st}) if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
  for (hipEvent_t e : {ev_copied[0], ev_copied[1], ev_consumed[0], ev_consumed[1], ev_start, ev_done, t0, t1}) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev_chunk) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
  for (const Rec& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (const CapGraph& g : graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
}
extern "C" int nif_destroy(nif_ctx* c) {
  if (!c) return NIF_OK;
  (void)nif_enter(c, NIF_FLUSH_NONE);      // (a deferred piece goes with the context; a failing device must not keep the memory alive)
  if (c->st) hipStreamSynchronize(c->st);
  delete c;
  return NIF_OK;
}

extern "C" int nif_param_count(nif_ctx* c, int64_t* n) { if (!c || !n) return fail(NIF_ERR_INVALID, "null"); *n = c->P; return NIF_OK; }
extern "C" int nif_po_dim(nif_ctx* c, int64_t* po) { if (!c || !po) return fail(NIF_ERR_INVALID, "null"); *po = c->po; return NIF_OK; }
extern "C" int nif_param_layout(nif_ctx* c, nif_tensor_desc* descs, int32_t* n_inout) {
  if (!c || !n_inout) return fail(NIF_ERR_INVALID, "null");
  const int need = (int)c->layout.size();
  if (!descs || *n_inout < need) { *n_inout = need; return descs ? fail(NIF_ERR_INVALID, "descs too small") : NIF_OK; }
  memcpy(descs, c->layout.data(), sizeof(nif_tensor_desc) * need);
  *n_inout = need;
  return NIF_OK;
}

extern "C" int nif_set_params(nif_ctx* c, const float* host, int64_t n) {
  if (!c || !host) return fail(NIF_ERR_INVALID, "null");
  if (n != c->P) return fail(NIF_ERR_INVALID, "parameter count mismatch");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipMemcpyAsync(c->theta, host, sizeof(float) * n, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  c->have_params = true; c->planes_stale();
  return NIF_OK;
}
extern "C" int nif_get_params(nif_ctx* c, float* host, int64_t n) {
  if (!c || !host) return fail(NIF_ERR_INVALID, "null");
  if (n != c->P) return fail(NIF_ERR_INVALID, "parameter count mismatch");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipMemcpyAsync(host, c->theta, sizeof(float) * n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}
extern "C" int nif_get_opt_state(nif_ctx* c, float* mh, float* vh, int64_t n, int64_t* step) {
  if (!c || !mh || !vh || !step) return fail(NIF_ERR_INVALID, "null");
  if (n != c->P) return fail(NIF_ERR_INVALID, "parameter count mismatch");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipMemcpyAsync(mh, c->m, sizeof(float) * n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(vh, c->v, sizeof(float) * n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  *step = c->step;
  return NIF_OK;
}
extern "C" int nif_set_opt_state(nif_ctx* c, const float* mh, const float* vh, int64_t n, int64_t step) {
  if (!c || !mh || !vh) return fail(NIF_ERR_INVALID, "null");
  if (n != c->P) return fail(NIF_ERR_INVALID, "parameter count mismatch");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipMemcpyAsync(c->m, mh, sizeof(float) * n, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(c->v, vh, sizeof(float) * n, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  c->step = step;
  // fresh slots (Adagrad's accumulator is still to be initialised): iteration 0 and nothing but zeros, what compile() of a new optimizer writes
  c->slots_fresh = step == 0;
  for (int64_t i = 0; i < n && c->slots_fresh; ++i) c->slots_fresh = mh[i] == 0.f && vh[i] == 0.f;
  c->ema_valid = false;      // (what fit() calls for a freshly compiled optimizer: the next EMA step seeds the average again)
  return NIF_OK;
}

extern "C" int nif_dev_alloc(nif_ctx* c, int64_t bytes, void** dptr) {
  if (!c || !dptr || bytes < 0) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipMalloc(dptr, bytes > 0 ? (size_t)bytes : 4));
  return NIF_OK;
}
extern "C" int nif_dev_free(nif_ctx* c, void* dptr) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  if (dptr) HIPCHK(hipFree(dptr));
  return NIF_OK;
}
extern "C" int nif_h2d(nif_ctx* c, void* dst, const void* src, int64_t bytes) {
  if (!c || !dst || !src) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}
extern "C" int nif_d2h(nif_ctx* c, void* dst, const void* src, int64_t bytes) {
  if (!c || !dst || !src) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}
extern "C" int nif_sync(nif_ctx* c) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}
// ---- shard streaming: pinned host staging + asynchronous H2D on a copy stream, double buffered -----------------------
extern "C" int nif_host_alloc(nif_ctx* c, int64_t bytes, void** hptr) {
  if (!c || !hptr || bytes < 0) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipHostMalloc(hptr, bytes > 0 ? (size_t)bytes : 4, hipHostMallocDefault));
  return NIF_OK;
}
extern "C" int nif_host_free(nif_ctx* c, void* hptr) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  if (c->st_copy) HIPCHK(hipStreamSynchronize(c->st_copy));
  if (hptr) HIPCHK(hipHostFree(hptr));
  return NIF_OK;
}
static int ensure_copy_stream(nif_ctx* c) {
  if (c->st_copy) return NIF_OK;
  HIPCHK(hipStreamCreateWithFlags(&c->st_copy, hipStreamNonBlocking));
  for (int s = 0; s < 2; ++s) {
    HIPCHK(hipEventCreateWithFlags(&c->ev_copied[s], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_consumed[s], hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_copied[s], c->st_copy));       // both start out signalled
    HIPCHK(hipEventRecord(c->ev_consumed[s], c->st));
  }
  return NIF_OK;
}
extern "C" int nif_h2d_async(nif_ctx* c, void* dst_dev, const void* src_pinned, int64_t bytes, int32_t slot) {
  if (!c || !dst_dev || !src_pinned || bytes < 0 || slot < 0 || slot > 1) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  int rc = ensure_copy_stream(c); if (rc) return rc;
  HIPCHK(hipStreamWaitEvent(c->st_copy, c->ev_consumed[slot], 0));   // the steps that read this slot's device buffer are done
  HIPCHK(hipMemcpyAsync(dst_dev, src_pinned, (size_t)bytes, hipMemcpyHostToDevice, c->st_copy));
  HIPCHK(hipEventRecord(c->ev_copied[slot], c->st_copy));
  return NIF_OK;
}
extern "C" int nif_copy_acquire(nif_ctx* c, int32_t slot) {       // compute stream: wait until the slot's copies have landed
  if (!c || slot < 0 || slot > 1) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  int rc = ensure_copy_stream(c); if (rc) return rc;
  HIPCHK(hipStreamWaitEvent(c->st, c->ev_copied[slot], 0));
  return NIF_OK;
}
extern "C" int nif_copy_release(nif_ctx* c, int32_t slot) {       // compute stream: everything enqueued so far has consumed the slot
  if (!c || slot < 0 || slot > 1) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  int rc = ensure_copy_stream(c); if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev_consumed[slot], c->st));
  return NIF_OK;
}
extern "C" int nif_copy_wait_host(nif_ctx* c, int32_t slot) {     // host: the slot's pinned staging buffer may be overwritten
  if (!c || slot < 0 || slot > 1) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  int rc = ensure_copy_stream(c); if (rc) return rc;
  HIPCHK(hipEventSynchronize(c->ev_copied[slot]));
  return NIF_OK;
}
extern "C" int nif_gather_rows_dev(nif_ctx* c, const float* src_dev, const int32_t* perm_dev, int64_t n, int32_t ncol, float* dst_dev) {
  if (!c || !src_dev || !perm_dev || !dst_dev || n < 0 || ncol < 1) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  if (n > 0) launch_gather_rows(src_dev, perm_dev, n, ncol, dst_dev, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}

extern "C" void* nif_stream(nif_ctx* c) { return c ? (void*)c->st : nullptr; }
// (no error code to return and no device work without a pending reduction: the guard only then)
extern "C" void* nif_grad_dev(nif_ctx* c) { if (c && c->tail_pending) (void)nif_enter(c, NIF_FLUSH_TAIL); return c ? (void*)c->grad : nullptr; }
extern "C" void* nif_params_dev(nif_ctx* c) { return c ? (void*)c->theta : nullptr; }

// ------------------------------------------------------------------------------------------
// internal orchestration
// ------------------------------------------------------------------------------------------
// Partial gradient rows and loss partials of a training step over B points: all a k_small step needs of ensure_capacity.
// One loss partial per workgroup of the fused kernel: the 16-point-tile kernels launch up to ceil(2*ntiles/4) workgroups (k_snet3/4,
// k_sob), k_ll_out ntiles/8, k_snet ntiles/4 (r6: k_small one per 16 points = 2 ntiles)
static int ensure_rows(nif_ctx* c, long B) {
  const long ntiles = (B + 31) / 32;
  const int rc = c->loss_partial.reserve(c, 2 * ntiles + 1); if (rc) return rc;
  return c->partial.reserve(c, 256 * c->pstride);
}
// Point workspaces for B points and, for a training step, the stashes and ensure_rows.  c->cap describes all of them: a failure on the
// way leaves none and cap = 0, so the next call builds them again.
static int ensure_capacity(nif_ctx* c, long B, bool train) {
  const long pts = (B + 31) / 32 * 32;
  if (pts > c->cap || (train && !(c->use_wide ? c->wide_stash : c->stash_s))) {
    const long newcap = pts > c->cap ? pts : c->cap;
    const bool ll = c->kind == NIF_KIND_LASTLAYER;
    if (c->use_wide && c->capturing)
      return fail(NIF_ERR_STATE, "a workspace of the wide ShapeNet would have to grow inside a graph capture: call nif_reserve for the largest batch first");
    DevBuf<float>* ws[] = {&c->Z, &c->DZ, &c->DU, &c->ZL, &c->PHI, &c->DPHI, &c->DA, &c->DZL};
    const long wsz[] = {(long)c->r * newcap, (long)c->r * newcap, (long)c->so * newcap, (long)32 * c->RB * newcap,
                        (long)c->r * c->so * newcap, (long)c->r * c->so * newcap, (long)c->r * newcap, (long)c->r * newcap};
    int rc = NIF_OK;
    for (int i = 0; i < (ll ? 8 : 4) && !rc; ++i) rc = ws[i]->reserve(c, wsz[i]);
    if (!rc && c->use_wide) rc = c->wide_act.reserve(c, 2L * c->n * newcap);
    if (!rc && newcap > c->cap) { rc = c->stash_s.release(c); if (!rc) rc = c->stash_p.release(c); if (!rc) rc = c->wide_stash.release(c); }      // (their slot strides follow cap)
    if (!rc && train && c->use_wide) {      // sin and cos of every layer's phase; the ShapeNet's 32-point stash does not exist
      c->slot_p = (long)c->NSTB * 32 * newcap;
      rc = c->wide_stash.reserve(c, 2L * (c->nh + 1) * c->n * newcap);
      if (!rc) rc = c->stash_p.reserve(c, c->slot_p * (2 * c->nm + 2));
    } else if (!rc && train) {
      c->slot_s = (long)c->NB * 32 * newcap;
      c->slot_p = (long)c->NSTB * 32 * newcap;
      // r6 (fuzz case 606/16): k_snet6 keeps its private h ring in this buffer -- [workgroups][8 waves][nh][64 features][16 points],
      // EVERY wave of a workgroup writes its slice, active or not -- and for batches of <= 32 points of a net with nh >= 2 that is more
      // than the 2 (nh + 1) stash slots of one 32-point tile: the ring ran 32 KB past the allocation into the ParameterNet's stash
      // (wrong ParameterNet gradients on the stash path: ParameterNets with > 2 hidden matrices or > 32 units)
      long s_floats = c->slot_s * 2 * (c->nh + 1);
      const long ring6 = snet6_ring_floats(newcap, c->nh);
      if (ring6 > s_floats) s_floats = ring6;
      rc = c->stash_s.reserve(c, s_floats);
      if (!rc) rc = c->stash_p.reserve(c, c->slot_p * (2 * c->nm + 2));
      if (!rc && c->NB * 32 > ((c->n + 15) / 16) * 16)    // 65..96 (and 33..48) units: the rows the fused kernels never write must read as zero
        rc = hipMemsetAsync(c->stash_s, 0, sizeof(float) * (size_t)s_floats, c->st) == hipSuccess ? NIF_OK : fail(NIF_ERR_HIP, "hipMemsetAsync(stash_s)");
    }
    if (rc) {
      for (DevBuf<float>* b : ws) b->drop();
      c->stash_s.drop(); c->stash_p.drop(); c->wide_act.drop(); c->wide_stash.drop();
      c->cap = 0;
      return rc;
    }
    c->cap = newcap;
  }
  return train ? ensure_rows(c, B) : NIF_OK;
}

static MatRef dense_ref(long w_off, int nin, int nout) { MatRef m; m.r = 0; m.base_k = 0; m.kstride = 0; m.base_last = w_off; m.ld = nout; m.nin = nin; m.nout = nout; return m; }
static MatRef vec_ref(long b_off, int nout) { MatRef m; m.r = 0; m.base_k = 0; m.kstride = 0; m.base_last = b_off; m.ld = 0; m.nin = 1; m.nout = nout; return m; }
static MatRef hyper_ref(const nif_ctx* c, long slot, int ld, int nin, int nout) {
  MatRef m; m.r = c->r; m.base_k = c->last_w + slot; m.kstride = c->po; m.base_last = c->last_b + slot; m.ld = ld; m.nin = nin; m.nout = nout; return m;
}
// Hyper-slot layout of one row of the [r][po] hyper kernel (and of the hyper bias): the ShapeNet's kernels first (si x n), hidden j
// (n x n each), last (n x so), then its biases in the same order.  Layer l: 0 = first, 1 + j = hidden matrix j, nh + 1 = last.  The
// host side's one statement of it (the kernels' prologues derive the same offsets from SNetArgs)
static long hyper_wslot(const nif_ctx* c, int l) { return l == 0 ? 0 : (long)c->si * c->n + (long)(l - 1) * c->n * c->n; }
static long hyper_bslot(const nif_ctx* c, int l) { return hyper_wslot(c, c->nh + 1) + (long)c->n * c->so + (long)l * c->n; }
// ... and the layers as operands of the weight-gradient reductions
static MatRef hyper_w(const nif_ctx* c, int l) {
  const int nin = l == 0 ? c->si : c->n, nout = l == c->nh + 1 ? c->so : c->n;
  return hyper_ref(c, hyper_wslot(c, l), nout, nin, nout);
}
static MatRef hyper_b(const nif_ctx* c, int l) { return hyper_ref(c, hyper_bslot(c, l), 0, 1, l == c->nh + 1 ? c->so : c->n); }

// matrix j of an MLP's hidden stack (pairs (w, w2) per layer with resblocks) -> offsets of its kernel and bias in theta
static void mlp_mat(bool res, const long* w, const long* b, const long* w2, const long* b2, int j, long* w_off, long* b_off) {
  const int i = res ? j / 2 : j;
  const bool second = res && (j & 1);
  *w_off = second ? w2[i] : w[i]; *b_off = second ? b2[i] : b[i];
}
static void pnet_mat(const nif_ctx* c, int j, long* w_off, long* b_off) { mlp_mat(c->cfg.p_resblock, c->hid_w, c->hid_b, c->hid_w2, c->hid_b2, j, w_off, b_off); }
static void snet_mat(const nif_ctx* c, int j, long* w_off, long* b_off) { mlp_mat(c->cfg.s_resblock, c->s_hid_w, c->s_hid_b, c->s_hid_w2, c->s_hid_b2, j, w_off, b_off); }
// the mixed policy's MFMA operand form: 0 exact bf16 splits (float32), 1 bf16 planes, 2 f16 planes
static int policy_prec(const nif_ctx* c) { return c->cfg.mixed_policy == NIF_POLICY_MIXED_BF16 ? 1 : (c->cfg.mixed_policy == NIF_POLICY_MIXED_F16 ? 2 : 0); }

static void fill_pnet(const nif_ctx* c, PNetArgs& a, const float* xin, long B) {
  memset(&a, 0, sizeof(a));
  a.theta = c->theta; a.xin = xin; a.ncol = c->pi + c->si; a.col0 = 0; a.B = B;
  a.pi = c->pi; a.nst = c->nst; a.lst = c->lst; a.r = c->r;
  a.act = c->cfg.p_act; a.res = c->cfg.p_resblock; a.siren = (c->cfg.p_act == NIF_ACT_SINE);
  a.omega = a.siren ? c->cfg.p_omega0 : 1.0f;
  a.first_w = c->first_w; a.first_b = c->first_b;
  for (int i = 0; i < c->lst; ++i) { a.hid_w[i] = c->hid_w[i]; a.hid_b[i] = c->hid_b[i]; a.hid_w2[i] = c->hid_w2[i]; a.hid_b2[i] = c->hid_b2[i]; }
  a.bott_w = c->bott_w; a.bott_b = c->bott_b; a.last_w = c->last_w; a.last_b = c->last_b;
  a.ll_kind = (c->kind == NIF_KIND_LASTLAYER); a.zl_rows = 32 * c->RB;
  a.WF = c->pWF; a.WB = c->pWB; a.stash = c->stash_p; a.slot_stride = c->slot_p;
  a.Z = c->Z; a.DZ = a.ll_kind ? c->DZL : c->DZ; a.ZL = c->ZL;
}
// last-layer class: the shared-weight SIREN ShapeNet x -> phi is the same MLP machinery (model.py:1219-1238)
// f32-input MFMA planes of the last-layer class's shared ShapeNet for the 32-point MLP kernels (k_pnet as the dense SIREN: the NIF_LL_MLP
// path, nets k_snet4<LL> does not take, model_x_to_phi / x_to_u_given_w).  r4: on demand -- the default training step (k_snet4<LL>) never
// reads them, and packing them after every Adam step cost L launches per step
static void ensure_ll_mlp_planes(nif_ctx* c) {
  if (c->ll_mlp_packed) return;
  const long plane_l = plane_f32x4(PLANES_T32, c->NB);
  for (int j = 0; j < c->nh; ++j) {
    long w_off, b_off; snet_mat(c, j, &w_off, &b_off);
    launch_pack(c->theta, dense_ref(w_off, c->n, c->n), c->NB, c->NB, c->lWF + j * plane_l, c->lWB + j * plane_l, c->st);
  }
  c->ll_mlp_packed = true;
}
static void fill_snet_mlp(const nif_ctx* c, PNetArgs& a, const float* xin, int ncol, int col0, long B) {
  memset(&a, 0, sizeof(a));
  a.theta = c->theta; a.xin = xin; a.ncol = ncol; a.col0 = col0; a.B = B;
  a.pi = c->si; a.nst = c->n; a.lst = c->L; a.r = c->r * c->so;
  a.act = NIF_ACT_SINE; a.res = c->cfg.s_resblock; a.siren = 1; a.omega = c->cfg.s_omega0;
  a.first_w = c->s_first_w; a.first_b = c->s_first_b;
  for (int i = 0; i < c->L; ++i) { a.hid_w[i] = c->s_hid_w[i]; a.hid_b[i] = c->s_hid_b[i]; a.hid_w2[i] = c->s_hid_w2[i]; a.hid_b2[i] = c->s_hid_b2[i]; }
  a.bott_w = c->s_bott_w; a.bott_b = c->s_bott_b; a.ll_kind = 0;
  a.WF = c->lWF; a.WB = c->lWB; a.stash = c->stash_s; a.slot_stride = c->slot_s;
  a.Z = c->PHI; a.DZ = c->DPHI; a.ZL = nullptr;
}
static void fill_ll(const nif_ctx* c, LLArgs& a, long B) {
  memset(&a, 0, sizeof(a));
  a.theta = c->theta; a.bias_off = c->ll_bias; a.last_w = c->last_w; a.loss_kind = c->loss_kind;
  a.PHI = c->PHI; a.Z = c->Z; a.B = B; a.r = c->r; a.so = c->so;
  a.DU = c->DU; a.DPHI = c->DPHI; a.DA = c->DA; a.DZL = c->DZL; a.loss_partial = c->loss_partial;
}
// last-layer class on k_snet4: slot offsets as in k_snet4's prologue (r = 0)
static void fill_snet_ll(const nif_ctx* c, SNetArgs& a, const float* xin, int ncol, int col0, long B) {
  memset(&a, 0, sizeof(a));
  const int sop = c->so * c->r;
  a.theta = c->ll_slots; a.xin = xin; a.ncol = ncol; a.col0 = col0; a.B = B; a.loss_kind = c->loss_kind;
  a.si = c->si; a.so = sop; a.n = c->n; a.nh = c->nh; a.r = 0; a.po = 0;
  a.act = NIF_ACT_SINE; a.res = c->cfg.s_resblock; a.nif_skip = 0; a.omega = c->cfg.s_omega0;
  a.off_Wh = 0; a.off_bh = 0;
  a.Z = c->Z; a.WF4 = c->sWF4; a.WB4 = c->sWB4; a.stash = c->stash_s; a.slot_stride = c->slot_s;
  a.DU = c->DU; a.DZ = nullptr; a.dring = c->dring;
  a.ll = 1; a.rl = c->r; a.so_u = c->so; a.DPHI = c->DPHI; a.DA_ll = c->DA; a.DZL = c->DZL;
  a.WPF = c->ll_wpf; a.WPB = c->ll_wpb;
  a.prec = c->opt_fp32_mfma ? 0 : policy_prec(c);     // (k_snet4<LL> only; k_sob / k_jac stay exact)
  a.WF4h = c->sWF4h; a.WB4h = c->sWB4h;
  a.WF4x = c->sWF4x; a.WB4x = c->sWB4x; a.wscale = c->sWscale;
  a.nsm = snet4_nsm_ll(c->si, sop, c->nh, c->n, c->so, c->r);
  a.tl = c->tl;
}
static void fill_snet(const nif_ctx* c, SNetArgs& a, const float* xin, int ncol, int col0, long B) {
  memset(&a, 0, sizeof(a));
  a.theta = c->theta; a.xin = xin; a.ncol = ncol; a.col0 = col0; a.B = B; a.loss_kind = c->loss_kind;
  a.si = c->si; a.so = c->so; a.n = c->n; a.nh = c->nh; a.r = c->r; a.po = c->po;
  a.act = c->kind == NIF_KIND_NIF ? c->cfg.s_act : NIF_ACT_SINE;
  a.res = c->cfg.s_resblock; a.nif_skip = (c->kind == NIF_KIND_NIF);
  a.omega = c->kind == NIF_KIND_NIF ? 1.0f : c->cfg.s_omega0;
  a.off_Wh = c->last_w; a.off_bh = c->last_b;
  a.Z = c->Z; a.WF = c->sWF; a.WB = c->sWB; a.stash = c->stash_s; a.slot_stride = c->slot_s;
  a.DU = c->DU; a.DZ = c->DZ;
  a.nsm = snet3_nsm(c->si, c->so, c->nh, c->n);
  a.WF4 = c->use_snet4 ? c->sWF4 : nullptr; a.WB4 = c->use_snet4 ? c->sWB4 : nullptr;   // packed only then
  a.WF4x = c->use_snet4 ? c->sWF4x : nullptr; a.WB4x = c->use_snet4 ? c->sWB4x : nullptr; a.wscale = c->sWscale;
  a.prec = c->opt_fp32_mfma ? 0 : policy_prec(c);
  if (!c->use_snet4) a.prec = a.prec == 2 ? 0 : a.prec;      // (no k_snet4 for this shape: the policy runs on the exact kernels)
  a.WF4h = c->use_snet4 ? c->sWF4h : nullptr; a.WB4h = c->use_snet4 ? c->sWB4h : nullptr;
  a.dring = c->dring;
  a.tl = c->tl;
}

// fp32 MFMA planes of the hidden hyper-matrices: needed by k_snet3 / k_snet (when the bf16-split kernel is not in
// use), k_jac and k_sob -- packed on demand, the training step on k_snet4 never pays for them
static int ensure_packed32(nif_ctx* c) {
  if (c->packed32 || c->kind == NIF_KIND_LASTLAYER) return NIF_OK;
  ProfScope ps_(c, NIF_PROF_PACK);
  const bool fmt16 = c->use_snet3 || c->jac_ok;     // 16-point-tile plane format (k_snet3, k_jac, k_sob) / 32-point (k_snet)
  const long plane_s = fmt16 ? plane_f32x4(PLANES_T16, snet3_nbl(c->n)) : plane_f32x4(PLANES_T32, c->NB);
  for (int j = 0; j < c->nh; ++j) {
    f32x4* wf = c->sWF + (long)j * (c->r + 1) * plane_s;
    f32x4* wb = c->sWB + (long)j * (c->r + 1) * plane_s;
    if (fmt16) launch_pack16(c->theta, hyper_w(c, 1 + j), snet3_nbl(c->n), wf, wb, c->st);
    else launch_pack(c->theta, hyper_w(c, 1 + j), c->NB, c->NB, wf, wb, c->st);
  }
  HIPCHK(hipGetLastError());
  c->packed32 = true;
  return NIF_OK;
}
// fp32 MFMA planes of the ParameterNet's hidden matrices.  A 32-wide ParameterNet (k_pnet<1>, k_pnet_bwg) splits
// its weights into bf16 operands itself, straight from theta -- the planes are then only needed by the stash-path
// adjoint (k_pnet_bwd) and k_mlpjac, and packed on demand
static int ensure_packed_p32(nif_ctx* c) {
  if (c->packed_p32) return NIF_OK;
  ProfScope ps_(c, NIF_PROF_PACK);
  const long plane_p = plane_f32x4(PLANES_T32, c->NSTB);
  for (int j = 0; j < c->nm; ++j) {
    long w_off, b_off; pnet_mat(c, j, &w_off, &b_off);
    launch_pack(c->theta, dense_ref(w_off, c->nst, c->nst), c->NSTB, c->NSTB, c->pWF + j * plane_p, c->pWB + j * plane_p, c->st);
  }
  HIPCHK(hipGetLastError());
  c->packed_p32 = true;
  return NIF_OK;
}
// the 16-bit plane sets of `nmat` hidden matrices from matrix j0 on (mstride slots apart, the first one m0), into the context's images:
// the split groups, on SIREN nets the half pairs and their scales with them, and the policy's compact set
static void pack_hidden_planes(nif_ctx* c, const MatRef& m0, long mstride, int nmat, int j0, float scale) {
  PackJob job{c->theta, m0, mstride, nmat, snet3_nbl(c->n), scale};
  job.mat0 = j0;
  job.split = {c->sWF4, c->sWB4};
  if (c->sWF4x) { job.half = {c->sWF4x, c->sWB4x}; job.pscale = c->sWscale + (size_t)j0 * (m0.r + 1) * 2; }
  if (c->sWF4h) { job.compact = {c->sWF4h, c->sWB4h}; job.compact_half = policy_prec(c) == 2; }
  launch_pack_planes(job, c->st);
}
static int ensure_packed(nif_ctx* c) {
  if (!c->have_params) return fail(NIF_ERR_STATE, "parameters not set (call nif_set_params first)");
  if (c->packed) return NIF_OK;
  c->packed_p32 = false;
  if (c->NSTB > 1) { const int rcp = ensure_packed_p32(c); if (rcp) return rcp; }
  ProfScope ps_(c, NIF_PROF_PACK);
  if (c->kind == NIF_KIND_LASTLAYER) {
    c->ll_packed32 = false;
    c->ll_mlp_packed = false;       // the f32 planes of the 32-point MLP kernels: packed when one of them runs (ensure_ll_mlp_planes)
    {
      SNetArgs probe; fill_snet_ll(c, probe, nullptr, 0, 0, 32);
      static const bool ll_old = [] { const char* e = getenv("NIF_LL_MLP"); return e && e[0] == '1'; }();
      c->use_ll4 = c->sWF4 && c->ll_slots && c->ll_wpf && c->ll_wpb && !ll_old && snet4_supported(probe);
    }
    if (c->ll_slots) {
      const int n = c->n, nh = c->nh, sop = c->so * c->r;
      LLSlotMap m; m.nseg = 0;
      auto seg = [&](long src, long dst, long len) { m.seg[m.nseg].src = src; m.seg[m.nseg].dst = dst; m.seg[m.nseg].len = len; ++m.nseg; };
      const long s_wl = (long)c->si * n + (long)nh * n * n, s_b1 = s_wl + (long)n * sop, s_bh = s_b1 + n, s_bl = s_bh + (long)nh * n;
      seg(c->s_first_w, 0, (long)c->si * n);
      seg(c->s_bott_w, s_wl, (long)n * sop);
      seg(c->s_first_b, s_b1, n);
      for (int j = 0; j < nh; ++j) {
        long w_off, b_off; snet_mat(c, j, &w_off, &b_off);
        seg(b_off, s_bh + (long)j * n, n);
        if (c->use_ll4) pack_hidden_planes(c, dense_ref(w_off, n, n), 0, 1, j, c->cfg.s_omega0);
      }
      seg(c->s_bott_b, s_bl, sop);
      seg(c->ll_bias, s_bl + sop, c->so);
      seg(c->last_w, s_bl + sop + c->so, (long)c->r * c->r);
      launch_ll_slots(c->theta, m, c->ll_slots, c->st);
      if (c->use_ll4) launch_pack_phi(c->theta, c->s_bott_w, n, sop, c->ll_wpf, c->ll_wpb, c->st);
    }
    HIPCHK(hipGetLastError());
    c->packed = true;
    return NIF_OK;
  }
  SNetArgs probe; fill_snet(c, probe, nullptr, 0, 0, 32);
  c->use_snet3 = snet3_supported(probe);
  c->jac_ok = jac_supported(probe);       // (a superset: one plane buffer when two do not fit)
  // NIF_FP32_MFMA=1 in the environment keeps every product on the f32-input MFMAs (k_snet3) for A/B runs
  const bool fp32_only = c->opt_fp32_mfma;
  // (the bf16-split kernel streams its planes in chunks: it also takes the shapes whose whole fp32 planes do not fit the LDS --
  // 128 units with latent_dim >= 3 and many matrices -- which k_snet3 / k_jac / k_sob at that width cannot)
  c->use_snet4 = c->sWF4 && !fp32_only && snet4_supported(probe);
  c->packed32 = false;
  // all hidden hyper-matrices (n^2 slots apart) in one batch: on SIREN nets ONE launch for split groups, half planes and scales (r5)
  if (c->use_snet4 && c->nh > 0) pack_hidden_planes(c, hyper_w(c, 1), hyper_wslot(c, 2) - hyper_wslot(c, 1), c->nh, 0, probe.omega);
  HIPCHK(hipGetLastError());
  c->packed = true;
  if (!c->use_snet4) return ensure_packed32(c);
  return NIF_OK;
}

// ---- last-layer class at 129..512 units: the shared SIREN ShapeNet layer by layer (k_wide.hip) -----------------------
// Layer l of the ShapeNet as the three roles see it: 0 the first layer (si -> n), 1 .. nh the hidden matrices, nh + 1 the linear
// bottleneck (n -> r so).  omega_0 multiplies the product of the sine layers only
static WideArgs wide_layer(const nif_ctx* c, int l, long B) {
  WideArgs a; memset(&a, 0, sizeof(a));
  a.theta = c->theta; a.B = B; a.ntiles = (B + 31) / 32;
  if (l == 0) { a.w_off = c->s_first_w; a.b_off = c->s_first_b; a.nin = c->si; a.nout = c->n; }
  else if (l <= c->nh) { snet_mat(c, l - 1, &a.w_off, &a.b_off); a.nin = c->n; a.nout = c->n; }
  else { a.w_off = c->s_bott_w; a.b_off = c->s_bott_b; a.nin = c->n; a.nout = c->r * c->so; }
  a.ld = a.nout;
  a.sine = l <= c->nh; a.scale = a.sine ? c->cfg.s_omega0 : 1.0f;
  return a;
}
// slot s of a buffer of n-row tiles sized for c->cap points
static float* wide_slot(const nif_ctx* c, const DevBuf<float>& buf, int s) { return buf.p + (long)s * c->n * c->cap; }
// x (columns col0 .. of xin [B][ncol]) -> c->PHI.  train: sin and cos of every layer's phase stay in wide_stash for the adjoint and the
// weight gradients; else the layers alternate between the halves of wide_act
static void wide_forward(nif_ctx* c, const float* xin, int ncol, int col0, long B, bool train) {
  const float* in = nullptr;
  for (int l = 0; l <= c->nh + 1; ++l) {
    WideArgs a = wide_layer(c, l, B);
    a.IN = in; a.xin = xin; a.ncol = ncol; a.col0 = col0;
    if (l == c->nh + 1) a.OUT = c->PHI;
    else if (train) { a.OUT = wide_slot(c, c->wide_stash, l); a.COS = wide_slot(c, c->wide_stash, c->nh + 1 + l); }
    else a.OUT = wide_slot(c, c->wide_act, l & 1);
    launch_wide_fwd(a, c->st);
    in = a.OUT;
  }
}
// Behind wide_forward(train) and the head (c->DPHI): the adjoint sweep and every ShapeNet weight gradient into `rows` partial rows.
// dL/da of layer l sits in half l & 1 of wide_act: the gradient of a layer is launched before the sweep overwrites its dL/da
static void wide_backward(nif_ctx* c, const float* xin, int ncol, int col0, long B, int rows) {
  const int nh = c->nh;
  const float* da = c->DPHI;
  for (int l = nh + 1; l >= 0; --l) {
    WideArgs a = wide_layer(c, l, B);
    a.DA = da; a.partial = c->partial; a.pstride = c->pstride;
    if (l > 0) {      // dL/da of the layer below, through this layer's matrix and that layer's cosine
      ProfScope p_(c, NIF_PROF_SNET);
      a.OUT = wide_slot(c, c->wide_act, (l - 1) & 1); a.COS = wide_slot(c, c->wide_stash, nh + 1 + (l - 1));
      launch_wide_adj(a, c->st);
    }
    {
      ProfScope p_(c, NIF_PROF_GW);
      a.IN = l > 0 ? wide_slot(c, c->wide_stash, l - 1) : nullptr; a.xin = xin; a.ncol = ncol; a.col0 = col0;
      launch_wide_gw(a, rows, c->st);
    }
    da = a.OUT;
  }
}
static int wide_refused(const nif_ctx* c, const char* who) {
  if (!c->use_wide) return NIF_OK;
  return fail(NIF_ERR_INVALID, std::string(who) + ": the derivative kernels take ShapeNets of up to 128 units (this one has " +
                                   std::to_string(c->n) + ")");
}

// The last-layer class' ShapeNet alone: phi of B points (the coordinates are columns col0 .. col0 + si of x [B][ncol]) into c->PHI,
// behind ensure_packed / ensure_capacity.  The caller holds the ProfScope, where it has one.
static void ll_phi_pass(nif_ctx* c, const float* x, int ncol, int col0, long B) {
  if (c->use_wide) wide_forward(c, x, ncol, col0, B, false);
  else { ensure_ll_mlp_planes(c); PNetArgs ma; fill_snet_mlp(c, ma, x, ncol, col0, B); launch_pnet(ma, c->NB, false, c->st); }
}

// The forward of B rows behind ensure_packed / ensure_capacity.  with_pnet: xin [B][pi + si], the ParameterNet fills Z; without (the
// snapshot entries): Z already holds every point's latent and the coordinates are columns col0 .. col0 + si of xin [B][ncol]
static int forward_rows(nif_ctx* c, const float* xin, int ncol, int col0, long B, float* u, bool with_pnet) {
  if (with_pnet) {
    PNetArgs pa; fill_pnet(c, pa, xin, B);
    ProfScope p_(c, NIF_PROF_PNET_FWD); launch_pnet(pa, c->NSTB, false, c->st);
  }
  if (c->kind == NIF_KIND_LASTLAYER) {
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    if (c->use_ll4) {
      SNetArgs sa; fill_snet_ll(c, sa, xin, ncol, col0, B);
      sa.u_out = u;
      if (launch_snet4(sa, false, false, c->st) < 0) return fail(NIF_ERR_STATE, "internal: no k_snet4 form for this net (SIREN planes not packed as half pairs)");
      HIPCHK(hipGetLastError());
      return NIF_OK;
    }
    ll_phi_pass(c, xin, ncol, col0, B);
    LLArgs la; fill_ll(c, la, B); la.u_out = u;
    launch_ll_out(la, false, c->st);
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  SNetArgs sa; fill_snet(c, sa, xin, ncol, col0, B);
  sa.u_out = u;
  {
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    if (c->use_snet4) { if (launch_snet4(sa, false, false, c->st) < 0) return fail(NIF_ERR_STATE, "internal: no k_snet4 form for this net (SIREN planes not packed as half pairs)"); }
    else if (c->use_snet3) launch_snet3(sa, false, false, nullptr, c->st);
    else launch_snet(sa, c->NB, false, c->st);
  }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_forward_dev(nif_ctx* c, const float* xin, int64_t B, float* u) {
  if (!c || !xin || !u || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  int rc = ensure_packed(c); if (rc) return rc;
  rc = ensure_capacity(c, B, false); if (rc) return rc;
  return forward_rows(c, xin, c->pi + c->si, c->pi, B, u, true);
}

static int stage(nif_ctx* c, DevBuf<float>& buf, const float* host, long n) {
  int rc = buf.reserve(c, n); if (rc) return rc;
  if (host) HIPCHK(hipMemcpyAsync(buf, host, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->st));
  return NIF_OK;
}

extern "C" int nif_forward(nif_ctx* c, const float* xin, int64_t B, float* u) {
  if (!c || !xin || !u || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  int rc = stage(c, c->d_a, xin, B * (c->pi + c->si)); if (rc) return rc;
  rc = stage(c, c->d_d, nullptr, B * c->so); if (rc) return rc;
  rc = nif_forward_dev(c, c->d_a, B, c->d_d); if (rc) return rc;
  HIPCHK(hipMemcpyAsync(u, c->d_d, sizeof(float) * (size_t)(B * c->so), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

// ---- snapshot-wise inference (k_snap.hip) --------------------------------------------------------------------
// The nets whose snapshot call is the point-wise forward on a device-built [p_t | x] table, kernel for kernel: every mixed policy and
// the shapes on the legacy k_snet family.  Everything else runs the ParameterNet once per snapshot.
static bool snap_pointwise(const nif_ctx* c) {
  if (c->cfg.mixed_policy != NIF_POLICY_FLOAT32) return true;
  return c->kind != NIF_KIND_LASTLAYER && !c->use_snet4 && !c->use_snet3;
}
// ---- the front end the snapshot calls share: nif_forward_snapshots*, nif_snapshot_normal_eq*, nif_snapshot_derivatives*,
// nif_snapshot_param_derivatives* ----
// Call geometry: T snapshots on a shared mesh of M points (off null) or on ragged meshes, snapshot t the points off[t] .. off[t + 1]
// (host memory of the caller); n points in all
struct SnapGeom { long T, M; const int64_t* off; long n; };
static int snap_geom_check(const nif_ctx* c, const void* rows, int64_t T, const void* x, const int64_t* offsets, int64_t M,
                           bool outputs_present, SnapGeom* g) {
  if (!c || !rows || T <= 0 || (offsets ? offsets[0] != 0 : M < 0)) return fail(NIF_ERR_INVALID, "bad argument");
  if (offsets) for (int64_t t = 0; t < T; ++t) if (offsets[t + 1] < offsets[t]) return fail(NIF_ERR_INVALID, "offsets must not decrease");
  *g = SnapGeom{(long)T, (long)M, offsets, offsets ? (long)offsets[T] : (long)(T * M)};
  if (g->n > 0 && (!x || !outputs_present)) return fail(NIF_ERR_INVALID, "bad argument");
  return NIF_OK;
}
// (the last check of every entry: the only refusal with NIF_ERR_STATE)
static int snap_not_capturing(const nif_ctx* c, const char* who) {
  if (c->capturing) return fail(NIF_ERR_STATE, std::string(who) + ": not capturable (inside nif_graph_begin / nif_graph_end)");
  return NIF_OK;
}
// the versioned argument structs: each says whether one of its own reserved members is set
static bool snap_reserved(const nif_encode_args& a) { return a.reserved0 != 0; }
static bool snap_reserved(const nif_snapderiv_args& a) { return a.reserved0 || a.reserved1 || a.reserved2; }
static bool snap_reserved(const nif_snapparam_args& a) { return a.reserved0 != 0; }
static bool snap_reserved(const nif_snapparam2_args&) { return false; }
static bool snap_reserved(const nif_snapfit_args& a) { return a.reserved0 != 0; }
static bool snap_reserved(const nif_sensors_args& a) { return a.reserved0 != 0; }
template <class A>
static int snap_args_check(const A* a, int version, const char* name) {
  if (!a) return fail(NIF_ERR_INVALID, "null");
  if (a->abi_version != version)
    return fail(NIF_ERR_INVALID, std::string(name) + ": abi_version " + std::to_string(a->abi_version) + " != " + std::to_string(version));
  if (snap_reserved(*a) || a->reserved[0] || a->reserved[1] || a->reserved[2] || a->reserved[3])
    return fail(NIF_ERR_INVALID, std::string(name) + ": reserved fields must be zero");
  return NIF_OK;
}
// the output rows y_idx [ny] of a derivative call, as the gather kernels take them
static int snap_y_index(const nif_ctx* c, const int32_t* y_idx, int ny, HessIdx* I) {
  if (!y_idx || ny <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  if (ny > 16) return fail(NIF_ERR_INVALID, "y_index: at most 16 entries");
  for (int i = 0; i < ny; ++i)
    if (y_idx[i] < 0 || y_idx[i] >= c->so) return fail(NIF_ERR_INVALID, "y_index out of range");
  I->ny = ny;
  for (int i = 0; i < 16; ++i) I->y_idx[i] = i < ny ? y_idx[i] : 0;
  return NIF_OK;
}
// The tangent kernels run exact products, a mixed policy's forward and ParameterNet do not: encode is refused under one, the derivative
// calls when they are given latents.
static int snap_policy_refusal(const nif_ctx* c, const char* who, bool latents) {
  if (c->cfg.mixed_policy == NIF_POLICY_FLOAT32) return NIF_OK;
  return fail(NIF_ERR_INVALID, std::string(who) + (latents ? ": latents are not built for the " : ": not built for the ") +
                                   (c->cfg.mixed_policy == NIF_POLICY_MIXED_BF16 ? "mixed_bfloat16" : "mixed_float16") +
                                   " policy (the tangent kernels run exact products, the policy's " +
                                   (latents ? "ParameterNet does not; pass p)" : "forward does not)"));
}
// What one chunk of snapshots may hold on the device (nif_set_option "snapshot_image_bytes", 0 = the default), and the snapshots of a
// chunk at per_snapshot_bytes each: at least one, at most a launch grid's 65535
#define NIF_SNAP_IMAGE_BYTES (256L << 20)
static long snap_budget(const nif_ctx* c) { return c->opt_snap_bytes > 0 ? c->opt_snap_bytes : NIF_SNAP_IMAGE_BYTES; }
static long snap_chunk(const nif_ctx* c, long T, long per_snapshot_bytes) {
  long tc = snap_budget(c) / per_snapshot_bytes;
  if (tc > 65535) tc = 65535;
  if (tc > T) tc = T;
  return tc < 1 ? 1 : tc;
}
// The chunks of at most tc_max snapshots of a call, the empty ones skipped: for (SnapWalk k{g, tc_max}; k.next();) sees the snapshots
// t0 .. t0 + tc, n_pts points in all and mmax in the longest
struct SnapWalk {
  SnapGeom g; long tc_max;
  long t0 = 0, tc = 0, mmax = 0, n_pts = 0;
  bool next() {
    for (t0 += tc; t0 < g.T; t0 += tc) {
      tc = g.T - t0 < tc_max ? g.T - t0 : tc_max;
      mmax = g.M; n_pts = tc * g.M;
      if (g.off) {
        mmax = 0; n_pts = g.off[t0 + tc] - g.off[t0];
        for (long t = t0; t < t0 + tc; ++t) if (g.off[t + 1] - g.off[t] > mmax) mmax = g.off[t + 1] - g.off[t];
      }
      if (n_pts) return true;
    }
    return false;
  }
};
static long snap_r4(long f) { return (f + 3) & ~3L; }
// The routes of a call and its slice of c->snap, one buffer with one growth: [offsets (ragged) | latent rows (from p) | the caller's extra
// head floats | the table (the point-wise route, or a shared mesh in front of a point kernel) or the combined nets of one chunk]
struct SnapPlan {
  bool pointwise;      // the point-wise kernels on the device-built [p_t | x] table, the ParameterNet per point (snap_pointwise nets, from p)
  bool combined;       // hypernetwork classes: the snapshot kernels on combined r = 0 nets, chunk by chunk
  bool phi_dot;        // last-layer class on a shared mesh: the ShapeNet once over the mesh, contracted with every snapshot's coefficients
  bool table;          // (else: the point kernels behind latent tiles built on the device)
  long off_f, lat_f, head_f;
  float *lat, *extra, *body;      // the latent rows, the extra head floats, the table or the combined nets
  SnapArgs sn;         // k_snap's expansion arguments: the geometry, x, the offsets on the device and the table
};
// phi_dot_ok / combined_ok: whether the caller's kernels have that form for this net
static void snap_routes(const nif_ctx* c, const SnapGeom& g, bool lat_in, bool phi_dot_ok, bool combined_ok, SnapPlan* P) {
  const bool ll = c->kind == NIF_KIND_LASTLAYER;
  P->pointwise = snap_pointwise(c) && !lat_in;        // (given latents never meet the ParameterNet: nothing of it to reproduce)
  P->combined = !ll && !snap_pointwise(c) && combined_ok;
  P->phi_dot = ll && !g.off && !snap_pointwise(c) && phi_dot_ok;
  P->table = P->pointwise || (!g.off && !P->phi_dot && !P->combined);
}
// the tiles of c->Z (and of the other point workspaces) that a route fills
static int snap_point_capacity(nif_ctx* c, const SnapGeom& g, const SnapPlan& P) {
  return ensure_capacity(c, P.combined ? g.T : (P.phi_dot ? (g.T > g.M ? g.T : g.M) : (g.n > g.T ? g.n : g.T)), false);
}
// Behind snap_routes: grows c->snap (and, with reserve_points, the point workspaces: the parameter-derivative call sizes those behind
// its point-wise return), uploads the offsets, lays out the slice.  tab_pi: the parameter columns in front of the table's coordinates
static int snap_plan_reserve(nif_ctx* c, const SnapGeom& g, const float* x, bool lat_in, int tab_pi, long extra_f, long combined_f,
                             bool reserve_points, SnapPlan* P) {
  P->off_f = g.off ? 2 * (g.T + 1) : 0;
  P->lat_f = (P->pointwise || lat_in) ? 0 : g.T * c->r;
  P->head_f = snap_r4(P->off_f + P->lat_f + extra_f);
  const long tab_f = P->table ? g.n * (tab_pi + c->si) : (P->combined ? combined_f : 0);
  int rc = c->snap.reserve(c, P->head_f + tab_f + 1); if (rc) return rc;
  if (reserve_points) { rc = snap_point_capacity(c, g, *P); if (rc) return rc; }
  P->lat = c->snap + P->off_f; P->extra = P->lat + P->lat_f; P->body = c->snap + P->head_f;
  SnapArgs& sn = P->sn;
  memset(&sn, 0, sizeof(sn));
  sn.T = g.T; sn.M = g.M; sn.n = g.n; sn.pi = tab_pi; sn.si = c->si; sn.r = c->r; sn.x = x;
  if (g.off) {      // (host memory of the caller: consumed before this returns)
    static_assert(sizeof(long) == sizeof(int64_t), "offsets travel as they are");
    HIPCHK(hipMemcpyAsync(c->snap.p, g.off, sizeof(int64_t) * (size_t)(g.T + 1), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    sn.offsets = reinterpret_cast<const long*>(c->snap.p);
  }
  if (P->table) sn.table = P->body;
  return NIF_OK;
}
// rows p [T][pi] -> the latent rows dst [T][r]: the ParameterNet over the T rows, its output tiles back as rows
static void snap_latents_from_p(nif_ctx* c, const float* rows, long T, float* dst) {
  PNetArgs pa; fill_pnet(c, pa, rows, T); pa.ncol = c->pi;
  { ProfScope p_(c, NIF_PROF_PNET_FWD); launch_pnet(pa, c->NSTB, false, c->st); }
  launch_tiles_to_rows(c->Z, T, c->r, dst, c->st);
}
// A chunk's combined nets as the dense r = 0 nets the snapshot kernels read: slot vectors w [tc][po], snapshot y's planes wstride units
// behind snapshot 0's (the caller sets the plane pointers of its kernel's format)
static void snap_r0_net(SNetArgs& sa, const float* w, const SnapPlan& P, const SnapWalk& k, long wstride) {
  sa.theta = w; sa.r = 0; sa.off_Wh = 0; sa.off_bh = 0; sa.Z = nullptr;
  sa.snap_off = P.sn.offsets ? P.sn.offsets + k.t0 : nullptr; sa.snap_M = k.g.M; sa.snap_wstride = wstride; sa.snap_T = (int)k.tc;
}
// The staging of a host-pointer entry: segments of c->snap_io, each rounded to whole float4s.  in: uploaded by snap_stage_in, which
// also assigns dev; out: downloaded by snap_stage_out (which waits for the stream); n floats
struct SnapSeg { const float* in; float* out; long n; float* dev; };
static int snap_stage_in(nif_ctx* c, SnapSeg* s, int k) {
  long f = 4;
  for (int i = 0; i < k; ++i) f += snap_r4(s[i].n);
  int rc = c->snap_io.reserve(c, f); if (rc) return rc;
  float* q = c->snap_io.p;
  for (int i = 0; i < k; q += snap_r4(s[i].n), ++i) {
    s[i].dev = q;
    if (s[i].in && s[i].n) HIPCHK(hipMemcpyAsync(q, s[i].in, sizeof(float) * (size_t)s[i].n, hipMemcpyHostToDevice, c->st));
  }
  return NIF_OK;
}
static int snap_stage_out(nif_ctx* c, const SnapSeg* s, int k) {
  for (int i = 0; i < k; ++i)
    if (s[i].out && s[i].n) HIPCHK(hipMemcpyAsync(s[i].out, s[i].dev, sizeof(float) * (size_t)s[i].n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

// Hypernetwork classes on k_snet4: every point of snapshot t sees the same combined matrices W_t = sum_k lat_k(t) M^(k), so the snapshot is a
// dense r = 0 net.  Per chunk of snapshots: the slot vectors w_t in fp32 from theta (the latent-to-weights kernel), their hidden matrices
// packed from w_t in the forward kernel's chunk format (one launch per hidden matrix over the whole chunk), one forward launch.
// P.body is sized by snap_combined_floats for the same tc_max.
// bytes of one combined hidden matrix's forward / adjoint image (SIREN nets: the half pairs, class NIF: the split groups), and of
// one snapshot: [slot vector | per hidden matrix: both images + its scale pair]
static void snap_combined_sizes(const nif_ctx* c, long* fb, long* bb, long* per_bytes) {
  const PlaneSet set = c->kind != NIF_KIND_NIF ? PLANES_HALF : PLANES_SPLIT;
  *fb = plane_mat_bytes(set, PLANE_FWD, c->n, 0);
  *bb = plane_mat_bytes(set, PLANE_BWD, c->n, 0);
  *per_bytes = sizeof(float) * c->po + (long)c->nh * (*fb + *bb + 2 * sizeof(float));
}
static long snap_combined_floats(const nif_ctx* c, long tc) {
  long fb, bb, per; snap_combined_sizes(c, &fb, &bb, &per);
  return snap_r4(tc * c->po) + snap_r4(2L * c->nh * tc) + tc * c->nh * (fb + bb) / (long)sizeof(float) + 4;
}
static int snap_combined(nif_ctx* c, const SnapPlan& P, const SnapGeom& g, long tc_max, const float* lat, const float* x, float* u) {
  const bool siren = c->kind != NIF_KIND_NIF;
  long fb, bb, per; snap_combined_sizes(c, &fb, &bb, &per);
  float* w = P.body;
  float* ws = w + snap_r4(tc_max * c->po);
  char* WF = reinterpret_cast<char*>(ws + snap_r4(2L * c->nh * tc_max));
  char* WB = WF + (size_t)tc_max * c->nh * fb;
  const int NBL = snet3_nbl(c->n);
  for (SnapWalk k{g, tc_max}; k.next();) {
    const long t0 = k.t0, tc = k.tc;
    SNetArgs sa; fill_snet(c, sa, x, c->si, 0, k.n_pts);
    {
      ProfScope p_(c, NIF_PROF_PACK);
      launch_latent_to_w(c->theta, c->last_w, c->last_b, c->r, c->po, lat + t0 * c->r, tc, w, c->st);
      for (int j = 0; j < c->nh; ++j) {       // matrix j of every snapshot of the chunk: images [snapshot][matrix], scales [matrix][snapshot]
        PackJob job{w, dense_ref(hyper_wslot(c, 1 + j), c->n, c->n), c->po, (int)tc, NBL, sa.omega};
        job.mat0 = j; job.dstep = c->nh;
        (siren ? job.half : job.split) = {WF, WB};
        job.pscale = ws + (long)j * tc * 2;
        launch_pack_planes(job, c->st);
      }
    }
    snap_r0_net(sa, w, P, k, c->nh * fb / PLANE_UNIT_BYTES);
    sa.WF4 = WF; sa.wscale = siren ? ws : nullptr;
    sa.u_out = g.off ? u : u + t0 * g.M * c->so;
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    if (launch_snet4_snap(sa, tc, k.mmax, c->st) < 0) return fail(NIF_ERR_STATE, "internal: no snapshot form of k_snet4 for this net");
  }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}

static int snap_check(const nif_ctx* c, const void* rows, int64_t T, const void* x, const int64_t* offsets, int64_t M, const void* u,
                      SnapGeom* g) {
  int rc = snap_geom_check(c, rows, T, x, offsets, M, u != nullptr, g); if (rc) return rc;
  return snap_not_capturing(c, "nif_forward_snapshots");
}
extern "C" int nif_forward_snapshots_dev(nif_ctx* c, const float* rows, int32_t rows_are_latent, int64_t T, const float* x,
                                         const int64_t* offsets, int64_t M, float* u) {
  SnapGeom g;
  int rc = snap_check(c, rows, T, x, offsets, M, u, &g); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  rc = ensure_packed(c); if (rc) return rc;
  if (g.n == 0) return NIF_OK;
  const bool lat_in = rows_are_latent != 0;
  SnapPlan P;
  snap_routes(c, g, lat_in, phi_dot_supported(c->r, c->so), c->use_snet4, &P);
  long tc_max = 0;
  if (P.combined) { long fb, bb, per; snap_combined_sizes(c, &fb, &bb, &per); tc_max = snap_chunk(c, g.T, per); }
  // (the table always carries the parameter columns here: forward_rows reads it in the full model's layout on either route)
  rc = snap_plan_reserve(c, g, x, lat_in, c->pi, 0, P.combined ? snap_combined_floats(c, tc_max) : 0, true, &P); if (rc) return rc;
  SnapArgs& sn = P.sn;
  if (P.pointwise) {
    sn.p = rows;
    launch_snap_expand(sn, c->st);
    return forward_rows(c, sn.table, c->pi + c->si, c->pi, g.n, u, true);
  }
  const float* lat = rows;
  if (!lat_in) { snap_latents_from_p(c, rows, g.T, P.lat); lat = P.lat; }
  if (P.combined) return snap_combined(c, P, g, tc_max, lat, x, u);
  if (P.phi_dot) {      // one ShapeNet pass over the mesh for all snapshots
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    ll_phi_pass(c, x, c->si, 0, g.M);
    launch_phi_dot(c->PHI, lat, c->theta + c->ll_bias, g.T, g.M, c->r, c->so, u, c->st);
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  sn.lat = lat; sn.Z = c->Z;
  launch_snap_expand(sn, c->st);
  if (P.table) return forward_rows(c, sn.table, c->pi + c->si, c->pi, g.n, u, false);
  return forward_rows(c, x, c->si, 0, g.n, u, false);
}
extern "C" int nif_forward_snapshots(nif_ctx* c, const float* rows, int32_t rows_are_latent, int64_t T, const float* x,
                                     const int64_t* offsets, int64_t M, float* u) {
  SnapGeom g;
  int rc = snap_check(c, rows, T, x, offsets, M, u, &g); if (rc) return rc;
  const long n = g.n;
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  if (n == 0) return ensure_packed(c);
  rc = stage(c, c->d_a, rows, T * (rows_are_latent ? c->r : c->pi)); if (rc) return rc;
  rc = stage(c, c->d_b, x, (offsets ? n : (long)M) * c->si); if (rc) return rc;
  rc = stage(c, c->d_d, nullptr, n * c->so); if (rc) return rc;
  rc = nif_forward_snapshots_dev(c, c->d_a, rows_are_latent, T, c->d_b, offsets, M, c->d_d); if (rc) return rc;
  HIPCHK(hipMemcpyAsync(u, c->d_d, sizeof(float) * (size_t)(n * c->so), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

// ---- per-snapshot normal equations in the latent (k_encode.hip, include/nif_hip_encode.h) --------------------------
static int enc_check(const nif_encode_args* a, SnapGeom* g) {
  int rc = snap_args_check(a, NIF_ENCODE_ABI_VERSION, "nif_encode_args"); if (rc) return rc;
  const nif_ctx* c = a->ctx;
  rc = snap_geom_check(c, a->latents, a->T, a->x, a->offsets_host, a->M, a->y != nullptr, g); if (rc) return rc;
  if (!a->S_out) return fail(NIF_ERR_INVALID, "bad argument");
  rc = snap_policy_refusal(c, "nif_snapshot_normal_eq", false); if (rc) return rc;
  if (c->r > 64) return fail(NIF_ERR_INVALID, "nif_snapshot_normal_eq: latent_dim " + std::to_string(c->r) + " > 64");
  return snap_not_capturing(c, "nif_snapshot_normal_eq");
}
// floats per padded point of a chunk: what encode holds in c->enc, and for the last-layer class what ensure_capacity holds besides
static long enc_point_floats(const nif_ctx* c) {
  if (c->kind == NIF_KIND_LASTLAYER) return c->si + 2L * c->r * c->so + 3L * c->r + c->so + (c->use_wide ? 2L * c->n : 0);
  return 2L * c->r + c->si + (long)c->so * c->r + c->so;
}
extern "C" int nif_snapshot_normal_eq_dev(const nif_encode_args* a) {
  SnapGeom g;
  int rc = enc_check(a, &g); if (rc) return rc;
  const long n = g.n;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  rc = ensure_packed(c); if (rc) return rc;
  const bool ll = c->kind == NIF_KIND_LASTLAYER;
  if (!ll) {
    if (!c->jac_ok) return fail(NIF_ERR_INVALID, "nif_snapshot_normal_eq: one weight plane and the small hyper-vectors of this shape exceed the 160 KB LDS of a CU (the JacobianLayer kernels do not take it)");
    rc = ensure_packed32(c); if (rc) return rc;
  }
  const long T = a->T, M = a->M;
  const int r = c->r, so = c->so, si = c->si;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(a->S_out, 0, sizeof(double) * (size_t)(T * (r + 1) * (r + 1)), c->st));
    return NIF_OK;
  }
  const int64_t* off = a->offsets_host;
  const bool shared_phi = ll && !off;      // one ShapeNet pass over the mesh for all snapshots, no padded copy of anything
  // the padded layout: snapshot t owns the tiles tile_start[t] .. tile_start[t + 1]
  static_assert(sizeof(long) == sizeof(int64_t), "offsets travel as they are");
  std::vector<long> meta(2 * (T + 1));
  long* tile_start = meta.data();
  long* offs = tile_start + T + 1;
  tile_start[0] = 0;
  for (long t = 0; t < T; ++t) {
    offs[t] = off ? off[t] : t * M;
    tile_start[t + 1] = tile_start[t] + ((off ? off[t + 1] - off[t] : M) + 31) / 32;
  }
  offs[T] = n;
  // chunks of whole snapshots within the budget of nif_forward_snapshots' images (at least one snapshot each)
  const long ppf = enc_point_floats(c);
  long tiles_budget = snap_budget(c) / (long)(sizeof(float) * 32 * ppf);
  if (tiles_budget < 1) tiles_budget = 1;
  std::vector<long> cuts{0};
  long tiles_max = 0;
  if (shared_phi) cuts.push_back(T);
  else
    for (long t = 0; t < T;) {
      long t1 = t + 1;
      while (t1 < T && tile_start[t1 + 1] - tile_start[t] <= tiles_budget) ++t1;
      if (tile_start[t1] - tile_start[t] > tiles_max) tiles_max = tile_start[t1] - tile_start[t];
      cuts.push_back(t1);
      t = t1;
    }
  const long meta_f = snap_r4(2 * (long)meta.size());
  const long pts_max = tiles_max * 32;
  const long f_z = ll ? 0 : pts_max * r, f_unit = ll ? 0 : pts_max * r + 32L * r, f_x = pts_max * si;
  const long f_dydx = ll ? 0 : pts_max * so * r, f_u = ll ? 0 : pts_max * so;
  rc = c->enc.reserve(c, meta_f + f_z + f_unit + f_x + f_dydx + f_u + 4); if (rc) return rc;
  if (ll) { rc = ensure_capacity(c, shared_phi ? M : pts_max, false); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(c->enc.p, meta.data(), sizeof(long) * meta.size(), hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));      // (host memory of this call: consumed before it returns)
  EncArgs ea; memset(&ea, 0, sizeof(ea));
  ea.tile_start = reinterpret_cast<const long*>(c->enc.p);
  ea.offsets = off ? ea.tile_start + T + 1 : nullptr;
  ea.M = M; ea.lat = a->latents; ea.x = a->x; ea.r = r; ea.si = si; ea.so = so;
  ea.y = a->y; ea.w = a->w; ea.S = a->S_out;
  float* Z = c->enc + meta_f;
  float* unit = Z + f_z;
  float* xpad = unit + f_unit;
  float* dydx = xpad + f_x;
  float* u = dydx + f_dydx;
  if (ll) { ea.PHI = c->PHI; ea.bias = c->theta + c->ll_bias; ea.phi_shared = shared_phi; }
  else { ea.dydx = dydx; ea.u = u; }
  auto phi_pass = [&](const float* xs, long B) {      // x -> phi of B points into c->PHI, as nif_x_to_phi runs it
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    ll_phi_pass(c, xs, si, 0, B);
  };
  if (shared_phi) phi_pass(a->x, M);
  for (size_t ci = 0; ci + 1 < cuts.size(); ++ci) {
    ea.t0 = cuts[ci]; ea.t1 = cuts[ci + 1];
    const long ntiles = shared_phi ? 0 : tile_start[ea.t1] - tile_start[ea.t0];
    if (!shared_phi && ntiles > 0) {
      EncArgs ex = ea;
      ex.xpad = xpad;
      if (!ll) { ex.Z = Z; ex.unit = unit; }
      { ProfScope p_(c, NIF_PROF_PACK); launch_encode_expand(ex, ntiles, c->st); }
      if (ll) phi_pass(xpad, ntiles * 32);
      else {
        // du/dz_k = k_jac's parameter-seed stream seeded with the unit tile e_k: three latents per launch, the primal with the first
        ProfScope p_(c, NIF_PROF_SNET_FWD);
        SNetArgs sa; fill_snet(c, sa, xpad, si, 0, ntiles * 32);
        sa.Z = Z;
        for (int k0 = 0; k0 < r; k0 += 3) {
          int seeds[3] = {-1, -1, -1};
          const float* zd[3] = {nullptr, nullptr, nullptr};
          const int ns = r - k0 < 3 ? r - k0 : 3;
          for (int d = 0; d < ns; ++d) zd[d] = unit + (long)((r - (k0 + d)) % r) * 32;
          sa.u_out = k0 == 0 ? u : nullptr;
          launch_jac(sa, ns, seeds, zd, r, k0, dydx, c->st);
        }
      }
    }
    ProfScope p_(c, NIF_PROF_REDUCE);
    launch_encode_gram(ea, c->st);
  }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_snapshot_normal_eq(const nif_encode_args* a) {
  SnapGeom g;
  int rc = enc_check(a, &g); if (rc) return rc;
  const long n = g.n;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  const long T = a->T, e = (long)(c->r + 1) * (c->r + 1);
  rc = stage(c, c->d_a, a->latents, T * c->r); if (rc) return rc;
  rc = c->enc_S.reserve(c, T * e); if (rc) return rc;
  nif_encode_args d = *a;
  d.latents = c->d_a; d.S_out = c->enc_S;
  if (n > 0) {
    rc = stage(c, c->d_b, a->x, (a->offsets_host ? n : (long)a->M) * c->si); if (rc) return rc;
    rc = stage(c, c->d_d, a->y, n * c->so); if (rc) return rc;
    if (a->w) { rc = stage(c, c->d_c, a->w, n); if (rc) return rc; }
    d.x = c->d_b; d.y = c->d_d; d.w = a->w ? c->d_c.p : nullptr;
  }
  rc = nif_snapshot_normal_eq_dev(&d); if (rc) return rc;
  HIPCHK(hipMemcpyAsync(a->S_out, c->enc_S, sizeof(double) * (size_t)(T * e), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

// The device core of nif_jacobian: xin_dev [B][pi + si] -> y [B][so] in c->d_d and dy/dx of EVERY output, [B][so][nx], in c->d_b, all
// enqueued on the context's stream.  The snapshot entries (nif_snapshot_param_derivatives*) run it on a table built on the device.
static int jacobian_core(nif_ctx* c, const float* xin_dev, int64_t B, const int32_t* x_idx, int32_t nx) {
  int rc = ensure_packed(c); if (rc) return rc;
  rc = ensure_packed32(c); if (rc) return rc;
  rc = ensure_packed_p32(c); if (rc) return rc;
  const bool ll = c->kind == NIF_KIND_LASTLAYER;
  if (!ll && !c->jac_ok) return fail(NIF_ERR_INVALID, "JacobianLayer: one weight plane and the small hyper-vectors of this shape exceed the 160 KB LDS of a CU");
  rc = ensure_capacity(c, B, false); if (rc) return rc;
  const long ntiles = (B + 31) / 32;
  const int ncol = c->pi + c->si;
  rc = stage(c, c->d_d, nullptr, B * c->so); if (rc) return rc;
  rc = stage(c, c->d_b, nullptr, B * c->so * nx); if (rc) return rc;
  // tangent buffers: dz/dp for up to 3 parameter seeds (and d phi / dx for the last-layer class)
  const long zd_sz = ntiles * 32 * (long)c->r * (ll ? c->so : 1);
  rc = c->d_c.reserve(c, 3 * zd_sz); if (rc) return rc;
  PNetArgs pa; fill_pnet(c, pa, xin_dev, B);
  if (ll) {
    // u = Dot(phi(x), a(p)) + bias: coordinate columns move phi, parameter columns move a
    rc = nif_forward_dev(c, xin_dev, B, c->d_d); if (rc) return rc;     // leaves Z (= a) on the device
    ensure_ll_mlp_planes(c); PNetArgs ma; fill_snet_mlp(c, ma, xin_dev, ncol, c->pi, B);
    if (c->use_ll4) launch_pnet(ma, c->NB, false, c->st);               // the fused forward keeps phi on chip: compute it here
    for (int j = 0; j < nx; ++j) {
      if (x_idx[j] >= c->pi) {
        PNetArgs mj = ma; mj.Z = c->DPHI;   // primal again into a scratch, tangent into d_c
        launch_mlp_jac(mj, c->NB, x_idx[j] - c->pi, c->d_c, c->st);
        launch_ll_jac_out(c->PHI, c->Z, c->d_c, nullptr, B, c->r, c->so, nx, j, c->d_b, c->st);
      } else {
        PNetArgs pj = pa; pj.Z = c->DA;
        launch_mlp_jac(pj, c->NSTB, x_idx[j], c->d_c, c->st);
        launch_ll_jac_out(c->PHI, c->Z, nullptr, c->d_c, B, c->r, c->so, nx, j, c->d_b, c->st);
      }
    }
  } else {
    launch_pnet(pa, c->NSTB, false, c->st);
    SNetArgs sa; fill_snet(c, sa, xin_dev, ncol, c->pi, B);
    for (int x0 = 0; x0 < nx; x0 += 3) {
      int seeds[3] = {0, 0, 0};
      const float* zd[3] = {nullptr, nullptr, nullptr};
      const int ns = nx - x0 < 3 ? nx - x0 : 3;
      for (int d = 0; d < ns; ++d) {
        const int col = x_idx[x0 + d];
        if (col >= c->pi) { seeds[d] = col - c->pi; }
        else {
          seeds[d] = -1;
          PNetArgs pj = pa; pj.Z = c->DZ;     // primal latent again into a scratch
          launch_mlp_jac(pj, c->NSTB, col, c->d_c + d * zd_sz, c->st);
          zd[d] = c->d_c + d * zd_sz;
        }
      }
      sa.u_out = x0 == 0 ? c->d_d : nullptr;
      launch_jac(sa, ns, seeds, zd, nx, x0, c->d_b, c->st);
    }
  }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_jacobian(nif_ctx* c, const float* xin, int64_t B, const int32_t* y_idx, int32_t ny,
                            const int32_t* x_idx, int32_t nx, float* y_out, float* dydx_out) {
  if (!c || !xin || !y_idx || !x_idx || !y_out || !dydx_out || B <= 0 || ny <= 0 || nx <= 0)
    return fail(NIF_ERR_INVALID, "bad argument");
  for (int i = 0; i < ny; ++i)
    if (y_idx[i] < 0 || y_idx[i] >= c->so) return fail(NIF_ERR_INVALID, "y_index out of range");
  for (int j = 0; j < nx; ++j)
    if (x_idx[j] < 0 || x_idx[j] >= c->pi + c->si) return fail(NIF_ERR_INVALID, "x_index out of range");
  { const int rcw = wide_refused(c, "JacobianLayer"); if (rcw) return rcw; }
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  int rc = stage(c, c->d_a, xin, B * (c->pi + c->si)); if (rc) return rc;
  rc = jacobian_core(c, c->d_a, B, x_idx, nx); if (rc) return rc;
  std::vector<float> full((size_t)B * c->so * nx);
  HIPCHK(hipMemcpyAsync(y_out, c->d_d, sizeof(float) * (size_t)(B * c->so), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(full.data(), c->d_b, sizeof(float) * full.size(), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  for (int64_t a_ = 0; a_ < B; ++a_)
    for (int i = 0; i < ny; ++i)
      for (int j = 0; j < nx; ++j) dydx_out[(a_ * ny + i) * nx + j] = full[((size_t)a_ * c->so + y_idx[i]) * nx + j];
  return NIF_OK;
}

// HessianLayer (gradient.py:130-180, :234-261): y [B, so], dy/dx [B, ny, nx] and d2y/dx2 [B, ny, nx, nx] for ANY input columns
// x_idx: one launch of the second-order tangent kernel per column pair (j <= k), then the gather of the rows y_idx -- and, for the
// last-layer class, the contraction with the ParameterNet output -- ON THE DEVICE (r3; r2 did both in host loops).  Everything is
// enqueued on the context's stream; the outputs are device pointers.
// The snapshot entries (nif_snapshot_derivatives*) run it behind latents of their own: with_pnet false, c->Z already holds every point's
// latent, xin_dev is [B][si] (coordinate columns only in x_idx, still numbered from pi_dim).  ll_tangents_only (last-layer class):
// stop behind the ShapeNet tangents phi, phi', phi'' of the B points in c->d_d, c->d_b, c->d_c; the caller contracts them.
static int hessian_core(nif_ctx* c, const float* xin_dev, int64_t B, const int32_t* y_idx, int32_t ny, const int32_t* x_idx,
                        int32_t nx, float* y_dev, float* dydx_dev, float* d2_dev, bool with_pnet = true, bool ll_tangents_only = false) {
  bool anyp = false;
  for (int j = 0; j < nx; ++j) anyp = anyp || x_idx[j] < c->pi;
  if (anyp && !with_pnet) return fail(NIF_ERR_INVALID, "internal: parameter columns need the ParameterNet");
  int rc = ensure_packed(c); if (rc) return rc;
  rc = ensure_capacity(c, B, false); if (rc) return rc;
  const int ncol = with_pnet ? c->pi + c->si : c->si, col0 = with_pnet ? c->pi : 0;
  const long ntl = (B + 31) / 32;
  HessIdx I; I.ny = ny;
  for (int i = 0; i < 16; ++i) I.y_idx[i] = i < ny ? y_idx[i] : 0;
  PNetArgs pa; fill_pnet(c, pa, xin_dev, B);
  if (with_pnet) launch_pnet(pa, c->NSTB, false, c->st);
  // parameter columns: z' = dz/dp of every parameter column once (k_pjac, forward mode), z'' per pair of them (k_pjac2)
  std::vector<int> xc, xp;                         // positions (in x_idx) of the coordinate / parameter columns
  for (int j = 0; j < nx; ++j) (x_idx[j] >= c->pi ? xc : xp).push_back(j);
  const int np_ = (int)xp.size();
  if (xc.size() > 16 || np_ > 16) return fail(NIF_ERR_INVALID, "HessianLayer: at most 16 coordinate and 16 parameter columns in x_index");
  const long blk = ntl * 32 * c->r;                // floats of one latent-layout vector
  if (anyp) {
    if (!pjac_supported(pa))
      return fail(NIF_ERR_INVALID, "HessianLayer on parameter columns: ParameterNets of up to 128 units");
    const long need_zt = (long)c->pi * blk, need_dd = (long)np_ * np_ * blk;
    rc = c->zt_par.reserve(c, need_zt); if (rc) return rc;
    rc = c->dzt_par.reserve(c, need_dd); if (rc) return rc;
    launch_pjac_fwd(pa, c->zt_par, c->st);
  }
  auto zt_of = [&](int col) -> const float* { return c->zt_par + (long)col * blk; };
  auto zdd_of = [&](int j, int k) -> float* { return c->dzt_par + (long)(j * np_ + k) * blk; };   // pair of xp positions, j <= k
  if (c->kind == NIF_KIND_LASTLAYER) {
    // u_i = sum_c phi[i,c](x) a_c(p) + bias_i: the coordinates only move phi (second-order tangents of the shared SIREN ShapeNet,
    // the r = 0 case of the same kernel with so * latent_dim outputs), the parameters only move a = latent last_w + last_b
    const int rl = c->r, sop = c->so * c->r;
    const int nxc = xc.empty() ? 1 : (int)xc.size();
    rc = stage(c, c->d_d, nullptr, B * sop); if (rc) return rc;
    rc = stage(c, c->d_b, nullptr, B * sop * nxc); if (rc) return rc;
    rc = stage(c, c->d_c, nullptr, B * sop * nxc * nxc); if (rc) return rc;
    SNetArgs sa; rc = fill_snet_ll_sob(c, sa, xin_dev, B, true); if (rc) return rc;
    sa.ncol = ncol; sa.col0 = col0;
    if (xc.empty()) { sa.u_out = c->d_d; launch_hess(sa, 0, 0, 0, 0, 1, c->d_b, c->d_c, c->st); }     // phi alone
    for (size_t j = 0; j < xc.size(); ++j)
      for (size_t k = j; k < xc.size(); ++k) {
        sa.u_out = (j == 0 && k == 0) ? c->d_d : nullptr;
        launch_hess(sa, x_idx[xc[j]] - c->pi, x_idx[xc[k]] - c->pi, (int)j, (int)k, nxc, c->d_b, c->d_c, c->st);
      }
    if (ll_tangents_only) { HIPCHK(hipGetLastError()); return NIF_OK; }
    // a'_j = z'_j last_w and a''_jk = z''_jk last_w: one k_pjac2 launch per parameter pair, ONE k_through_lw over all of them
    const int nvec = np_ + np_ * np_;
    float* ap = nullptr;
    if (nvec > 0) {
      const long need = (long)nvec * blk + 2L * nvec + 2;      // + the nvec source offsets (longs, as raw bytes behind the vectors)
      rc = c->jac_mu.reserve(c, need); if (rc) return rc;
      ap = c->jac_mu;
      for (int j = 0; j < np_; ++j)
        for (int k = j; k < np_; ++k) launch_pjac2(pa, x_idx[xp[j]], x_idx[xp[k]], zdd_of(j, k), c->st);
      // source of vector v: z'_j inside zt_par, z''_jk inside dzt_par -- addressed relative to zt_par (both are device arrays of floats)
      std::vector<long> off(nvec, 0);
      for (int j = 0; j < np_; ++j) off[j] = (long)(zt_of(x_idx[xp[j]]) - c->zt_par);
      for (int j = 0; j < np_; ++j)
        for (int k = 0; k < np_; ++k) off[np_ + j * np_ + k] = (long)(zdd_of(j < k ? j : k, j < k ? k : j) - c->zt_par);
      long* off_dev = reinterpret_cast<long*>(ap + (long)nvec * blk);
      HIPCHK(hipMemcpyAsync(off_dev, off.data(), sizeof(long) * nvec, hipMemcpyHostToDevice, c->st));
      HIPCHK(hipStreamSynchronize(c->st));            // (off is a host temporary)
      launch_through_lw(c->zt_par, off_dev, nvec, c->theta + c->last_w, rl, ntl * 32, ap, c->st);
    }
    HessLLArgs H;
    memset(&H, 0, sizeof(H));
    H.f0 = c->d_d; H.fj = c->d_b; H.fh = c->d_c; H.Za = c->Z; H.AP = ap; H.bias = c->theta + c->ll_bias;
    H.B = B; H.npts = ntl * 32; H.so = c->so; H.rl = rl; H.nxc = (int)xc.size(); H.np = np_; H.nx = nx; H.I = I;
    for (size_t j = 0; j < xc.size(); ++j) H.xc[j] = xc[j];
    for (int j = 0; j < np_; ++j) H.xp[j] = xp[j];
    H.y = y_dev; H.dydx = dydx_dev; H.d2 = d2_dev;
    launch_ll_hess(H, c->st);
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  rc = ensure_packed32(c); if (rc) return rc;
  if (!c->jac_ok) return fail(NIF_ERR_INVALID, "HessianLayer: one weight plane and the small hyper-vectors of this shape exceed the 160 KB LDS of a CU");
  rc = stage(c, c->d_b, nullptr, B * c->so * nx); if (rc) return rc;
  rc = stage(c, c->d_c, nullptr, B * c->so * nx * nx); if (rc) return rc;
  SNetArgs sa; fill_snet(c, sa, xin_dev, ncol, col0, B);
  std::vector<int> ppos(nx, -1);                    // position among the parameter columns of x_idx
  for (int j = 0; j < np_; ++j) ppos[xp[j]] = j;
  for (int j = 0; j < nx; ++j)
    for (int k = j; k < nx; ++k) {
      sa.u_out = (j == 0 && k == 0) ? y_dev : nullptr;
      const bool pj = x_idx[j] < c->pi, pk = x_idx[k] < c->pi;
      float* zdd = (pj && pk) ? zdd_of(ppos[j], ppos[k]) : nullptr;
      if (pj && pk) launch_pjac2(pa, x_idx[j], x_idx[k], zdd, c->st);
      launch_hess(sa, pj ? -1 : x_idx[j] - c->pi, pk ? -1 : x_idx[k] - c->pi, j, k, nx, c->d_b, c->d_c, c->st,
                  pj ? zt_of(x_idx[j]) : nullptr, pk ? zt_of(x_idx[k]) : nullptr, zdd);
    }
  launch_hess_gather(c->d_b, c->d_c, B, c->so, nx, I, dydx_dev, d2_dev, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}

static int hessian_check(nif_ctx* c, const void* xin, int64_t B, const int32_t* y_idx, int32_t ny, const int32_t* x_idx, int32_t nx,
                         const void* y_out, const void* dydx_out, const void* d2_out) {
  if (!c || !xin || !y_idx || !x_idx || !y_out || !dydx_out || !d2_out || B <= 0 || ny <= 0 || nx <= 0)
    return fail(NIF_ERR_INVALID, "bad argument");
  if (ny > 16) return fail(NIF_ERR_INVALID, "y_index: at most 16 entries");
  for (int i = 0; i < ny; ++i)
    if (y_idx[i] < 0 || y_idx[i] >= c->so) return fail(NIF_ERR_INVALID, "y_index out of range");
  for (int j = 0; j < nx; ++j)
    if (x_idx[j] < 0 || x_idx[j] >= c->pi + c->si) return fail(NIF_ERR_INVALID, "x_index out of range (0 <= i < pi_dim + si_dim)");
  return wide_refused(c, "HessianLayer");
}
extern "C" int nif_hessian_dev(nif_ctx* c, const float* xin_dev, int64_t B, const int32_t* y_idx, int32_t ny, const int32_t* x_idx,
                               int32_t nx, float* y_dev, float* dydx_dev, float* d2_dev) {
  int rc = hessian_check(c, xin_dev, B, y_idx, ny, x_idx, nx, y_dev, dydx_dev, d2_dev); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  return hessian_core(c, xin_dev, B, y_idx, ny, x_idx, nx, y_dev, dydx_dev, d2_dev);
}
extern "C" int nif_hessian(nif_ctx* c, const float* xin, int64_t B, const int32_t* y_idx, int32_t ny, const int32_t* x_idx,
                           int32_t nx, float* y_out, float* dydx_out, float* d2_out) {
  int rc = hessian_check(c, xin, B, y_idx, ny, x_idx, nx, y_out, dydx_out, d2_out); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  rc = stage(c, c->d_a, xin, B * (c->pi + c->si)); if (rc) return rc;
  const size_t n_y = (size_t)B * c->so, n_d = (size_t)B * ny * nx, n_h = n_d * nx;
  DevBuf<float> out;      // this call's own device copy of the three outputs
  rc = out.alloc((long)(n_y + n_d + n_h)); if (rc) return rc;
  rc = hessian_core(c, c->d_a, B, y_idx, ny, x_idx, nx, out, out + n_y, out + n_y + n_d);
  if (rc == NIF_OK) {
    hipError_t e = hipMemcpyAsync(y_out, out, sizeof(float) * n_y, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipMemcpyAsync(dydx_out, out + n_y, sizeof(float) * n_d, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipMemcpyAsync(d2_out, out + n_y + n_d, sizeof(float) * n_h, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) rc = fail(NIF_ERR_HIP, hipGetErrorString(e));
  } else (void)hipStreamSynchronize(c->st);
  return rc;
}

// ---- snapshot-wise derivatives (include/nif_hip_snapderiv.h) ---------------------------------------------------------
static int sd_check(const nif_snapderiv_args* a, SnapGeom* g, HessIdx* I) {
  int rc = snap_args_check(a, NIF_SNAPDERIV_ABI_VERSION, "nif_snapderiv_args"); if (rc) return rc;
  const nif_ctx* c = a->ctx;
  rc = snap_geom_check(c, a->rows, a->T, a->x, a->offsets_host, a->M, a->u && a->dudx && (a->order != 2 || a->d2udx2), g); if (rc) return rc;
  if (a->order != 1 && a->order != 2) return fail(NIF_ERR_INVALID, "nif_snapshot_derivatives: order must be 1 or 2");
  rc = snap_y_index(c, a->y_idx, a->ny, I); if (rc) return rc;
  if (!a->x_idx || a->nx <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  for (int j = 0; j < a->nx; ++j) {
    if (a->x_idx[j] < 0 || a->x_idx[j] >= c->si) return fail(NIF_ERR_INVALID, "x_index out of range (0 <= j < si_dim: coordinates only)");
    for (int k = 0; k < j; ++k) if (a->x_idx[k] == a->x_idx[j]) return fail(NIF_ERR_INVALID, "x_index: an index is repeated");
  }
  if (a->nx > 16) return fail(NIF_ERR_INVALID, "HessianLayer: at most 16 coordinate and 16 parameter columns in x_index");
  { const int rcw = wide_refused(c, "nif_snapshot_derivatives"); if (rcw) return rcw; }
  return snap_not_capturing(c, "nif_snapshot_derivatives");
}
// One snapshot of the tangent kernels' combined path: its slot vector and the forward f32 planes of its hidden matrices (the format
// k_jac reads), each with g more beside it for the direction streams of a launch group (k_jac_wt; the coordinate derivatives: g = 0):
// slot vectors [1 + g][tc][po], then per snapshot and hidden matrix the 1 + g planes [W_j | W'_0,j | ..]
static long sd_plane_f32x4(const nif_ctx* c) { return plane_f32x4(PLANES_T16, snet3_nbl(c->n)); }
static long sp_snapshot_bytes(const nif_ctx* c, int g) {
  return (1 + g) * ((long)sizeof(float) * c->po + (long)c->nh * sd_plane_f32x4(c) * (long)sizeof(f32x4));
}
static long sp_combined_floats(const nif_ctx* c, long tc, int g) { return snap_r4((1 + g) * tc * c->po) + (1 + g) * tc * c->nh * sd_plane_f32x4(c) * 4 + 4; }
// the slot vectors w [tc][po] in fp32 from the latent rows of a chunk and their hidden matrices as f32 planes (one launch per hidden
// matrix over the chunk): matrix j of snapshot y at WF + (y nh + j) ps planes
static void snap_pack_f32(nif_ctx* c, const float* lat, long tc, float* w, f32x4* WF, int ps) {
  const long plane_s = sd_plane_f32x4(c);
  ProfScope p_(c, NIF_PROF_PACK);
  launch_latent_to_w(c->theta, c->last_w, c->last_b, c->r, c->po, lat, tc, w, c->st);
  for (int j = 0; j < c->nh; ++j)
    launch_pack16_fwd_batch(w, dense_ref(hyper_wslot(c, 1 + j), c->n, c->n), c->po, (int)tc, snet3_nbl(c->n), WF + (long)j * ps * plane_s,
                            c->nh * ps * plane_s, c->st);
}
// Hypernetwork classes on k_jac_snap.  Per chunk of snapshots: the slot vectors and planes (snap_pack_f32), then one launch per seed
// group over the chunk.  The kernels leave every output row [n][so][nx] / [n][so][nx][nx] in c->d_b / c->d_c; the rows y_idx are
// gathered behind the last chunk.
static int sd_combined(nif_ctx* c, const nif_snapderiv_args* a, const SnapPlan& P, const SnapGeom& g, long tc_max, const float* lat,
                       const HessIdx& I) {
  const long n = g.n;
  const int nx = a->nx, so = c->so;
  const bool hess = a->order == 2;
  int rc = stage(c, c->d_b, nullptr, n * so * nx); if (rc) return rc;
  if (hess) { rc = stage(c, c->d_c, nullptr, n * so * nx * nx); if (rc) return rc; }
  float* w = P.body;
  f32x4* WF = reinterpret_cast<f32x4*>(w + snap_r4(tc_max * c->po));
  for (SnapWalk k{g, tc_max}; k.next();) {
    const long tc = k.tc;
    snap_pack_f32(c, lat + k.t0 * c->r, tc, w, WF, 1);
    SNetArgs sa; fill_snet(c, sa, a->x, c->si, 0, k.mmax);
    snap_r0_net(sa, w, P, k, c->nh * sd_plane_f32x4(c));
    sa.WF = WF; sa.WB = nullptr;
    // (ragged: the kernel rebases by the call's own offsets; shared mesh: by t M inside the chunk)
    const long pb = g.off ? 0 : k.t0 * g.M;
    float* u = a->u + pb * so;
    float* fj = c->d_b + pb * so * nx;
    float* fh = hess ? c->d_c + pb * so * nx * nx : nullptr;
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    if (hess) {
      for (int j = 0; j < nx; ++j)
        for (int k = j; k < nx; ++k) {
          sa.u_out = (j == 0 && k == 0) ? u : nullptr;
          launch_hess_snap(sa, tc, a->x_idx[j], a->x_idx[k], j, k, nx, fj, fh, c->st);
        }
    } else {
      for (int x0 = 0; x0 < nx; x0 += 3) {
        int seeds[3] = {0, 0, 0};
        const int ns = nx - x0 < 3 ? nx - x0 : 3;
        for (int d = 0; d < ns; ++d) seeds[d] = a->x_idx[x0 + d];
        sa.u_out = x0 == 0 ? u : nullptr;
        launch_jac_snap(sa, tc, ns, seeds, nx, x0, fj, c->st);
      }
    }
  }
  if (hess) launch_hess_gather(c->d_b, c->d_c, n, so, nx, I, a->dudx, a->d2udx2, c->st);
  else launch_jac_gather(c->d_b, n, so, nx, I, a->dudx, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_snapshot_derivatives_dev(const nif_snapderiv_args* a) {
  SnapGeom g; HessIdx I;
  int rc = sd_check(a, &g, &I); if (rc) return rc;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  rc = ensure_packed(c); if (rc) return rc;
  const bool lat_in = a->rows_are_latent != 0, ll = c->kind == NIF_KIND_LASTLAYER;
  if (lat_in) { rc = snap_policy_refusal(c, "nif_snapshot_derivatives", true); if (rc) return rc; }
  if (!ll && !c->jac_ok) return fail(NIF_ERR_INVALID, "HessianLayer: one weight plane and the small hyper-vectors of this shape exceed the 160 KB LDS of a CU");
  const long n = g.n, T = g.T, M = g.M;
  if (n == 0) return NIF_OK;
  const int nx = a->nx, ny = a->ny;
  const bool hess = a->order == 2;
  int32_t xi[16];      // HessianLayer's numbering of the same columns
  for (int j = 0; j < nx; ++j) xi[j] = c->pi + a->x_idx[j];
  // the routes: the point-wise layers on the device-built [p_t | x] table; k_jac_snap on combined nets; the last-layer
  // class' tangents once per shared mesh; else the point-wise kernels behind latent tiles built on the device
  SnapPlan P;
  snap_routes(c, g, lat_in, phi_dot_d2_supported(c->r, c->so, nx, hess), true, &P);
  const long tc_max = P.combined ? snap_chunk(c, T, sp_snapshot_bytes(c, 0)) : 0;
  rc = snap_plan_reserve(c, g, a->x, lat_in, P.pointwise ? c->pi : 0, 0, P.combined ? sp_combined_floats(c, tc_max, 0) : 0, true, &P);
  if (rc) return rc;
  float* d2 = a->d2udx2;
  if (!hess && !P.combined) {      // these routes run the second-order kernels at either order
    rc = c->sd_tmp.reserve(c, (P.phi_dot ? 0 : n * ny * nx * nx) + 1); if (rc) return rc;
    d2 = P.phi_dot ? nullptr : c->sd_tmp.p;
  }
  SnapArgs& sn = P.sn;
  if (P.pointwise) {
    sn.p = a->rows;
    launch_snap_expand(sn, c->st);
    return hessian_core(c, sn.table, n, a->y_idx, ny, xi, nx, a->u, a->dudx, d2);
  }
  const float* lat = a->rows;
  if (!lat_in) { snap_latents_from_p(c, a->rows, T, P.lat); lat = P.lat; }
  if (P.combined) return sd_combined(c, a, P, g, tc_max, lat, I);
  if (P.phi_dot) {      // phi, phi', phi'' of the mesh once, contracted with every snapshot's coefficients
    rc = hessian_core(c, a->x, M, a->y_idx, ny, xi, nx, nullptr, nullptr, nullptr, false, true); if (rc) return rc;
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    launch_phi_dot_d2(c->d_d, c->d_b, hess ? c->d_c.p : nullptr, lat, c->theta + c->ll_bias, T, M, c->r, c->so, nx, I, a->u, a->dudx, d2, c->st);
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  sn.lat = lat; sn.Z = c->Z;
  launch_snap_expand(sn, c->st);
  return hessian_core(c, P.table ? sn.table : a->x, n, a->y_idx, ny, xi, nx, a->u, a->dudx, d2, false);
}
extern "C" int nif_snapshot_derivatives(const nif_snapderiv_args* a) {
  SnapGeom g; HessIdx I;
  int rc = sd_check(a, &g, &I); if (rc) return rc;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  const long n = g.n, n_d = n * a->ny * a->nx;
  SnapSeg s[5] = {{a->rows, nullptr, g.T * (a->rows_are_latent ? c->r : c->pi)}, {a->x, nullptr, (g.off ? n : g.M) * c->si},
                  {nullptr, a->u, n * c->so}, {nullptr, a->dudx, n_d}, {nullptr, a->d2udx2, a->order == 2 ? n_d * a->nx : 0}};
  rc = snap_stage_in(c, s, 5); if (rc) return rc;
  nif_snapderiv_args d = *a;
  d.rows = s[0].dev; d.x = s[1].dev; d.u = s[2].dev; d.dudx = s[3].dev; d.d2udx2 = s[4].dev;
  rc = nif_snapshot_derivatives_dev(&d); if (rc) return rc;
  return snap_stage_out(c, s, 5);
}

// ---- snapshot-wise parameter derivatives (include/nif_hip_snapparam.h) ------------------------------------------------
static int sp_check(const nif_snapparam_args* a, SnapGeom* g, HessIdx* I) {
  int rc = snap_args_check(a, NIF_SNAPPARAM_ABI_VERSION, "nif_snapparam_args"); if (rc) return rc;
  const nif_ctx* c = a->ctx;
  rc = snap_geom_check(c, a->rows, a->T, a->x, a->offsets_host, a->M, a->u && a->dudp, g); if (rc) return rc;
  if (a->rows_are_latent) {
    if (!a->drows) return fail(NIF_ERR_INVALID, "nif_snapshot_param_derivatives: latent rows need drows [T, nd, r]");
    if (a->p_idx || a->np) return fail(NIF_ERR_INVALID, "nif_snapshot_param_derivatives: p_idx / np go with rows [T, pi], not with latents");
    if (a->nd < 1 || a->nd > 16) return fail(NIF_ERR_INVALID, "nif_snapshot_param_derivatives: 1 to 16 directions (nd)");
  } else {
    if (a->drows || a->nd) return fail(NIF_ERR_INVALID, "nif_snapshot_param_derivatives: drows / nd go with latent rows (rows_are_latent = 1)");
    if (!a->p_idx || a->np < 1 || a->np > 16) return fail(NIF_ERR_INVALID, "nif_snapshot_param_derivatives: 1 to 16 parameter columns (p_idx, np)");
    for (int j = 0; j < a->np; ++j) {
      if (a->p_idx[j] < 0 || a->p_idx[j] >= c->pi) return fail(NIF_ERR_INVALID, "p_index out of range (0 <= c < pi_dim)");
      for (int k = 0; k < j; ++k) if (a->p_idx[k] == a->p_idx[j]) return fail(NIF_ERR_INVALID, "p_index: an index is repeated");
    }
  }
  rc = snap_y_index(c, a->y_idx, a->ny, I); if (rc) return rc;
  return snap_not_capturing(c, "nif_snapshot_param_derivatives");
}
constexpr int SP_GROUP = 3;      // direction streams of one launch (the tangent kernels' NIF_JAC_MAXSEED)
// Hypernetwork classes on k_jac_wt.  lat [T][r], D [nd][T][r] (direction-major).  Per chunk of snapshots: w_t and its planes once; per
// group of g <= 3 directions the tangent slot vectors wd_t,d (k_dlatent_to_w), their planes beside W_j's, one launch.  The kernel leaves
// every output row [n][so][nd] in c->d_b; the rows y_idx are gathered behind the last chunk.
static int sp_combined(nif_ctx* c, const nif_snapparam_args* a, const SnapPlan& P, const SnapGeom& g_, long tc_max, int gmax, const float* lat,
                       const float* D, int nd, const HessIdx& I) {
  const long T = g_.T, n = g_.n;
  const int so = c->so, NBL = snet3_nbl(c->n), ps = 1 + gmax;
  int rc = stage(c, c->d_b, nullptr, n * so * nd); if (rc) return rc;
  float* w = P.body;                                // [1 + gmax][tc_max][po]: w_t, then each stream's wd_t
  f32x4* WF = reinterpret_cast<f32x4*>(w + snap_r4((long)ps * tc_max * c->po));
  const long plane_s = sd_plane_f32x4(c);
  for (SnapWalk k{g_, tc_max}; k.next();) {
    const long t0 = k.t0, tc = k.tc;
    snap_pack_f32(c, lat + t0 * c->r, tc, w, WF, ps);
    SNetArgs sa; fill_snet(c, sa, a->x, c->si, 0, k.mmax);
    snap_r0_net(sa, w, P, k, c->nh * ps * plane_s);
    sa.WF = WF; sa.WB = nullptr;
    const long pb = g_.off ? 0 : t0 * g_.M;      // (ragged: the kernel rebases by the call's own offsets; shared mesh: by t M inside the chunk)
    for (int d0 = 0; d0 < nd; d0 += gmax) {
      const int g = nd - d0 < gmax ? nd - d0 : gmax;
      const float* wd[SP_GROUP] = {nullptr, nullptr, nullptr};
      {
        ProfScope p_(c, NIF_PROF_PACK);
        for (int d = 0; d < g; ++d) {
          float* wdd = w + (long)(1 + d) * tc_max * c->po;
          launch_dlatent_to_w(c->theta, c->last_w, c->r, c->po, D + ((long)(d0 + d) * T + t0) * c->r, tc, wdd, c->st);
          for (int j = 0; j < c->nh; ++j)
            launch_pack16_fwd_batch(wdd, dense_ref(hyper_wslot(c, 1 + j), c->n, c->n), c->po, (int)tc, NBL,
                                    WF + ((long)j * ps + 1 + d) * plane_s, c->nh * ps * plane_s, c->st);
          wd[d] = wdd;
        }
      }
      sa.u_out = d0 == 0 ? a->u + pb * so : nullptr;
      ProfScope p_(c, NIF_PROF_SNET_FWD);
      launch_jac_wt(sa, tc, g, wd, ps, nd, d0, c->d_b + pb * so * nd, c->st);
    }
  }
  launch_jac_gather(c->d_b, n, so, nd, I, a->dudp, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_snapshot_param_derivatives_dev(const nif_snapparam_args* a) {
  SnapGeom g; HessIdx I;
  int rc = sp_check(a, &g, &I); if (rc) return rc;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  rc = ensure_packed(c); if (rc) return rc;
  const bool lat_in = a->rows_are_latent != 0, ll = c->kind == NIF_KIND_LASTLAYER;
  if (lat_in) { rc = snap_policy_refusal(c, "nif_snapshot_param_derivatives", true); if (rc) return rc; }
  const int nd = lat_in ? a->nd : a->np, si = c->si, r = c->r, so = c->so;
  // the routes: JacobianLayer's kernels on the table; k_jac_wt on combined nets; the last-layer class' phi once per shared
  // mesh; else the point-wise kernels behind latent and direction tiles built on the device
  SnapPlan P;
  snap_routes(c, g, lat_in, phi_dot_supported(r, so), true, &P);
  const bool pointwise = P.pointwise, combined = P.combined, phi_dot = P.phi_dot, table = P.table;
  if (pointwise) { const int rcw = wide_refused(c, "JacobianLayer"); if (rcw) return rcw; }
  if (!ll && !c->jac_ok) return fail(NIF_ERR_INVALID, "JacobianLayer: one weight plane and the small hyper-vectors of this shape exceed the 160 KB LDS of a CU");
  if (combined) {
    SNetArgs probe; fill_snet(c, probe, nullptr, 0, 0, 32);
    if (!jac_wt_supported(probe))
      return fail(NIF_ERR_INVALID, "nif_snapshot_param_derivatives: one weight plane and four images of the small hyper-vectors of this shape exceed the 160 KB LDS of a CU");
  }
  const long n = g.n, T = g.T, M = g.M;
  if (n == 0) return NIF_OK;
  const int gmax = nd < SP_GROUP ? nd : SP_GROUP;
  const long tc_max = combined ? snap_chunk(c, T, sp_snapshot_bytes(c, gmax)) : 0;
  // the extra head floats: [direction rows [nd][T][r] | so zeros].  The point workspaces are sized behind the point-wise return
  // (jacobian_core sizes its own)
  const long dir_f = pointwise ? 0 : (long)nd * T * r;
  rc = snap_plan_reserve(c, g, a->x, lat_in, pointwise ? c->pi : 0, dir_f + so, combined ? sp_combined_floats(c, tc_max, gmax) : 0, false, &P);
  if (rc) return rc;
  SnapArgs& sn = P.sn;
  if (pointwise) {
    sn.p = a->rows;
    launch_snap_expand(sn, c->st);
    rc = jacobian_core(c, sn.table, n, a->p_idx, nd); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(a->u, c->d_d, sizeof(float) * (size_t)(n * so), hipMemcpyDeviceToDevice, c->st));
    launch_jac_gather(c->d_b, n, so, nd, I, a->dudp, c->st);
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  // ---- the latent and the directions of every snapshot: lat [T][r], D [nd][T][r] ------------------------------------------------------
  const long ttiles = (T + 31) / 32;
  rc = snap_point_capacity(c, g, P); if (rc) return rc;
  const float* lat = a->rows;
  float* D = P.extra;
  float* zero = D + dir_f;
  if (lat_in) launch_dir_rows(a->drows, T, nd, r, D, c->st);
  else {      // per column the ParameterNet's input tangent over the T rows (k_mlp_jac, as nif_jacobian runs it) back as rows, then the latents
    rc = ensure_packed_p32(c); if (rc) return rc;
    rc = c->d_c.reserve(c, ttiles * 32 * r); if (rc) return rc;
    PNetArgs pa; fill_pnet(c, pa, a->rows, T); pa.ncol = c->pi;
    for (int j = 0; j < nd; ++j) {
      PNetArgs pj = pa; pj.Z = ll ? c->DA : c->DZ;      // (primal again into a scratch)
      launch_mlp_jac(pj, c->NSTB, a->p_idx[j], c->d_c, c->st);
      launch_tiles_to_rows(c->d_c, T, r, D + (long)j * T * r, c->st);
    }
    snap_latents_from_p(c, a->rows, T, P.lat);
    lat = P.lat;
  }
  if (combined) return sp_combined(c, a, P, g, tc_max, gmax, lat, D, nd, I);
  if (phi_dot) {      // phi of the mesh once; u, and the same contraction over the nd T tangent coefficient rows without the bias
    HIPCHK(hipMemsetAsync(zero, 0, sizeof(float) * (size_t)so, c->st));
    rc = stage(c, c->d_b, nullptr, n * so * nd); if (rc) return rc;
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    ll_phi_pass(c, a->x, si, 0, M);
    launch_phi_dot(c->PHI, lat, c->theta + c->ll_bias, T, M, r, so, a->u, c->st);
    launch_phi_dot(c->PHI, D, zero, (long)nd * T, M, r, so, c->d_b, c->st);
    launch_snapparam_gather(c->d_b, T, M, so, nd, I, a->dudp, c->st);
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  // ---- point-wise kernels behind tiles: the latent of every point in c->Z, direction d's in a tile array of the same layout -----------
  const long ntl = (n + 31) / 32, zd_sz = ntl * 32 * r;
  rc = stage(c, c->d_b, nullptr, n * so * nd); if (rc) return rc;
  rc = c->d_c.reserve(c, (ll ? 1 : SP_GROUP) * zd_sz); if (rc) return rc;
  sn.lat = lat; sn.Z = c->Z;
  launch_snap_expand(sn, c->st);
  const float* xg = table ? sn.table : a->x;
  sn.table = nullptr;
  if (ll) {
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    ll_phi_pass(c, xg, si, 0, n);
    LLArgs la; fill_ll(c, la, n); la.u_out = a->u;
    launch_ll_out(la, false, c->st);
    for (int d = 0; d < nd; ++d) {
      sn.lat = D + (long)d * T * r; sn.Z = c->d_c;
      launch_snap_expand(sn, c->st);
      launch_ll_jac_out(c->PHI, c->Z, nullptr, c->d_c, n, r, so, nd, d, c->d_b, c->st);
    }
  } else {      // latents on a legacy float32 shape: the point-wise k_jac, its ZD operand exactly such a tile array
    rc = ensure_packed32(c); if (rc) return rc;
    SNetArgs sa; fill_snet(c, sa, xg, si, 0, n);
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    for (int d0 = 0; d0 < nd; d0 += SP_GROUP) {
      const int ns = nd - d0 < SP_GROUP ? nd - d0 : SP_GROUP;
      int seeds[SP_GROUP] = {-1, -1, -1};
      const float* zd[SP_GROUP] = {nullptr, nullptr, nullptr};
      for (int d = 0; d < ns; ++d) {
        sn.lat = D + (long)(d0 + d) * T * r; sn.Z = c->d_c + d * zd_sz;
        launch_snap_expand(sn, c->st);
        zd[d] = sn.Z;
      }
      sa.u_out = d0 == 0 ? a->u : nullptr;
      launch_jac(sa, ns, seeds, zd, nd, d0, c->d_b, c->st);
    }
  }
  launch_jac_gather(c->d_b, n, so, nd, I, a->dudp, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_snapshot_param_derivatives(const nif_snapparam_args* a) {
  SnapGeom g; HessIdx I;
  int rc = sp_check(a, &g, &I); if (rc) return rc;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  const bool lat_in = a->rows_are_latent != 0;
  const long n = g.n, nd = lat_in ? a->nd : a->np;
  SnapSeg s[5] = {{a->rows, nullptr, g.T * (lat_in ? c->r : c->pi)}, {a->drows, nullptr, lat_in ? g.T * nd * c->r : 0},
                  {a->x, nullptr, (g.off ? n : g.M) * c->si}, {nullptr, a->u, n * c->so}, {nullptr, a->dudp, n * a->ny * nd}};
  rc = snap_stage_in(c, s, 5); if (rc) return rc;
  nif_snapparam_args d = *a;
  d.rows = s[0].dev; d.drows = lat_in ? s[1].dev : nullptr; d.x = s[2].dev; d.u = s[3].dev; d.dudp = s[4].dev;
  rc = nif_snapshot_param_derivatives_dev(&d); if (rc) return rc;
  return snap_stage_out(c, s, 5);
}

// ---- second order of the snapshot-wise parameter derivatives (include/nif_hip_snapparam2.h) ----------------------------
static int sp2_check(const nif_snapparam2_args* a, SnapGeom* g, HessIdx* I) {
  const char* who = "nif_snapshot_param_second_derivatives";
  int rc = snap_args_check(a, NIF_SNAPPARAM2_ABI_VERSION, "nif_snapparam2_args"); if (rc) return rc;
  const nif_ctx* c = a->ctx;
  if (a->nxc < 0) return fail(NIF_ERR_INVALID, std::string(who) + ": nxc < 0");
  const bool xc = a->nxc > 0;
  rc = snap_geom_check(c, a->rows, a->T, a->x, a->offsets_host, a->M, a->u && a->dudp && a->d2udp2 && (!xc || (a->dudx && a->d2udpdx)), g);
  if (rc) return rc;
  if (a->rows_are_latent) {
    if (!a->drows) return fail(NIF_ERR_INVALID, std::string(who) + ": latent rows need drows [T, nd, r]");
    if (a->p_idx || a->np) return fail(NIF_ERR_INVALID, std::string(who) + ": p_idx / np go with rows [T, pi], not with latents");
    if (a->nd < 1 || a->nd > 8) return fail(NIF_ERR_INVALID, std::string(who) + ": 1 to 8 directions (nd)");
  } else {
    if (a->drows || a->ddrows || a->nd) return fail(NIF_ERR_INVALID, std::string(who) + ": drows / ddrows / nd go with latent rows (rows_are_latent = 1)");
    if (!a->p_idx || a->np < 1 || a->np > 8) return fail(NIF_ERR_INVALID, std::string(who) + ": 1 to 8 parameter columns (p_idx, np)");
    for (int j = 0; j < a->np; ++j) {
      if (a->p_idx[j] < 0 || a->p_idx[j] >= c->pi) return fail(NIF_ERR_INVALID, "p_index out of range (0 <= c < pi_dim)");
      for (int k = 0; k < j; ++k) if (a->p_idx[k] == a->p_idx[j]) return fail(NIF_ERR_INVALID, "p_index: an index is repeated");
    }
  }
  if (xc != (a->x_idx != nullptr)) return fail(NIF_ERR_INVALID, std::string(who) + ": x_idx and nxc go together");
  if (!xc && (a->dudx || a->d2udpdx)) return fail(NIF_ERR_INVALID, std::string(who) + ": dudx / d2udpdx are null exactly when nxc is 0");
  if (a->nxc > c->si) return fail(NIF_ERR_INVALID, std::string(who) + ": more coordinate columns than coordinates (nxc <= si_dim)");
  if (a->nxc > 16) return fail(NIF_ERR_INVALID, "HessianLayer: at most 16 coordinate and 16 parameter columns in x_index");
  for (int j = 0; j < a->nxc; ++j) {
    if (a->x_idx[j] < 0 || a->x_idx[j] >= c->si) return fail(NIF_ERR_INVALID, "x_index out of range (0 <= j < si_dim: coordinates only)");
    for (int k = 0; k < j; ++k) if (a->x_idx[k] == a->x_idx[j]) return fail(NIF_ERR_INVALID, "x_index: an index is repeated");
  }
  rc = snap_y_index(c, a->y_idx, a->ny, I); if (rc) return rc;
  if (xc) { const int rcw = wide_refused(c, "nif_snapshot_derivatives"); if (rcw) return rcw; }      // (phi' of a wide ShapeNet is not built)
  return snap_not_capturing(c, who);
}
// Hypernetwork classes on k_jac_wt2.  lat [T][r], D [nd][T][r], DD [nd nd][T][r] (pair (a, b), a <= b, at a nd + b; null: no second
// directions).  Per chunk of snapshots: w_t, every direction's tangent slot vector and their planes ONCE ([W_j | W'_0,j .. W'_nd-1,j |
// W''_j] per hidden layer); per pair a <= b its second slot vector wdd = DD_ab . Wh (k_dlatent_to_w: never a difference of combined
// vectors) into the one W'' slot, then one launch that is told its planes' places; per (direction, coordinate) one launch of the mixed
// form.  The kernel leaves every output row [n][so][nd nd] in c->d_c and [n][so][nd nxc] in c->d_b; the rows y_idx are gathered behind
// the last chunk.
static int sp2_combined(nif_ctx* c, const nif_snapparam2_args* a, const SnapPlan& P, const SnapGeom& g_, long tc_max, const float* lat,
                        const float* D, const float* DD, int nd, const HessIdx& I) {
  const long T = g_.T, n = g_.n;
  const int so = c->so, NBL = snet3_nbl(c->n), ps = 2 + nd, nxc = a->nxc;
  int rc = stage(c, c->d_c, nullptr, n * so * nd * nd); if (rc) return rc;
  if (nxc) { rc = stage(c, c->d_b, nullptr, n * so * nd * nxc); if (rc) return rc; }
  float* w = P.body;                                // [2 + nd][tc_max][po]: w_t, each direction's wd_t, the pair's wdd_t
  f32x4* WF = reinterpret_cast<f32x4*>(w + snap_r4((long)ps * tc_max * c->po));
  const long plane_s = sd_plane_f32x4(c);
  auto slot = [&](int i) { return w + (long)i * tc_max * c->po; };
  auto pack = [&](const float* dir, long tc, int i) {      // slot vector i of the chunk from its direction rows, and its planes
    launch_dlatent_to_w(c->theta, c->last_w, c->r, c->po, dir, tc, slot(i), c->st);
    for (int j = 0; j < c->nh; ++j)
      launch_pack16_fwd_batch(slot(i), dense_ref(hyper_wslot(c, 1 + j), c->n, c->n), c->po, (int)tc, NBL, WF + ((long)j * ps + i) * plane_s,
                              c->nh * ps * plane_s, c->st);
  };
  for (SnapWalk k{g_, tc_max}; k.next();) {
    const long t0 = k.t0, tc = k.tc;
    snap_pack_f32(c, lat + t0 * c->r, tc, w, WF, ps);
    {
      ProfScope p_(c, NIF_PROF_PACK);
      for (int d = 0; d < nd; ++d) pack(D + ((long)d * T + t0) * c->r, tc, 1 + d);
    }
    SNetArgs sa; fill_snet(c, sa, a->x, c->si, 0, k.mmax);
    snap_r0_net(sa, w, P, k, c->nh * ps * plane_s);
    sa.WF = WF; sa.WB = nullptr; sa.u_out = nullptr;
    const long pb = g_.off ? 0 : t0 * g_.M;      // (ragged: the kernel rebases by the call's own offsets; shared mesh: by t M inside the chunk)
    for (int i = 0; i < nd; ++i)
      for (int j = i; j < nd; ++j) {
        if (DD) { ProfScope p_(c, NIF_PROF_PACK); pack(DD + ((long)(i * nd + j) * T + t0) * c->r, tc, 1 + nd); }
        ProfScope p_(c, NIF_PROF_SNET_FWD);
        launch_jac_wt2(sa, tc, i == j ? 1 : 0, slot(1 + i), slot(1 + j), DD ? slot(1 + nd) : nullptr, 1 + i, 1 + j, 1 + nd, ps, 0, nd * nd,
                       i * nd + j, j * nd + i, c->d_c + pb * so * nd * nd, c->st);
      }
    for (int i = 0; i < nd; ++i)
      for (int j = 0; j < nxc; ++j) {
        ProfScope p_(c, NIF_PROF_SNET_FWD);
        launch_jac_wt2(sa, tc, 2, slot(1 + i), nullptr, nullptr, 1 + i, 0, 0, ps, a->x_idx[j], nd * nxc, i * nxc + j, i * nxc + j,
                       c->d_b + pb * so * nd * nxc, c->st);
      }
  }
  launch_jac_gather(c->d_c, n, so, nd * nd, I, a->d2udp2, c->st);
  if (nxc) launch_jac_gather(c->d_b, n, so, nd * nxc, I, a->d2udpdx, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
// Last-layer class, u = phi(x) . a + bias with the latent a: d2u/dp_a dp_b = phi . a''_ab and d2u/dp_a dx_j = phi'_j . a'_a.  lat [T][r],
// D [nd][T][r] the tangent coefficient rows, DDc [pairs][T][r] the second ones (pair (a, b), a <= b, in that order; null: none), zero:
// so zeros.  Shared mesh (P.phi_dot): phi once per call and phi'_j once per coordinate (k_mlp_jac over the mesh), each contracted with
// every row by k_phi_dot.  Else: the point-wise epilogue behind coefficient tiles (k_snap_expand), as the first order runs it.
static int sp2_lastlayer(nif_ctx* c, const nif_snapparam2_args* a, SnapPlan& P, const SnapGeom& g, const float* lat, const float* D,
                         const float* DDc, const float* zero, int nd, const HessIdx& I) {
  const long n = g.n, T = g.T, M = g.M;
  const int r = c->r, so = c->so, si = c->si, nxc = a->nxc, npair = nd * (nd + 1) / 2;
  Sp2Map mp, mx;
  memset(&mp, 0, sizeof(mp)); memset(&mx, 0, sizeof(mx));
  mp.n = nd * nd; mx.n = nd * nxc;
  for (int i = 0, q = 0; i < nd; ++i)
    for (int j = i; j < nd; ++j, ++q) { mp.src[i * nd + j] = q; mp.src[j * nd + i] = q; }
  int rc = c->sd_tmp.reserve(c, n * so * (npair + (long)nd * nxc) + 1); if (rc) return rc;
  float* fa = c->sd_tmp.p;                 // the pairs' rows over every output
  float* fx = fa + n * so * npair;         // the mixed rows
  if (!DDc) HIPCHK(hipMemsetAsync(a->d2udp2, 0, sizeof(float) * (size_t)(n * a->ny * nd * nd), c->st));
  if (nxc) ensure_ll_mlp_planes(c);
  ProfScope p_(c, NIF_PROF_SNET_FWD);
  if (P.phi_dot) {
    rc = c->d_c.reserve(c, ((M + 31) / 32) * 32 * (long)r * so); if (rc) return rc;
    ll_phi_pass(c, a->x, si, 0, M);
    if (DDc) {
      launch_phi_dot(c->PHI, DDc, zero, (long)npair * T, M, r, so, fa, c->st);
      launch_snapparam2_gather(fa, n, n * so, so, 1, I, mp, a->d2udp2, c->st);
    }
    for (int j = 0; j < nxc; ++j) {      // phi'_j of the mesh in phi's tile layout, contracted with every tangent row
      PNetArgs mj; fill_snet_mlp(c, mj, a->x, si, 0, M); mj.Z = c->DPHI;
      launch_mlp_jac(mj, c->NB, a->x_idx[j], c->d_c, c->st);
      launch_phi_dot(c->d_c, D, zero, (long)nd * T, M, r, so, fx + (long)j * nd * n * so, c->st);
      for (int i = 0; i < nd; ++i) mx.src[i * nxc + j] = j * nd + i;
    }
    if (nxc) launch_snapparam2_gather(fx, n, n * so, so, 1, I, mx, a->d2udpdx, c->st);
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  const long zd_sz = ((n + 31) / 32) * 32 * r;
  rc = c->d_c.reserve(c, zd_sz * (1 + (nxc ? so : 0))); if (rc) return rc;
  float* zt = c->d_c;                      // one coefficient row of every snapshot as tiles
  float* dphi = c->d_c + zd_sz;            // phi'_j of every point
  SnapArgs& sn = P.sn;
  sn.lat = lat; sn.Z = c->Z;
  launch_snap_expand(sn, c->st);
  const float* xg = P.table ? sn.table : a->x;
  sn.table = nullptr;
  ll_phi_pass(c, xg, si, 0, n);
  if (DDc) {
    for (int q = 0; q < npair; ++q) {
      sn.lat = DDc + (long)q * T * r; sn.Z = zt;
      launch_snap_expand(sn, c->st);
      launch_ll_jac_out(c->PHI, c->Z, nullptr, zt, n, r, so, npair, q, fa, c->st);
    }
    launch_snapparam2_gather(fa, n, 1, (long)so * npair, npair, I, mp, a->d2udp2, c->st);
  }
  for (int j = 0; j < nxc; ++j) {
    PNetArgs mj; fill_snet_mlp(c, mj, xg, si, 0, n); mj.Z = c->DPHI;
    launch_mlp_jac(mj, c->NB, a->x_idx[j], dphi, c->st);
    for (int i = 0; i < nd; ++i) {
      sn.lat = D + (long)i * T * r; sn.Z = zt;
      launch_snap_expand(sn, c->st);
      launch_ll_jac_out(c->PHI, zt, dphi, nullptr, n, r, so, nd * nxc, i * nxc + j, fx, c->st);
    }
  }
  if (nxc) launch_jac_gather(fx, n, so, nd * nxc, I, a->d2udpdx, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_snapshot_param_second_derivatives_dev(const nif_snapparam2_args* a) {
  SnapGeom g; HessIdx I;
  int rc = sp2_check(a, &g, &I); if (rc) return rc;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  const char* who = "nif_snapshot_param_second_derivatives";
  rc = ensure_packed(c); if (rc) return rc;
  const bool lat_in = a->rows_are_latent != 0, ll = c->kind == NIF_KIND_LASTLAYER;
  if (lat_in) { rc = snap_policy_refusal(c, who, true); if (rc) return rc; }
  const int nd = lat_in ? a->nd : a->np, r = c->r, so = c->so, ny = a->ny, nxc = a->nxc;
  // the routes: k_jac_wt2 on combined nets; the last-layer class' phi and phi' against the coefficient rows; else, from
  // p, HessianLayer's kernels on the device-built table
  SnapPlan P;
  snap_routes(c, g, lat_in, phi_dot_supported(r, so), true, &P);
  bool combined = P.combined && c->jac_ok;
  if (combined) { SNetArgs probe; fill_snet(c, probe, nullptr, 0, 0, 32); combined = jac_wt_supported(probe); }
  const bool lastlayer = ll && !snap_pointwise(c);
  if (!combined && !lastlayer && lat_in)
    return fail(NIF_ERR_INVALID, std::string(who) + (P.combined
        ? ": one weight plane and four images of the small hyper-vectors of this shape exceed the 160 KB LDS of a CU"
        : ": latents are not built for this shape (its nets run the legacy kernels; pass p)"));
  if (!combined && !lastlayer) { const int rcw = wide_refused(c, "HessianLayer"); if (rcw) return rcw; }
  PNetArgs pa; fill_pnet(c, pa, a->rows, g.T); pa.ncol = c->pi;
  if (!lat_in && !pjac_supported(pa)) return fail(NIF_ERR_INVALID, "HessianLayer on parameter columns: ParameterNets of up to 128 units");
  const long n = g.n, T = g.T;
  if (n == 0) return NIF_OK;
  // u, dudx and dudp as the first-order calls give them, bit for bit: their own routes, ahead of the second order on the stream
  if (nxc) {
    nif_snapderiv_args d; memset(&d, 0, sizeof(d));
    d.abi_version = NIF_SNAPDERIV_ABI_VERSION; d.order = 1; d.ctx = c; d.rows = a->rows; d.rows_are_latent = a->rows_are_latent; d.T = a->T;
    d.x = a->x; d.offsets_host = a->offsets_host; d.M = a->M; d.y_idx = a->y_idx; d.ny = ny; d.x_idx = a->x_idx; d.nx = nxc;
    d.u = a->u; d.dudx = a->dudx;
    rc = nif_snapshot_derivatives_dev(&d); if (rc) return rc;
  }
  {
    nif_snapparam_args d; memset(&d, 0, sizeof(d));
    d.abi_version = NIF_SNAPPARAM_ABI_VERSION; d.rows_are_latent = a->rows_are_latent; d.ctx = c; d.rows = a->rows; d.drows = a->drows;
    d.nd = a->nd; d.np = a->np; d.p_idx = a->p_idx; d.T = a->T; d.x = a->x; d.offsets_host = a->offsets_host; d.M = a->M;
    d.y_idx = a->y_idx; d.ny = ny; d.u = a->u; d.dudp = a->dudp;
    rc = nif_snapshot_param_derivatives_dev(&d); if (rc) return rc;
  }
  if (lastlayer) {
    // ---- the coefficient rows of every snapshot: lat [T][r], a' = D [nd][T][r], a'' = DDc [pairs][T][r] ------------------------------
    const int npair = nd * (nd + 1) / 2;
    const long ttiles = (T + 31) / 32, blk = ttiles * 32 * r;
    const long dir_f = (long)nd * T * r, ddc_f = (long)npair * T * r, ddf_f = (lat_in && a->ddrows) ? (long)nd * nd * T * r : 0;
    rc = snap_plan_reserve(c, g, a->x, lat_in, 0, dir_f + ddc_f + ddf_f + so, 0, false, &P); if (rc) return rc;
    rc = snap_point_capacity(c, g, P); if (rc) return rc;
    const float* lat = a->rows;
    float* D = P.extra;
    float* DDc = D + dir_f;
    float* DDf = DDc + ddc_f;
    float* zero = DDf + ddf_f;
    HIPCHK(hipMemsetAsync(zero, 0, sizeof(float) * (size_t)so, c->st));
    if (lat_in) {
      launch_dir_rows(a->drows, T, nd, r, D, c->st);
      if (a->ddrows) {
        launch_dir_rows(a->ddrows, T, nd * nd, r, DDf, c->st);
        for (int i = 0, q = 0; i < nd; ++i)
          for (int j = i; j < nd; ++j, ++q)
            HIPCHK(hipMemcpyAsync(DDc + (long)q * T * r, DDf + (long)(i * nd + j) * T * r, sizeof(float) * (size_t)(T * r), hipMemcpyDeviceToDevice, c->st));
      } else DDc = nullptr;
    } else {      // a' per column as the first-order call forms it (k_mlp_jac); a'' = z'' last_w per pair (k_pjac2, ONE k_through_lw)
      rc = ensure_packed_p32(c); if (rc) return rc;
      rc = c->d_c.reserve(c, blk); if (rc) return rc;
      rc = c->jac_mu.reserve(c, 2 * npair * blk + 2L * npair + 2); if (rc) return rc;      // [z'' | a'' | npair source offsets (longs)]
      for (int j = 0; j < nd; ++j) {
        PNetArgs pj = pa; pj.Z = c->DA;      // (primal again into a scratch)
        launch_mlp_jac(pj, c->NSTB, a->p_idx[j], c->d_c, c->st);
        launch_tiles_to_rows(c->d_c, T, r, D + (long)j * T * r, c->st);
      }
      float* zs = c->jac_mu;
      float* ap = zs + (long)npair * blk;
      for (int i = 0, q = 0; i < nd; ++i)
        for (int j = i; j < nd; ++j, ++q) launch_pjac2(pa, a->p_idx[i], a->p_idx[j], zs + (long)q * blk, c->st);
      long* off_dev = reinterpret_cast<long*>(ap + (long)npair * blk);
      launch_stride_offsets(off_dev, npair, blk, c->st);      // vector q sits q blk floats behind zs (on the device: the entry stays asynchronous)
      launch_through_lw(zs, off_dev, npair, c->theta + c->last_w, r, ttiles * 32, ap, c->st);
      for (int q = 0; q < npair; ++q) launch_tiles_to_rows(ap + (long)q * blk, T, r, DDc + (long)q * T * r, c->st);
      snap_latents_from_p(c, a->rows, T, P.lat);
      lat = P.lat;
    }
    return sp2_lastlayer(c, a, P, g, lat, D, DDc, zero, nd, I);
  }
  if (!combined) {      // HessianLayer on the table over [p_idx | pi + x_idx]; its parameter rows of the Hessian are the two blocks
    P.pointwise = true; P.combined = false; P.phi_dot = false; P.table = true;
    const int nx = nd + nxc;
    const long n_j = n * ny * nx;
    rc = snap_plan_reserve(c, g, a->x, false, c->pi, 0, 0, true, &P); if (rc) return rc;
    rc = c->sd_tmp.reserve(c, n * so + n_j + n_j * nx + 1); if (rc) return rc;
    int32_t cols[24];
    for (int j = 0; j < nd; ++j) cols[j] = a->p_idx[j];
    for (int j = 0; j < nxc; ++j) cols[nd + j] = c->pi + a->x_idx[j];
    P.sn.p = a->rows;
    launch_snap_expand(P.sn, c->st);
    float* H = c->sd_tmp.p + n * so + n_j;
    rc = hessian_core(c, P.sn.table, n, a->y_idx, ny, cols, nx, c->sd_tmp.p, c->sd_tmp.p + n * so, H); if (rc) return rc;
    launch_snapparam2_blocks(H, n * ny, nd, nxc, a->d2udp2, a->d2udpdx, c->st);
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  // ---- the latent, the directions and the second directions of every snapshot: lat [T][r], D [nd][T][r], DD [nd nd][T][r] -------------
  const long tc_max = snap_chunk(c, T, sp_snapshot_bytes(c, 1 + nd));
  const long dir_f = (long)nd * T * r, dd_f = (long)nd * nd * T * r;
  rc = snap_plan_reserve(c, g, a->x, lat_in, 0, dir_f + dd_f, sp_combined_floats(c, tc_max, 1 + nd), false, &P); if (rc) return rc;
  rc = snap_point_capacity(c, g, P); if (rc) return rc;
  const float* lat = a->rows;
  float* D = P.extra;
  float* DD = D + dir_f;
  if (lat_in) {
    launch_dir_rows(a->drows, T, nd, r, D, c->st);
    if (a->ddrows) launch_dir_rows(a->ddrows, T, nd * nd, r, DD, c->st);
    else DD = nullptr;
  } else {      // dz/dp per column as the first-order call forms it (k_mlp_jac), d2z/dp_a dp_b per pair (k_pjac2), over the T rows
    rc = ensure_packed_p32(c); if (rc) return rc;
    rc = c->d_c.reserve(c, ((T + 31) / 32) * 32 * r); if (rc) return rc;
    for (int j = 0; j < nd; ++j) {
      PNetArgs pj = pa; pj.Z = c->DZ;      // (primal again into a scratch)
      launch_mlp_jac(pj, c->NSTB, a->p_idx[j], c->d_c, c->st);
      launch_tiles_to_rows(c->d_c, T, r, D + (long)j * T * r, c->st);
    }
    for (int i = 0; i < nd; ++i)
      for (int j = i; j < nd; ++j) {
        launch_pjac2(pa, a->p_idx[i], a->p_idx[j], c->d_c, c->st);
        launch_tiles_to_rows(c->d_c, T, r, DD + (long)(i * nd + j) * T * r, c->st);
      }
    snap_latents_from_p(c, a->rows, T, P.lat);
    lat = P.lat;
  }
  return sp2_combined(c, a, P, g, tc_max, lat, D, DD, nd, I);
}
extern "C" int nif_snapshot_param_second_derivatives(const nif_snapparam2_args* a) {
  SnapGeom g; HessIdx I;
  int rc = sp2_check(a, &g, &I); if (rc) return rc;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  const bool lat_in = a->rows_are_latent != 0;
  const long n = g.n, nd = lat_in ? a->nd : a->np, n_p = n * a->ny * nd;
  SnapSeg s[9] = {{a->rows, nullptr, g.T * (lat_in ? c->r : c->pi)}, {a->drows, nullptr, lat_in ? g.T * nd * c->r : 0},
                  {a->ddrows, nullptr, (lat_in && a->ddrows) ? g.T * nd * nd * c->r : 0}, {a->x, nullptr, (g.off ? n : g.M) * c->si},
                  {nullptr, a->u, n * c->so}, {nullptr, a->dudp, n_p}, {nullptr, a->d2udp2, n_p * nd},
                  {nullptr, a->dudx, n * a->ny * a->nxc}, {nullptr, a->d2udpdx, n_p * a->nxc}};
  rc = snap_stage_in(c, s, 9); if (rc) return rc;
  nif_snapparam2_args d = *a;
  d.rows = s[0].dev; d.drows = lat_in ? s[1].dev : nullptr; d.ddrows = (lat_in && a->ddrows) ? s[2].dev : nullptr; d.x = s[3].dev;
  d.u = s[4].dev; d.dudp = s[5].dev; d.d2udp2 = s[6].dev;
  d.dudx = a->nxc ? s[7].dev : nullptr; d.d2udpdx = a->nxc ? s[8].dev : nullptr;
  rc = nif_snapshot_param_second_derivatives_dev(&d); if (rc) return rc;
  return snap_stage_out(c, s, 9);
}

extern "C" int nif_pnet_latent(nif_ctx* c, const float* p, int64_t B, float* lr) {
  if (!c || !p || !lr || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  int rc = ensure_packed(c); if (rc) return rc;
  rc = ensure_capacity(c, B, false); if (rc) return rc;
  rc = stage(c, c->d_a, p, B * c->pi); if (rc) return rc;
  rc = stage(c, c->d_d, nullptr, B * c->r); if (rc) return rc;
  PNetArgs pa; fill_pnet(c, pa, c->d_a, B);
  pa.ncol = c->pi;
  launch_pnet(pa, c->NSTB, false, c->st);
  launch_tiles_to_rows(c->Z, B, c->r, c->d_d, c->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(lr, c->d_d, sizeof(float) * (size_t)(B * c->r), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

extern "C" int nif_x_to_phi(nif_ctx* c, const float* x, int64_t B, float* phi) {
  if (!c || !x || !phi || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  if (c->kind != NIF_KIND_LASTLAYER) return fail(NIF_ERR_INVALID, "model_x_to_phi exists only for the last-layer class");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  int rc = ensure_packed(c); if (rc) return rc;
  rc = ensure_capacity(c, B, false); if (rc) return rc;
  rc = stage(c, c->d_a, x, B * c->si); if (rc) return rc;
  rc = stage(c, c->d_d, nullptr, B * c->so * c->r); if (rc) return rc;
  ll_phi_pass(c, c->d_a, c->si, 0, B);
  launch_tiles_to_rows(c->PHI, B, c->so * c->r, c->d_d, c->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(phi, c->d_d, sizeof(float) * (size_t)(B * c->so * c->r), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

extern "C" int nif_latent_to_w_dev(nif_ctx* c, const float* lr, int64_t B, float* w) {
  if (!c || !lr || !w || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  if (!c->have_params) return fail(NIF_ERR_STATE, "parameters not set");
  if (c->kind == NIF_KIND_LASTLAYER)
    return fail(NIF_ERR_INVALID, "In this class: NIFMultiScaleLastLayerParameterization, `w` is the same as `lr`");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  { ProfScope p_(c, NIF_PROF_LATENT_TO_W); launch_latent_to_w(c->theta, c->last_w, c->last_b, c->r, c->po, lr, B, w, c->st); }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_latent_to_w(nif_ctx* c, const float* lr, int64_t B, float* w) {
  if (!c || !lr || !w || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  int rc = stage(c, c->d_a, lr, B * c->r); if (rc) return rc;
  rc = stage(c, c->d_b, nullptr, B * c->po); if (rc) return rc;
  rc = nif_latent_to_w_dev(c, c->d_a, B, c->d_b); if (rc) return rc;
  HIPCHK(hipMemcpyAsync(w, c->d_b, sizeof(float) * (size_t)(B * c->po), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

extern "C" int nif_shapenet_given_w_dev(nif_ctx* c, const float* x, const float* w, int64_t B, float* u) {
  if (!c || !x || !w || !u || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  if (c->kind == NIF_KIND_LASTLAYER) {   // u = Dot(phi(x), w) + bias with caller-supplied w [B, r]
    int rc = ensure_packed(c); if (rc) return rc;
    rc = ensure_capacity(c, B, false); if (rc) return rc;
    ll_phi_pass(c, x, c->si, 0, B);
    launch_rows_to_tiles(w, B, c->r, c->Z, c->st);
    LLArgs la; fill_ll(c, la, B); la.u_out = u;
    launch_ll_out(la, false, c->st);
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  const int act = c->kind == NIF_KIND_NIF ? c->cfg.s_act : NIF_ACT_SINE;
  const float om = c->kind == NIF_KIND_NIF ? 1.0f : c->cfg.s_omega0;
  { ProfScope p_(c, NIF_PROF_GIVEN_W);
    launch_given_w(x, w, u, B, c->si, c->so, c->n, c->nh, c->po, act, c->cfg.s_resblock, c->kind == NIF_KIND_NIF, om, c->st); }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_shapenet_given_w(nif_ctx* c, const float* x, const float* w, int64_t B, float* u) {
  if (!c || !x || !w || !u || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  int rc = stage(c, c->d_a, x, B * c->si); if (rc) return rc;
  rc = stage(c, c->d_b, w, B * c->po); if (rc) return rc;   // po == r for the last-layer class
  rc = stage(c, c->d_d, nullptr, B * c->so); if (rc) return rc;
  rc = nif_shapenet_given_w_dev(c, c->d_a, c->d_b, B, c->d_d); if (rc) return rc;
  HIPCHK(hipMemcpyAsync(u, c->d_d, sizeof(float) * (size_t)(B * c->so), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

// ---- training step: the pieces every class and pass shares -------------------------------------------
static int rows_for(const nif_ctx* c, long ntiles) {
  int rows = (int)((ntiles + 3) / 4);
  if (rows > c->rows_cap()) rows = c->rows_cap();
  return rows < 1 ? 1 : rows;
}
// NIF_PNET_STASH=1 forces the ParameterNet adjoint through its HBM stash (A/B runs, tests); default: small ParameterNets keep no stash,
// the adjoint kernel recomputes the forward pass and reduces the weight gradients itself (k_pnetbw.hip)
static bool pnet_force_stash() {
  static const bool on = [] { const char* e = getenv("NIF_PNET_STASH"); return e && e[0] == '1'; }();
  return on;
}
static int ensure_jac_tmp(nif_ctx* c) { return c->jac_tmp ? NIF_OK : c->jac_tmp.alloc(c->P + 2); }
// block of c->dzt_par that holds dL/dz' of each parameter column (jac_reg_pass, given mu); -1: none
struct MuBlk { int blk[16]; MuBlk() { for (int& b : blk) b = -1; } };
// The SobPar of a plan, as every launch_sob call (query or launch) starts from it; a site adds only what is its own: the last-layer
// class sets par = -1 and its head fields, the hypernetwork classes ZT / DZT
static SobPar sob_par_of(const SobPlan& sp) {
  SobPar q{};
  for (int d = 0; d < 3; ++d) { q.par[d] = sp.par[d]; q.gcol[d] = sp.gcol[d]; }
  q.gstride = sp.gstride; q.nx_all = sp.nx_all; q.ny = sp.ny; q.no_primal = sp.no_primal; q.ymask = sp.ymask; q.hess = sp.hess;
  return q;
}
// z' = dz/dp of every parameter column into c->zt_par (k_pjac, forward mode), in front of the ShapeNet; train: + room for the
// dL/dz' of up to three streams
static int ensure_zt_par(nif_ctx* c, const PNetArgs& pa, long ntiles, bool train) {
  if (!pjac_supported(pa))
    return fail(NIF_ERR_INVALID, "Sobolev x_index on parameter columns: ParameterNets of up to 128 units");
  int rc = c->zt_par.reserve(c, (long)c->pi * ntiles * 32 * c->r); if (rc) return rc;
  if (train) { rc = c->dzt_par.reserve(c, 3 * ntiles * 32 * c->r); if (rc) return rc; }
  launch_pjac_fwd(pa, c->zt_par, c->st);
  return NIF_OK;
}
// Workgroups (= loss partials) of the last-layer class's k_snet4<LL> step, and its act'(a) ring
static int ll4_plan(nif_ctx* c, SNetArgs& sa, int* nloss) {
  *nloss = launch_snet4(sa, true, true, c->st);
  const int rc = c->dring.reserve(c, (long)*nloss * 4 * snet3_ring_floats_per_wave(c->n, c->nh)); if (rc) return rc;
  sa.dring = c->dring;
  return NIF_OK;
}

// Weight-gradient reductions into partial rows.  Every GwArgs of a step starts from gw_base; gw_add_tangents makes the reduction run
// over n blocks of tangent pseudo-tiles behind the real tiles as well (Sobolev streams, the z' tangents of jac_reg_pass).  The two
// stacks below are the one statement of the reduction sequence of the ParameterNet and of the hypernetwork ShapeNet
static GwArgs gw_base(const nif_ctx* c, long ntiles, long B, float* partial) {
  GwArgs q;
  memset(&q, 0, sizeof(q));
  q.ntiles = ntiles; q.B = B; q.partial = partial; q.pstride = c->pstride; q.has_bias = 1; q.scale = 1.0f;
  return q;
}
static void gw_add_tangents(GwArgs& q, int n, const int* seeds) {
  q.zt_mod = q.ntiles; q.bias_ntiles = q.ntiles; q.ntiles *= 1 + n;
  for (int d = 0; d < 3; ++d) q.seed[d] = (seeds && d < n) ? seeds[d] : 0;
}
// ParameterNet: first layer, hidden matrices, bottleneck -- from the stash slots at pST, SM = dL/d(bottleneck output).  ncol: the
// columns of xin's rows (0: the table's pi + si; the snapshot step's rows of p alone: pi)
static void gw_pnet_stack(const nif_ctx* c, const GwArgs& base, const float* xin, const float* pST, const float* SM, float omega, int rows,
                          hipStream_t st, int ncol = 0) {
  GwArgs g = base;
  g.DA = pST + (long)(c->nm + 1) * c->slot_p; g.xin = xin; g.ncol = ncol > 0 ? ncol : c->pi + c->si; g.col0 = 0; g.nd = c->pi; g.scale = omega;
  g.W = dense_ref(c->first_w, c->pi, c->nst); g.Bv = vec_ref(c->first_b, c->nst);
  launch_gw_first(g, c->NSTB, rows, st);
  for (int mi = 0; mi < c->nm; ++mi) {
    g = base; g.IN = pST + (long)mi * c->slot_p; g.DA = pST + (long)(c->nm + 2 + mi) * c->slot_p; g.scale = omega;
    long w_off, b_off; pnet_mat(c, mi, &w_off, &b_off);
    g.W = dense_ref(w_off, c->nst, c->nst); g.Bv = vec_ref(b_off, c->nst);
    launch_gw_mfma(g, c->NSTB, c->NSTB, rows, st);
  }
  g = base; g.IN = pST + (long)c->nm * c->slot_p; g.SM = SM; g.nc = c->r;
  g.W = dense_ref(c->bott_w, c->nst, c->r); g.Bv = vec_ref(c->bott_b, c->r);
  launch_gw_out(g, c->NSTB, rows, st);
}
// Hypernetwork ShapeNet: first layer, hidden matrices, last layer -- the stashes and DU of sa, block blk of their tiles as the dL/da
// side (0: the step's own tiles and pseudo-tiles; 1 + d: stream d alone, sob_par_pass), Z in the latent's place; base carries the
// tangent pseudo-tiles (zt_mod = the real tiles), the first layer runs over first_ntiles of them.  < 0: launch_gw_mfma's refusal
static int gw_hyper_snet_stack(const nif_ctx* c, const GwArgs& base, const SNetArgs& sa, const float* xin, const float* Z, long blk,
                               long first_ntiles, bool da_bf16, bool in_ph16, int rows, hipStream_t st) {
  const float* sIN = sa.stash;
  const float* sDA = sa.stash + (long)(c->nh + 1) * c->slot_s + blk * base.zt_mod * 1024 * c->NB;
  GwArgs g = base;
  g.DA = sDA; g.xin = xin; g.ncol = c->pi + c->si; g.col0 = c->pi; g.nd = c->si; g.Z = Z; g.r = c->r; g.scale = sa.omega;
  g.W = hyper_w(c, 0); g.Bv = hyper_b(c, 0);
  g.ntiles = first_ntiles;
  launch_gw_first(g, c->NB, rows, st);
  for (int j = 0; j < c->nh; ++j) {
    g = base; g.IN = sIN + (long)j * c->slot_s; g.DA = sDA + (long)(j + 1) * c->slot_s; g.Z = Z; g.r = c->r; g.scale = sa.omega;
    g.da_bf16 = da_bf16 ? 1 : 0;
    g.in_ph16 = in_ph16 ? 1 : 0;
    g.W = hyper_w(c, 1 + j); g.Bv = hyper_b(c, 1 + j);
    if (launch_gw_mfma(g, c->NB, c->NB, rows, st) < 0) return -1;
  }
  g = base; g.IN = sIN + (long)c->nh * c->slot_s; g.SM = sa.DU + blk * base.zt_mod * c->so * 32; g.nc = c->so; g.Z = Z; g.r = c->r;
  g.W = hyper_w(c, c->nh + 1); g.Bv = hyper_b(c, c->nh + 1);
  launch_gw_out(g, c->NB, rows, st);
  return 0;
}

// ---- last-layer-parameterised class: loss and gradient ---------------------------------------------
// SNetArgs of the last-layer class for k_sob (Sobolev step / its predict): k_snet4's arguments for that class plus, beyond the
// widths whose bf16 planes fit the LDS (n > 96), the f32-input MFMA planes of the shared hidden matrices, packed on demand
static int fill_snet_ll_sob(nif_ctx* c, SNetArgs& sa, const float* xin, long B, bool f32_planes) {
  if (!c->ll_slots) return fail(NIF_ERR_INVALID, "JacobianLayer-as-output / HessianLayer on the last-layer class: ShapeNet with at least one hidden layer and units <= 128");
  fill_snet_ll(c, sa, xin, c->pi + c->si, c->pi, B);
  if (!sob_ll_supported(sa)) return fail(NIF_ERR_INVALID, "JacobianLayer-as-output / HessianLayer on the last-layer class: so * latent_dim <= 64");
  const int NBL = snet3_nbl(c->n);
  if (!c->use_ll4) { sa.WF4 = nullptr; sa.WB4 = nullptr; f32_planes = true; }   // (bf16-split planes are packed for k_snet4<LL> only)
  if (NBL > 6 || f32_planes) {     // (k_jac / the Hessian take the f32-input planes at every width)
    const long plane_s = plane_f32x4(PLANES_T16, NBL);
    if (!c->ll_packed32) {
      for (int j = 0; j < c->nh; ++j) {
        long w_off, b_off; snet_mat(c, j, &w_off, &b_off);
        launch_pack16(c->theta, dense_ref(w_off, c->n, c->n), NBL, c->sWF + (long)j * plane_s, c->sWB + (long)j * plane_s, c->st);
      }
      c->ll_packed32 = true;
    }
    sa.WF = c->sWF; sa.WB = c->sWB;
    if (NBL > 6) { sa.WF4 = nullptr; sa.WB4 = nullptr; }
  }
  return NIF_OK;
}

static int loss_grad_ll(nif_ctx* c, const float* xin, const float* y, const float* sw, long B, long Bg, int ns = 0,
                        const SobPlan* sp = nullptr, const float* gt = nullptr, float wj = 0.f) {
  const long ntiles = (B + 31) / 32;
  const int ncol = c->pi + c->si;
  const int nsc = ns > 0 ? sp->nsc : 0, nhead = ns > 0 ? sp->ns - sp->nsc : 0;   // coordinate streams / parameter-column heads
  PNetArgs pa; fill_pnet(c, pa, xin, B);
  if (!c->use_wide) ensure_ll_mlp_planes(c);      // (a wide net has no plane image)
  PNetArgs ma; fill_snet_mlp(c, ma, xin, ncol, c->pi, B);
  LLArgs la; fill_ll(c, la, B);
  la.y = y; la.sw = sw; la.inv_bg = 1.0f / (float)Bg;
  const bool fused_p = !pnet_force_stash() && pnet_bwg_supported(pa);
  if (!fused_p) { const int rcp = ensure_packed_p32(c); if (rcp) return rcp; }
  { ProfScope p_(c, NIF_PROF_PNET_FWD); launch_pnet(pa, c->NSTB, !fused_p, c->st); }
  int nloss = (int)((ntiles * 32 + 255) / 256);
  bool ll_dab = false, ll_ph = false;
  if (ns > 0) {   // Sobolev: primal + tangents + their adjoint on k_sob<.., LL>; stashes and DPHI hold (1 + ns) blocks of tiles
    SNetArgs sa; int rc = fill_snet_ll_sob(c, sa, xin, B); if (rc) return rc;
    sa.y = y; sa.sw = sw; sa.loss_partial = c->loss_partial; sa.inv_bg = 1.0f / (float)Bg;
    SobPar spar = sob_par_of(*sp);
    for (int d = 0; d < 3; ++d) spar.par[d] = -1;       // (parameter columns are heads of the epilogue here, not streams)
    nloss = launch_sob(sa, true, nsc, sp->seeds, nullptr, 0.f, nullptr, nullptr, true, c->st, &spar);
    if (nloss < 0) return fail(NIF_ERR_INVALID, "Sobolev step: the kernel's working set of this shape does not fit the 160 KB LDS of a CU");
    const long need = (long)nloss * 4 * sob_ring_floats_per_wave(c->n, c->nh);
    rc = c->dring.reserve(c, need); if (rc) return rc;
    if (nhead > 0) {     // parameter columns: heads of the epilogue (z' = dz/dp sits in c->zt_par, loss_grad_core)
      const long need_a = 3 * ntiles * 32 * c->r, need_l = 3 * ntiles * 32 * 32 * c->RB;
      rc = c->dat_par.reserve(c, need_a); if (rc) return rc;
      if (need_l > c->ztl_par.n) {
        rc = c->ztl_par.reserve(c, need_l); if (rc) return rc;
        HIPCHK(hipMemsetAsync(c->ztl_par, 0, sizeof(float) * (size_t)need_l, c->st));     // the padding rows stay zero
      }
      spar.npar = nhead; spar.ZT = c->zt_par; spar.DZT = c->dzt_par; spar.DAT = c->dat_par; spar.ZTL = c->ztl_par;
      spar.zl_rows = 32 * c->RB;
      for (int e = 0; e < nhead; ++e) { spar.parc[e] = sp->par[nsc + e]; spar.pcol[e] = sp->gcol[nsc + e]; }
    }
    ProfScope p_(c, NIF_PROF_SNET);
    launch_sob(sa, true, nsc, sp->seeds, gt, wj, c->dring, nullptr, false, c->st, &spar);
  } else if (c->use_wide) {      // layer by layer; the adjoint sweep runs next to the weight gradients below
    ProfScope p_(c, NIF_PROF_SNET);
    wide_forward(c, xin, ncol, c->pi, B, true);
    launch_ll_out(la, true, c->st);
  } else if (c->use_ll4) {
    SNetArgs sa; fill_snet_ll(c, sa, xin, ncol, c->pi, B);
    sa.y = y; sa.sw = sw; sa.loss_partial = c->loss_partial; sa.inv_bg = 1.0f / (float)Bg;
    {   // mixed_bfloat16: bf16 dL/da stash rows of the shared hidden layers (step_chunk has the hypernetwork classes' rule)
      const int nbl = snet3_nbl(c->n);
      ll_dab = sa.prec == 1 && (nbl == 2 || nbl == 4 || nbl == 8) && gw_da_bf16_ok(c->NB, c->NB, 0);
      sa.da_bf16 = ll_dab ? 1 : 0;
      if (snet4_writes_da_bf16(sa) != ll_dab) return fail(NIF_ERR_STATE, "internal: dL/da stash format of producer and plan disagree");
      // ... and, on the 128-wide kernel, the hidden matrices' input rows as 16-bit phases (k_gw8<0, true, true> reads them)
      sa.h_ph16 = (ll_dab && nbl == 8 && !c->cfg.s_resblock && gw_in_ph16_ok(c->NB, c->NB, 0)) ? 1 : 0;
      ll_ph = snet4_writes_h_ph16(sa);
      if (ll_ph != (sa.h_ph16 != 0)) return fail(NIF_ERR_STATE, "internal: layer-input stash format of producer and plan disagree");
    }
    int rc = ll4_plan(c, sa, &nloss); if (rc) return rc;
    ProfScope p_(c, NIF_PROF_SNET);
    if (launch_snet4(sa, true, false, c->st) < 0) return fail(NIF_ERR_STATE, "internal: no k_snet4 form for this net (SIREN planes not packed as half pairs)");
  } else {
    ProfScope p_(c, NIF_PROF_SNET);
    launch_pnet(ma, c->NB, true, c->st);
    launch_ll_out(la, true, c->st);
    launch_pnet_bwd(ma, c->NB, c->st);
  }
  int n_act = 0;
  if (act_on(c)) {    // + c/Bg phi'(a) into dL/da and dL/dlatent, before their consumers; the loss term joins after the row reduction
    const long nlp = (B + 255) / 256;
    int rc = c->act_loss.reserve(c, nlp); if (rc) return rc;
    const bool l1 = c->act_l2 == 0.f;
    n_act = launch_ll_actreg(c->Z, c->theta + c->last_w, c->r, B, (l1 ? c->act_l1 : c->act_l2) / (float)Bg, l1, c->DA, c->DZL, c->act_loss, c->st);
  }
  const int rows = rows_for(c, ntiles);
  { ProfScope p_(c, NIF_PROF_PNET_BWD);
    if (fused_p) launch_pnet_bwg(pa, c->partial, c->pstride, rows, c->st);
    else launch_pnet_bwd(pa, c->NSTB, c->st); }
  if (c->use_wide) wide_backward(c, xin, ncol, c->pi, B, rows);      // adjoint sweep + first, hidden, bottleneck gradients (k_wide.hip)
  {
    ProfScope p_(c, NIF_PROF_GW);
    const GwArgs base = gw_base(c, ntiles, B, c->partial);
    GwArgs sbase = base;            // Sobolev: the ShapeNet reductions also run over the tangent pseudo-tiles
    if (nsc > 0) gw_add_tangents(sbase, nsc, sp->seeds);
    const int nms = c->nh;  // hidden matrices of the ShapeNet (2L with resblocks)
    float* sST = c->stash_s;
    // ShapeNet (dense SIREN): first, hidden matrices, bottleneck (n -> r*so), last_layer_bias
    GwArgs g = sbase;
    if (!c->use_wide) {      // (a wide net: wide_backward above)
      g.DA = sST + (long)(nms + 1) * c->slot_s; g.xin = xin; g.ncol = ncol; g.col0 = c->pi; g.nd = c->si; g.scale = ma.omega;
      if (ns > 0 && sp->hess) g.ntiles = ntiles * 3;      // (the second-order stream has no first-layer input: a'' = 0 there)
      g.W = dense_ref(c->s_first_w, c->si, c->n); g.Bv = vec_ref(c->s_first_b, c->n);
      launch_gw_first(g, c->NB, rows, c->st);
      for (int mi = 0; mi < nms; ++mi) {
        g = sbase; g.IN = sST + (long)mi * c->slot_s; g.DA = sST + (long)(nms + 2 + mi) * c->slot_s; g.scale = ma.omega;
        long w_off, b_off; snet_mat(c, mi, &w_off, &b_off);
        g.W = dense_ref(w_off, c->n, c->n); g.Bv = vec_ref(b_off, c->n);
        g.da_bf16 = ll_dab ? 1 : 0;
        g.in_ph16 = ll_ph ? 1 : 0;
        if (launch_gw_mfma(g, c->NB, c->NB, rows, c->st) < 0) return fail(NIF_ERR_STATE, "internal: bf16 dL/da stash rows without a reader of that form");
      }
      g = sbase; g.IN = sST + (long)nms * c->slot_s; g.SM = c->DPHI; g.nc = c->r * c->so;
      g.W = dense_ref(c->s_bott_w, c->n, c->r * c->so); g.Bv = vec_ref(c->s_bott_b, c->r * c->so);
      launch_gw_out(g, c->NB, rows, c->st);
    }
    g = base; g.IN = c->use_wide ? nullptr : sST + (long)nms * c->slot_s; g.SM = c->DU; g.nc = c->so;   // only the bias part: W.nin = 0 (k_gw_bias reads SM alone)
    g.W = dense_ref(0, 0, c->so); g.Bv = vec_ref(c->ll_bias, c->so);
    launch_gw_out(g, c->NB, rows, c->st);
    // ParameterNet: first, hidden matrices, bottleneck, last (r x r)
    if (!fused_p) gw_pnet_stack(c, base, xin, c->stash_p, c->DZL, pa.omega, rows, c->st);
    g = base; g.IN = c->ZL; g.SM = c->DA; g.nc = c->r;   // latent (padded rows) x dL/da
    g.W = dense_ref(c->last_w, c->r, c->r); g.Bv = vec_ref(c->last_b, c->r);
    launch_gw_out(g, c->RB, rows, c->st);
  }
  {
    ProfScope pr_(c, NIF_PROF_REDUCE);
    launch_reduce(c->partial, c->pstride, rows, c->loss_partial, nloss, c->grad, c->P, c->st);
  }
  if (n_act > 0) launch_add_sum(c->act_loss, n_act, c->grad + c->P, c->st);
  if (c->jac_l1 != 0.f) { int rc = jac_reg_pass(c, xin, B, Bg); if (rc) return rc; }
  if (nhead > 0) {
    // the heads' share of the r x r layer: dL/dlast_w += z'^T dL/da' (a' = z' last_w has no bias), the same reduction as the
    // main one with (z', dL/da') as the operand pair; then the (primal, tangent) ParameterNet for dL/dz' (jac_reg_pass, given mu)
    { const int rca = ensure_jac_tmp(c); if (rca) return rca; }
    MuBlk mu;
    const long rr = (long)c->r * c->r;
    for (int e = 0; e < nhead; ++e) {
      mu.blk[sp->par[nsc + e]] = e;
      GwArgs g = gw_base(c, ntiles, B, c->partial);
      g.IN = c->ztl_par + (long)e * ntiles * 32 * 32 * c->RB; g.SM = c->dat_par + (long)e * ntiles * 32 * c->r; g.nc = c->r;
      g.W = dense_ref(c->last_w, c->r, c->r); g.Bv = vec_ref(c->last_b, c->r);     // (the bias columns are not taken over)
      launch_gw_out(g, c->RB, rows, c->st);
      launch_reduce(c->partial + c->last_w, c->pstride, rows, nullptr, 0, c->jac_tmp, rr, c->st);
      launch_axpy_cols(c->grad + c->last_w, c->jac_tmp, rr, c->P - c->last_w, c->st);
    }
    HIPCHK(hipGetLastError());
    return jac_reg_pass(c, xin, B, Bg, mu.blk);
  }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}

// Workspace sizing of the fused ShapeNet kernel the step will launch (no launch): number of workgroups (= loss partials),
// the act'(a) ring, the optional edge-gradient partials.  Grows buffers when needed (stream sync + device allocation): call
// nif_reserve() once up front to keep that out of the timed steps.
static int snet_plan(nif_ctx* c, SNetArgs& sa, int ns, const int* seeds, int* nloss, const SobPlan* sp = nullptr) {
  int rc;
  if (ns > 0) {
    SobPar spq{};     // (the parameter streams' extra per-wave LDS counts; no plan: first-order coordinate streams, as launch_sob takes no SobPar)
    if (sp) spq = sob_par_of(*sp);
    const int nblk = launch_sob(sa, true, ns, seeds, nullptr, 0.f, nullptr, nullptr, true, c->st, sp ? &spq : nullptr);
    if (nblk < 0)
      return fail(NIF_ERR_INVALID, "Sobolev step: the kernel's working set of this shape (units, latent_dim, parameter columns) does not fit the 160 KB LDS of a CU");
    const long need = (long)nblk * 4 * sob_ring_floats_per_wave(c->n, c->nh);
    rc = c->dring.reserve(c, need); if (rc) return rc;
    *nloss = nblk;
  } else if (c->use_snet3 || c->use_snet4) {
    int waves = 4;
    const int nblk = c->use_snet4 ? launch_snet4(sa, true, true, c->st) : launch_snet3(sa, true, true, &waves, c->st);
    const long need = (long)nblk * waves * snet3_ring_floats_per_wave(c->n, c->nh);
    rc = c->dring.reserve(c, need); if (rc) return rc;
    *nloss = nblk;
  }
  sa.dring = c->dring;
  return NIF_OK;
}

// chunk size (points) of the two-stream pipeline, 0 = off.  nif_set_option("pipe_chunk", points) / NIF_PIPE_CHUNK;
// default: on for batches of at least four chunks of 2^17 points
static long pipe_chunk_points(const nif_ctx* c, long B) {
  long ch = c->opt_pipe_chunk;
  if (ch < 0) ch = 0;     // measured slower than the single-stream step: off unless asked for
  if (ch <= 0) return 0;
  ch = (ch + 2047) / 2048 * 2048;          // whole groups of 4 x 16-point tiles x 32 (and 32-point stash tiles)
  return ch;
}

static int ensure_pipe(nif_ctx* c, int nchunk) {
  if (!c->st2) {
    HIPCHK(hipStreamCreateWithFlags(&c->st2, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ev_start, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
  }
  while ((int)c->ev_chunk.size() < nchunk) {
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->ev_chunk.push_back(e);
  }
  return c->chunk_grad.reserve(c, (long)nchunk * c->pstride);
}

// Forward + adjoint + weight-gradient partial rows of the points [off, off + Bc) of a batch (NIF / NIFMultiScale).
// The ParameterNet forward and the fused ShapeNet kernel go to stream sa_st, everything that consumes their output (the
// ParameterNet adjoint, the weight-gradient reductions) to sb_st, ordered behind them by an event when the streams differ.
// ns = 0: loss = mse(u, y).  ns > 0 (Sobolev, whole batch only): + wj * mse(du/dx_seed, gt), k_sob instead of k_snet3/4;
// the ShapeNet stashes then hold (1+ns) blocks of tiles (real, then one block of tangent pseudo-tiles per seed).
static int step_chunk(nif_ctx* c, const float* xin0, const float* y0, const float* sw0, long off, long B, long Bg, int ns,
                      const int* seeds, const float* gt, float wj, hipStream_t sa_st, hipStream_t sb_st, hipStream_t pb_st,
                      float* partial, float* loss_partial, int* nloss_out, int chunk_idx, bool whole, SNetArgs* sa_out = nullptr,
                      const SobPlan* sp = nullptr, bool* pb_aside = nullptr) {
  int rc;
  const int ncol = c->pi + c->si;
  const long ntiles = (B + 31) / 32, t0 = off / 32;       // off is a multiple of 32 points
  const float* xin = xin0 + off * ncol;
  const float* y = y0 + off * c->so;
  const float* sw = sw0 ? sw0 + off : nullptr;
  // forward + adjoint
  PNetArgs pa; fill_pnet(c, pa, xin, B);
  pa.Z = c->Z + t0 * 32 * c->r; pa.DZ = c->DZ + t0 * 32 * c->r;
  if (pa.stash) pa.stash += t0 * 32 * 32 * c->NSTB;
  const bool fused_p = !pnet_force_stash() && pnet_bwg_supported(pa);
  if (!fused_p) { const int rcp = ensure_packed_p32(c); if (rcp) return rcp; }
  { ProfScope p_(c, NIF_PROF_PNET_FWD, sa_st); launch_pnet(pa, c->NSTB, !fused_p, sa_st); }
  SNetArgs sa; fill_snet(c, sa, xin, ncol, c->pi, B);
  sa.Z = pa.Z; sa.DZ = pa.DZ; sa.DU = c->DU + t0 * 32 * c->so;
  sa.stash = c->stash_s + t0 * 32 * 32 * c->NB;
  sa.y = y; sa.sw = sw; sa.u_out = nullptr; sa.loss_partial = loss_partial; sa.inv_bg = 1.0f / (float)Bg;
  if (!whole) sa.wg_cap = c->opt_pipe_wgs;        // leave room on every CU for the reductions of the previous chunk
  int nloss = (int)((ntiles + 3) / 4);
  rc = snet_plan(c, sa, ns, seeds, &nloss, sp); if (rc) return rc;
  // plain SIREN step on the bf16-split kernel: every ShapeNet weight gradient inside the training kernel (k_snet6) -- its workgroups
  // are the partial-gradient rows, so the row count of this step has to be the kernel's grid
  const bool fused_gw = ns == 0 && whole && c->use_snet4 && c->opt_fuse_gw && snet6_supported(sa) &&
                        snet6_rows(sa) == rows_for(c, ntiles);
  if (fused_gw) nloss = snet6_rows(sa);
  *nloss_out = nloss;
  // the ParameterNet adjoint goes aside (pb_st) to run NEXT TO the ShapeNet's weight-gradient reductions.  The fused step has none: the
  // adjoint stays behind k_snet6 on its stream -- no event, no stream wait, launch order = execution order.  *pb_aside tells the
  // caller whether there is a second stream to join
  if (fused_gw) pb_st = sb_st;
  if (pb_aside) *pb_aside = pb_st != sa_st;
  {   // mixed_bfloat16: the hidden layers' dL/da stash rows in bf16 when both the producer of this step (k_snet4<PR> / k_sobw<PR>)
      // and the consumer (k_gw_lds) have the form -- half the bytes of that operand on either side
    const int nbl = snet3_nbl(c->n);
    bool dab = sa.prec == 1 && (nbl == 2 || nbl == 4 || nbl == 8) && gw_da_bf16_ok(c->NB, c->NB, c->r);
    if (ns > 0) dab = dab && sobw_supported(sa, ns, sp && sp->any_par);
    else dab = dab && c->use_snet4 && !fused_gw;
    sa.da_bf16 = dab ? 1 : 0;
    // ... and, on the 128-wide kernel, the hidden matrices' input rows as 16-bit phases (k_gw8<R, true, true> reads them)
    sa.h_ph16 = (dab && ns == 0 && nbl == 8 && !c->cfg.s_resblock && !sa.nif_skip && gw_in_ph16_ok(c->NB, c->NB, c->r)) ? 1 : 0;
  }
  // what the producer of this step really writes (its own predicate, next to its kernels); the readers below follow THAT
  const bool wrote_da_bf16 = ns > 0 ? sob_writes_da_bf16(sa, ns, sp && sp->any_par)
                                    : (!fused_gw && c->use_snet4 && snet4_writes_da_bf16(sa));
  if (wrote_da_bf16 != (sa.da_bf16 != 0)) return fail(NIF_ERR_STATE, "internal: dL/da stash format of producer and plan disagree");
  const bool wrote_h_ph16 = ns == 0 && !fused_gw && c->use_snet4 && snet4_writes_h_ph16(sa);
  if (wrote_h_ph16 != (sa.h_ph16 != 0)) return fail(NIF_ERR_STATE, "internal: layer-input stash format of producer and plan disagree");
  {
    ProfScope p_(c, NIF_PROF_SNET, sa_st);
    if (ns > 0) {
      SobPar spar{};
      if (sp) spar = sob_par_of(*sp);      // (a plan without parameter columns has par = -1 throughout: sobolev_plan)
      if (sp && sp->any_par) { spar.ZT = c->zt_par; spar.DZT = c->dzt_par; }
      launch_sob(sa, true, ns, seeds, gt, wj, c->dring, nullptr, false, sa_st, sp ? &spar : nullptr);
    }
    else if (fused_gw) launch_snet6(sa, partial, c->pstride, sa_st, c->opt_s6_shape_generic);
    else if (c->use_snet4) { if (launch_snet4(sa, true, false, sa_st) < 0) return fail(NIF_ERR_STATE, "internal: no k_snet4 form for this net (SIREN planes not packed as half pairs)"); }
    else if (c->use_snet3) launch_snet3(sa, true, false, nullptr, sa_st);
    else launch_snet(sa, c->NB, true, sa_st);
  }
  if (act_on(c)) {   // + c/Bg sum phi'(out) M^(k) into dL/dz, before the ParameterNet adjoint consumes it; its loss partials
    const long nlp = (B + 255) / 256;
    rc = c->act_loss.reserve(c, nlp); if (rc) return rc;
    const bool l1 = c->act_l2 == 0.f;
    launch_actreg_points(l1, c->theta, c->last_w, c->last_b, c->r, c->po, sa.Z, B, (l1 ? c->act_l1 : c->act_l2) / (float)Bg, sa.DZ,
                         c->act_loss, sa_st);
  }
  if (sb_st != sa_st || pb_st != sa_st) {
    HIPCHK(hipEventRecord(c->ev_chunk[chunk_idx], sa_st));
    if (sb_st != sa_st) HIPCHK(hipStreamWaitEvent(sb_st, c->ev_chunk[chunk_idx], 0));
    if (pb_st != sa_st && pb_st != sb_st) HIPCHK(hipStreamWaitEvent(pb_st, c->ev_chunk[chunk_idx], 0));
  }
  // weight gradients -> partial rows
  const int rows = rows_for(c, ntiles);
  { ProfScope p_(c, NIF_PROF_PNET_BWD, pb_st);
    // the compute-bound adjoint also pulls the first gradient kernel's stash slot (dL/da of the first layer) through
    // the cache hierarchy -- see PbwArgs::touch.  NIF_PBW_TOUCH=0 turns it off (A/B)
    static const bool touch_on = [] { const char* e = getenv("NIF_PBW_TOUCH"); return !(e && e[0] == '0'); }();
    const float* touch = (touch_on && whole && pb_st == sb_st && !fused_gw) ? sa.stash + (long)(c->nh + 1) * c->slot_s : nullptr;
    if (fused_p) launch_pnet_bwg(pa, partial, c->pstride, rows, pb_st, touch, (long)c->NB * 1024);
    else launch_pnet_bwd(pa, c->NSTB, pb_st); }
  ProfScope pgw(c, NIF_PROF_GW, sb_st);
  const GwArgs base = gw_base(c, ntiles, B, partial);
  if (!fused_gw) {     // ShapeNet: its reductions also run over the tangent pseudo-tiles
    GwArgs sbase = base;
    gw_add_tangents(sbase, ns, seeds);
    long first_ntiles = sbase.ntiles;
    if (sp) first_ntiles = ntiles * (1 + sp->nsc);      // a parameter stream has no tangent input here (x' = 0): its pairs go to sob_par_pass
    if (sp && sp->hess) first_ntiles = ntiles * 3;      // nor has the second-order stream (a'' = 0 at the first layer)
    if (gw_hyper_snet_stack(c, sbase, sa, xin, sa.Z, 0, first_ntiles, wrote_da_bf16, wrote_h_ph16, rows, sb_st) < 0)
      return fail(NIF_ERR_STATE, "internal: bf16 dL/da stash rows without a reader of that form");
  }
  if (!fused_p) gw_pnet_stack(c, base, xin, pa.stash, pa.DZ, pa.omega, rows, pb_st);
  if (sa_out) *sa_out = sa;
  HIPCHK(hipGetLastError());
  return NIF_OK;
}

// k_small's tables of this context (the index map of its LDS images and the tensor descriptors: offsets only), built once
static int ensure_small_tables(nif_ctx* c, const PNetArgs& pa, const SNetArgs& sa) {
  if (c->small_idx) return NIF_OK;
  if (c->capturing) return fail(NIF_ERR_STATE, "small-batch step tables inside a graph capture (nif_graph_begin builds them)");
  std::vector<int> idx, desc;
  small_tables(pa, sa, idx, desc);
  // the context takes the tables only when both exist and are filled: a failure on the way leaves it without any (the next call tries again)
  DevBuf<int> d_idx, d_desc;
  int rc = d_idx.alloc((long)idx.size()); if (rc) return rc;
  rc = d_desc.alloc((long)desc.size()); if (rc) return rc;
  HIPCHK(hipMemcpy(d_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_desc, desc.data(), desc.size() * sizeof(int), hipMemcpyHostToDevice));
  c->small_idx = std::move(d_idx); c->small_desc = std::move(d_desc);
  return NIF_OK;
}
// r6: the row reduction of a plain step waits for its consumer when nothing else needs [grad | loss] first: the optimizer step runs it fused
// with the update (k_reduce_opt: one launch less per step -- 5 of the 31 us of a 512-point step, 0.5 % of the 2^20-point one).  The
// reduction is NOT deferred with a communicator attached, inside a graph capture, under the profiler (its per-group events would lose
// the REDUCE group) or when a regulariser adds to the gradient behind it.
int nif_tail_flush(nif_ctx* c) {
  if (!c->tail_pending) return NIF_OK;
  c->tail_pending = false;
  launch_reduce(c->partial, c->pstride, c->tail_rows, c->loss_partial, c->tail_nloss, c->grad, c->P, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
static bool tail_can_defer(const nif_ctx* c) {
  if (!c->opt_fuse_tail || c->comm || c->capturing || c->prof_on) return false;
  if ((c->reg_l1 != 0.f || c->reg_l2 != 0.f) && c->reg_hi > c->reg_lo) return false;
  if (c->sreg_l1 != 0.f || c->sreg_l2 != 0.f) return false;
  return true;
}
// a Keras loss-metric accumulation that nif_metric_accumulate left for the next k_small launch (r6: one launch less per small step):
// everything that would change grad[P] or read the metric without such a launch runs it now
int nif_metric_flush(nif_ctx* c) {
  if (!c->metric_pending) return NIF_OK;
  const int rc = nif_tail_flush(c); if (rc) return rc;
  c->metric_pending = false;
  launch_metric(c->grad, c->P, c->metric_pending_w, c->metric, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
int nif_enter(nif_ctx* c, nif_flush what) {
  HIPCHK(hipSetDevice(c->dev));
  if (what == NIF_FLUSH_NONE) return NIF_OK;
  const int rc = nif_tail_flush(c); if (rc) return rc;
  return what == NIF_FLUSH_METRIC ? nif_metric_flush(c) : NIF_OK;
}
static int loss_grad_core(nif_ctx* c, const float* xin, const float* y, const float* sw, int64_t B, int64_t Bg, int ns,
                          const int* seeds, const float* gt, float wj, const SobPlan* sp = nullptr) {
  c->last_step_small = false;      // (also what a refused step leaves behind)
  // r6: a small batch of a small net -- ONE launch for the loss and every gradient (k_small: fp32 FMAs straight from theta, no plane
  // packing), then the usual row reduction.  configs[0]'s 512-point steps spent 82 us in eleven tile-kernel launches
  if (ns == 0 && c->opt_small_step && B <= NIF_SMALL_MAX_B && c->kind != NIF_KIND_LASTLAYER && !act_on(c) && !c->opt_fp32_mfma) {
    if (!c->have_params) return fail(NIF_ERR_STATE, "parameters not set (call nif_set_params first)");
    PNetArgs pa; fill_pnet(c, pa, xin, B);
    SNetArgs sa; fill_snet(c, sa, xin, c->pi + c->si, c->pi, B);
    if (small_supported(pa, sa) && small_rows(B) <= 256) {
      int rc = ensure_rows(c, B); if (rc) return rc;      // (no point workspaces, no stashes: k_small keeps everything on chip)
      const int rows = small_rows(B);
      if (rows > c->rows_cap()) return fail(NIF_ERR_STATE, "internal: partial-row buffer too small for the small-batch step");
      if (rows > c->loss_partial.n) return fail(NIF_ERR_STATE, "internal: loss partial buffer too small for the small-batch step");
      c->grad_rewritten();
      sa.y = y; sa.sw = sw; sa.loss_partial = c->loss_partial; sa.inv_bg = 1.0f / (float)Bg;
      rc = ensure_small_tables(c, pa, sa); if (rc) return rc;
      const bool mp = c->metric_pending && c->metric != nullptr;
      { ProfScope p_(c, NIF_PROF_SNET);
        launch_small(pa, sa, c->partial, c->pstride, c->P, c->small_idx, c->small_desc, mp ? c->metric : nullptr, c->metric_pending_w,
                     c->grad + c->P, c->st); }
      if (mp) c->metric_pending = false;
      c->last_step_small = true;
      if (c->jac_l1 == 0.f && tail_can_defer(c)) { c->tail_pending = true; c->tail_rows = rows; c->tail_nloss = rows; }
      else { ProfScope pr_(c, NIF_PROF_REDUCE); launch_reduce(c->partial, c->pstride, rows, c->loss_partial, rows, c->grad, c->P, c->st); }
      if (c->jac_l1 != 0.f) { rc = jac_reg_pass(c, xin, B, Bg); if (rc) return rc; }
      HIPCHK(hipGetLastError());
      return NIF_OK;
    }
  }
  int rc = nif_metric_flush(c); if (rc) return rc;
  rc = ensure_packed(c); if (rc) return rc;
  const long ntiles = (B + 31) / 32;
  if (ns > 0) { rc = ensure_packed32(c); if (rc) return rc; }
  if (ns > 0) {
    if (c->kind != NIF_KIND_LASTLAYER && !c->jac_ok)
      return fail(NIF_ERR_INVALID, "Sobolev training: one weight plane and the small hyper-vectors of this shape exceed the 160 KB LDS of a CU");
    if (c->cfg.s_resblock && (c->nh & 1)) return fail(NIF_ERR_INVALID, "resblock ShapeNet with an odd matrix count");
  }
  rc = ensure_capacity(c, ntiles * 32 * (1 + ns), true); if (rc) return rc;
  if (sp && sp->any_par) {   // z' = dz/dp of the parameter columns, in front of the ShapeNet
    PNetArgs pa; fill_pnet(c, pa, xin, B);
    rc = ensure_zt_par(c, pa, ntiles, true); if (rc) return rc;
  }
  c->grad_rewritten();
  if (c->kind == NIF_KIND_LASTLAYER) return loss_grad_ll(c, xin, y, sw, B, Bg, ns, sp, gt, wj);
  // Two-stream pipeline over chunks of the batch (plain step on the 16-point-tile kernels): the fused ShapeNet kernel of
  // chunk i+1 (VALU / latency bound, 2 workgroups per CU) overlaps the HBM-bound weight-gradient reductions of chunk i
  const long chunk = (ns == 0 && c->use_snet3 && !act_on(c) && c->jac_l1 == 0.f) ? pipe_chunk_points(c, B) : 0;
  if (chunk <= 0 || chunk >= B) {
    int nloss = 0;
    SNetArgs sae;
    // the compute-bound ParameterNet adjoint runs on a second stream NEXT TO the HBM-bound weight-gradient reductions of
    // the ShapeNet (both only need the fused kernel's outputs); joined in front of the row reduction
    const bool side = c->opt_side_pnet && B >= 65536;
    if (side) { rc = ensure_pipe(c, 1); if (rc) return rc; }
    bool aside = false;
    rc = step_chunk(c, xin, y, sw, 0, B, Bg, ns, seeds, gt, wj, c->st, c->st, side ? c->st2 : c->st, c->partial, c->loss_partial,
                    &nloss, 0, true, &sae, sp, &aside);
    if (rc) return rc;
    if (aside) {
      HIPCHK(hipEventRecord(c->ev_done, c->st2));
      HIPCHK(hipStreamWaitEvent(c->st, c->ev_done, 0));
    }
    const int rows = rows_for(c, ntiles);
    if (ns == 0 && !act_on(c) && c->jac_l1 == 0.f && !(sp && sp->any_par) && tail_can_defer(c)) {
      c->tail_pending = true; c->tail_rows = rows; c->tail_nloss = nloss;
      HIPCHK(hipGetLastError());
      return NIF_OK;
    }
    ProfScope pr_(c, NIF_PROF_REDUCE);
    launch_reduce(c->partial, c->pstride, rows, c->loss_partial, nloss, c->grad, c->P, c->st);
    if (act_on(c)) {   // the plane side of the activity regulariser and its loss, on top of the reduced gradient
      const long need = (long)NIF_ACT_SLABS * (c->r + 1) * c->po;
      rc = c->act_part.reserve(c, need); if (rc) return rc;
      const bool l1 = c->act_l2 == 0.f;
      launch_actreg_planes(l1, c->theta, c->last_w, c->last_b, c->r, c->po, c->Z, B, NIF_ACT_SLABS, c->act_part, c->st);
      launch_actreg_apply(c->act_part, NIF_ACT_SLABS, c->r, c->po, (l1 ? c->act_l1 : c->act_l2) / (float)Bg, c->last_w, c->last_b,
                          c->act_loss, (int)((B + 255) / 256), c->grad, c->P, c->st);
    }
    if (c->jac_l1 != 0.f) { rc = jac_reg_pass(c, xin, B, Bg); if (rc) return rc; }
    if (sp && sp->any_par) { rc = sob_par_pass(c, xin, B, Bg, *sp, sae); if (rc) return rc; }
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  const int nchunk = (int)((B + chunk - 1) / chunk);
  rc = ensure_pipe(c, nchunk); if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev_start, c->st));             // stream B starts behind whatever st has queued (packing, Adam)
  HIPCHK(hipStreamWaitEvent(c->st2, c->ev_start, 0));
  const long lp_stride = c->loss_partial.n / nchunk;            // loss partials of chunk i at i * lp_stride
  for (int i = 0; i < nchunk; ++i) {
    const long off = (long)i * chunk;
    const long Bc = B - off < chunk ? B - off : chunk;
    int nloss = 0;
    rc = step_chunk(c, xin, y, sw, off, Bc, Bg, 0, nullptr, nullptr, 0.f, c->st, c->st2, c->st2, c->partial,
                    c->loss_partial + i * lp_stride, &nloss, i, false);
    if (rc) return rc;
    if (nloss > lp_stride) return fail(NIF_ERR_STATE, "loss partial buffer too small for the chunk pipeline");
    // this chunk's partial rows -> row i of the second-level buffer (loss in column P); stream B is in order, so the
    // next chunk's reductions may overwrite the partial rows afterwards
    const int rows = rows_for(c, (Bc + 31) / 32);
    launch_reduce(c->partial, c->pstride, rows, c->loss_partial + i * lp_stride, nloss, c->chunk_grad + (long)i * c->pstride, c->P, c->st2);
  }
  HIPCHK(hipEventRecord(c->ev_done, c->st2));
  HIPCHK(hipStreamWaitEvent(c->st, c->ev_done, 0));
  {
    ProfScope pr_(c, NIF_PROF_REDUCE);   // rows of the chunks -> flat gradient | loss (column P rides along as a regular column)
    launch_reduce(c->chunk_grad, c->pstride, nchunk, nullptr, 0, c->grad, c->P + 1, c->st);
  }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}

extern "C" int nif_loss_grad_dev(nif_ctx* c, const float* xin, const float* y, const float* sw, int64_t B, int64_t Bg) {
  if (!c || !xin || !y || B <= 0 || Bg < B) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)      // (a step whose gradient was never consumed: its rows are about to be overwritten)
  return loss_grad_core(c, xin, y, sw, B, Bg, 0, nullptr, nullptr, 0.f);
}

// ---- the snapshot-wise training step of the last-layer class (include/nif_hip_snapfit.h, k_snapfit.hip) ----------------
// loss_grad_ll's step on the table [repeat(p, M) | tile(x, T)] from its factors: the ParameterNet over the T rows of p, the ShapeNet
// (with its training stash) over the M rows of x, the head over (t, m), then each net's adjoint and weight-gradient reductions over its
// own tiles.
static int snapfit_check(const nif_snapfit_args* a) {
  int rc = snap_args_check(a, NIF_SNAPFIT_ABI_VERSION, "nif_snapfit_args"); if (rc) return rc;
  const nif_ctx* c = a->ctx;
  const char* who = "nif_snapshot_loss_grad";
  if (!c || a->T < 0 || a->M < 0 || a->batch_global < 0) return fail(NIF_ERR_INVALID, "bad argument");
  const int64_t n = a->T * a->M;
  if (n > 0 && (!a->p || !a->x || !a->y)) return fail(NIF_ERR_INVALID, "bad argument");
  if (a->batch_global != 0 && a->batch_global < n) return fail(NIF_ERR_INVALID, "bad argument");
  if (c->kind != NIF_KIND_LASTLAYER)
    return fail(NIF_ERR_INVALID, std::string(who) + ": not built for the hypernetwork classes (NIF, NIFMultiScale): their weight gradients are "
                                 "per-snapshot sums no kernel forms; the step factors for NIFMultiScaleLastLayerParameterized only");
  if (c->cfg.mixed_policy != NIF_POLICY_FLOAT32)
    return fail(NIF_ERR_INVALID, std::string(who) + ": not built for the " +
                                 (c->cfg.mixed_policy == NIF_POLICY_MIXED_BF16 ? "mixed_bfloat16" : "mixed_float16") + " policy");
  if (act_on(c)) return fail(NIF_ERR_INVALID, std::string(who) + ": not built with an activity regulariser set on the context");
  if (c->jac_l1 != 0.f) return fail(NIF_ERR_INVALID, std::string(who) + ": not built with a latent Jacobian regulariser set on the context");
  if (!snapfit_supported(c->r, c->so))
    return fail(NIF_ERR_INVALID, std::string(who) + ": so * latent_dim = " + std::to_string(c->so * c->r) + " > 64");
  return snap_not_capturing(c, who);
}
static int snapshot_loss_grad_core(nif_ctx* c, const float* p, const float* x, const float* y, const float* sw, long T, long M, long Bg) {
  c->last_step_small = false;
  int rc = nif_metric_flush(c); if (rc) return rc;      // (grad[P] is rewritten without a k_small launch)
  rc = ensure_packed(c); if (rc) return rc;
  if (T == 0 || M == 0) {
    HIPCHK(hipMemsetAsync(c->grad, 0, sizeof(float) * (size_t)(c->P + 1), c->st));
    c->grad_rewritten();
    return NIF_OK;
  }
  rc = ensure_capacity(c, T > M ? T : M, true); if (rc) return rc;
  rc = c->sf_dap.reserve(c, snapfit_dap_floats(T, M, c->r)); if (rc) return rc;
  c->grad_rewritten();
  const long mtiles = (M + 31) / 32, ttiles = (T + 31) / 32;
  const int si = c->si;
  PNetArgs pa; fill_pnet(c, pa, p, T); pa.ncol = c->pi;
  const bool fused_p = !pnet_force_stash() && pnet_bwg_supported(pa);
  if (!fused_p) { const int rcp = ensure_packed_p32(c); if (rcp) return rcp; }
  { ProfScope p_(c, NIF_PROF_PNET_FWD); launch_pnet(pa, c->NSTB, !fused_p, c->st); }
  PNetArgs ma;
  if (!c->use_wide) { ensure_ll_mlp_planes(c); fill_snet_mlp(c, ma, x, si, 0, M); }
  {      // phi of the mesh, stashed: the 32-point MLP kernels (k_snet4<.., LL> fuses the point-wise head), layer by layer from 129 units
    ProfScope p_(c, NIF_PROF_SNET_FWD);
    if (c->use_wide) wide_forward(c, x, si, 0, M, true);
    else launch_pnet(ma, c->NB, true, c->st);
  }
  {
    SnapFitArgs ha; memset(&ha, 0, sizeof(ha));
    ha.loss_kind = c->loss_kind; ha.PHI = c->PHI; ha.A = c->Z; ha.bias = c->theta + c->ll_bias; ha.last_w = c->theta + c->last_w;
    ha.y = y; ha.sw = sw; ha.T = T; ha.M = M; ha.r = c->r; ha.so = c->so; ha.inv_bg = 1.0f / (float)Bg;
    ha.DPHI = c->DPHI; ha.DU = c->DU; ha.DAP = c->sf_dap; ha.DA = c->DA; ha.DZL = c->DZL; ha.loss_partial = c->loss_partial;
    ProfScope p_(c, NIF_PROF_SNET);
    launch_snapfit_head(ha, c->st);
    launch_snapfit_da(ha, c->st);
  }
  // The ShapeNet's reductions run over the mesh tiles, the ParameterNet's over the snapshot tiles: each group gets the partial rows of
  // its own tile count and is reduced on its own below (the two column ranges of a row are disjoint: theta is [ParameterNet | ShapeNet]),
  // so nothing depends on what a reduction kernel leaves in a row it has no tile for
  const int rows_m = rows_for(c, mtiles), rows_t = rows_for(c, ttiles);
  if (c->use_wide) wide_backward(c, x, si, 0, M, rows_m);
  {
    ProfScope p_(c, NIF_PROF_GW);
    const GwArgs base = gw_base(c, mtiles, M, c->partial);
    GwArgs g = base;
    if (!c->use_wide) {
      launch_pnet_bwd(ma, c->NB, c->st);
      const int nms = c->nh;
      float* sST = c->stash_s;
      g.DA = sST + (long)(nms + 1) * c->slot_s; g.xin = x; g.ncol = si; g.col0 = 0; g.nd = si; g.scale = ma.omega;
      g.W = dense_ref(c->s_first_w, c->si, c->n); g.Bv = vec_ref(c->s_first_b, c->n);
      launch_gw_first(g, c->NB, rows_m, c->st);
      for (int mi = 0; mi < nms; ++mi) {
        g = base; g.IN = sST + (long)mi * c->slot_s; g.DA = sST + (long)(nms + 2 + mi) * c->slot_s; g.scale = ma.omega;
        long w_off, b_off; snet_mat(c, mi, &w_off, &b_off);
        g.W = dense_ref(w_off, c->n, c->n); g.Bv = vec_ref(b_off, c->n);
        if (launch_gw_mfma(g, c->NB, c->NB, rows_m, c->st) < 0) return fail(NIF_ERR_STATE, "internal: no reader for the hidden matrices' stash rows");
      }
      g = base; g.IN = sST + (long)nms * c->slot_s; g.SM = c->DPHI; g.nc = c->r * c->so;
      g.W = dense_ref(c->s_bott_w, c->n, c->r * c->so); g.Bv = vec_ref(c->s_bott_b, c->r * c->so);
      launch_gw_out(g, c->NB, rows_m, c->st);
    }
    g = base; g.IN = c->use_wide ? nullptr : c->stash_s + (long)c->nh * c->slot_s; g.SM = c->DU; g.nc = c->so;   // (k_gw_bias reads SM alone)
    g.W = dense_ref(0, 0, c->so); g.Bv = vec_ref(c->ll_bias, c->so);
    launch_gw_out(g, c->NB, rows_m, c->st);
  }
  {
    ProfScope p_(c, NIF_PROF_PNET_BWD);
    if (fused_p) launch_pnet_bwg(pa, c->partial, c->pstride, rows_t, c->st);
    else launch_pnet_bwd(pa, c->NSTB, c->st);
    const GwArgs base = gw_base(c, ttiles, T, c->partial);
    if (!fused_p) gw_pnet_stack(c, base, p, c->stash_p, c->DZL, pa.omega, rows_t, c->st, c->pi);
    GwArgs g = base; g.IN = c->ZL; g.SM = c->DA; g.nc = c->r;   // latent (padded rows) x dL/da
    g.W = dense_ref(c->last_w, c->r, c->r); g.Bv = vec_ref(c->last_b, c->r);
    launch_gw_out(g, c->RB, rows_t, c->st);
  }
  {
    ProfScope pr_(c, NIF_PROF_REDUCE);
    const long np = c->s_first_w;      // (the loss slot of the first reduction is the first column of the second)
    launch_reduce(c->partial, c->pstride, rows_t, nullptr, 0, c->grad, np, c->st);
    launch_reduce(c->partial + np, c->pstride, rows_m, c->loss_partial, (int)mtiles, c->grad + np, c->P - np, c->st);
  }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_snapshot_loss_grad_dev(const nif_snapfit_args* a) {
  int rc = snapfit_check(a); if (rc) return rc;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  const long n = (long)(a->T * a->M);
  return snapshot_loss_grad_core(c, a->p, a->x, a->y, a->sw, (long)a->T, (long)a->M, a->batch_global ? (long)a->batch_global : n);
}
extern "C" int nif_snapshot_loss_grad(const nif_snapfit_args* a) {
  int rc = snapfit_check(a); if (rc) return rc;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  const long T = (long)a->T, M = (long)a->M, n = T * M;
  nif_snapfit_args d = *a;
  if (n > 0) {
    rc = stage(c, c->d_a, a->p, T * c->pi); if (rc) return rc;
    rc = stage(c, c->d_b, a->x, M * c->si); if (rc) return rc;
    rc = stage(c, c->d_d, a->y, n * c->so); if (rc) return rc;
    if (a->sw) { rc = stage(c, c->d_c, a->sw, n); if (rc) return rc; }
    d.p = c->d_a; d.x = c->d_b; d.y = c->d_d; d.sw = a->sw ? c->d_c.p : nullptr;
  }
  rc = nif_snapshot_loss_grad_dev(&d); if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

// ---- sensor placement on the last-layer class's basis (include/nif_hip_sensors.h, k_sensors.hip) ------------------------
static int sensors_check(const nif_sensors_args* a) {
  int rc = snap_args_check(a, NIF_SENSORS_ABI_VERSION, "nif_sensors_args"); if (rc) return rc;
  const nif_ctx* c = a->ctx;
  const char* who = "nif_select_sensors";
  if (!c) return fail(NIF_ERR_INVALID, "bad argument");
  if (c->kind != NIF_KIND_LASTLAYER)
    return fail(NIF_ERR_INVALID, std::string(who) + ": not built for the hypernetwork classes (NIF, NIFMultiScale): their basis du/dz depends on "
                                 "the latent, and selection on it at a given latent is not built; the field is linear in a fixed basis "
                                 "phi(x) for NIFMultiScaleLastLayerParameterized only");
  if (a->M < 1) return fail(NIF_ERR_INVALID, std::string(who) + ": M = " + std::to_string(a->M) + " < 1");
  if (!sens_supported(c->r)) return fail(NIF_ERR_INVALID, std::string(who) + ": latent_dim " + std::to_string(c->r) + " > 64");
  if (a->K < 1 || a->K > c->r)
    return fail(NIF_ERR_INVALID, std::string(who) + ": K = " + std::to_string(a->K) + " outside 1 .. latent_dim = " + std::to_string(c->r) +
                                 " (the rows of phi live in R^r: more sensors than r is oversampling, a different algorithm that is not built)");
  if (!a->x || !a->pivots_out || !a->diag_out) return fail(NIF_ERR_INVALID, "bad argument");
  return snap_not_capturing(c, who);
}
// phi of the mesh as nif_x_to_phi runs it, then K dependent steps of one streaming pass each: 2 K launches behind the first (the
// update behind the last pivot would serve no step)
static int select_sensors_core(nif_ctx* c, const float* x, long M, const unsigned char* mask, int K, long long* piv, float* d) {
  int rc = ensure_packed(c); if (rc) return rc;
  rc = ensure_capacity(c, M, false); if (rc) return rc;
  const long tiles = (M + 31) / 32, sop = (long)c->so * c->r;
  const long f_pr = 2L * NIF_SENS_GRID, f_ps = NIF_SENS_GRID, f_q = snap_r4((long)K * c->r), f_sc = tiles * c->so * 32;
  rc = c->sens.reserve(c, f_pr + f_ps + f_q + f_sc + tiles * sop * 32); if (rc) return rc;
  { ProfScope p_(c, NIF_PROF_SNET_FWD); ll_phi_pass(c, x, c->si, 0, M); }
  SensArgs sa; memset(&sa, 0, sizeof(sa));
  sa.PHI = c->PHI; sa.PR = reinterpret_cast<long long*>(c->sens.p); sa.PS = c->sens + f_pr; sa.Q = sa.PS + f_ps; sa.SC = sa.Q + f_q;
  sa.RES = sa.SC + f_sc; sa.piv = piv; sa.d = d; sa.mask = mask; sa.M = M; sa.r = c->r; sa.so = c->so;
  ProfScope p_(c, NIF_PROF_REDUCE);
  launch_sens_init(sa, c->st);
  for (int k = 0; k < K; ++k) {
    sa.k = k;
    launch_sens_pivot(sa, c->st);
    if (k + 1 < K) launch_sens_update(sa, c->st);
  }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_select_sensors_dev(const nif_sensors_args* a) {
  int rc = sensors_check(a); if (rc) return rc;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  static_assert(sizeof(long long) == sizeof(int64_t), "pivots travel as they are");
  return select_sensors_core(c, a->x, (long)a->M, a->mask, (int)a->K, reinterpret_cast<long long*>(a->pivots_out), a->diag_out);
}
extern "C" int nif_select_sensors(const nif_sensors_args* a) {
  int rc = sensors_check(a); if (rc) return rc;
  nif_ctx* c = a->ctx;
  NIF_ENTER(a->ctx, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  const long M = (long)a->M, K = (long)a->K;
  rc = stage(c, c->d_a, a->x, M * c->si); if (rc) return rc;
  rc = stage(c, c->d_d, nullptr, 3 * K); if (rc) return rc;      // pivots (int64) | d
  nif_sensors_args d = *a;
  d.x = c->d_a; d.pivots_out = reinterpret_cast<int64_t*>(c->d_d.p); d.diag_out = c->d_d + 2 * K;
  if (a->mask) {
    rc = c->d_c.reserve(c, (M + 3) / 4); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->d_c.p, a->mask, (size_t)M, hipMemcpyHostToDevice, c->st));
    d.mask = reinterpret_cast<const uint8_t*>(c->d_c.p);
  }
  rc = nif_select_sensors_dev(&d); if (rc) return rc;
  HIPCHK(hipMemcpyAsync(a->pivots_out, d.pivots_out, sizeof(int64_t) * (size_t)K, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(a->diag_out, d.diag_out, sizeof(float) * (size_t)K, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

// Size every workspace of a training step over up to B_max points (n_tangents Sobolev seeds, 0 = plain step) now, so
// that no device allocation / stream synchronisation happens inside a later (timed) step.
extern "C" int nif_reserve(nif_ctx* c, int64_t B_max, int32_t n_tangents) {
  if (!c || B_max <= 0 || n_tangents < 0 || n_tangents > 16) return fail(NIF_ERR_INVALID, "bad argument");
  if (n_tangents > 3) n_tangents = 3;      // (more x_index columns run as passes over groups of three)
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  int rc = ensure_packed(c); if (rc) return rc;
  const long ntiles = (B_max + 31) / 32;
  rc = ensure_capacity(c, ntiles * 32 * (1 + n_tangents), true); if (rc) return rc;
  if (c->kind == NIF_KIND_LASTLAYER) {
    if (c->use_ll4) {
      SNetArgs sa; fill_snet_ll(c, sa, nullptr, c->pi + c->si, c->pi, B_max);
      int nblk = 0;
      rc = ll4_plan(c, sa, &nblk); if (rc) return rc;
    }
    return NIF_OK;
  }
  SNetArgs sa; fill_snet(c, sa, nullptr, c->pi + c->si, c->pi, B_max);
  int nloss = 0;
  const int seeds[3] = {0, 0, 0};
  rc = snet_plan(c, sa, n_tangents, seeds, &nloss); if (rc) return rc;
  const long chunk = (n_tangents == 0 && c->use_snet3) ? pipe_chunk_points(c, B_max) : 0;
  if (chunk > 0 && chunk < B_max) { rc = ensure_pipe(c, (int)((B_max + chunk - 1) / chunk)); if (rc) return rc; }
  return NIF_OK;
}

static int sobolev_plan(nif_ctx* c, const int32_t* x_idx, int32_t nx, SobPlan* sp) {
  if (!x_idx || nx < 1 || nx > 3) return fail(NIF_ERR_INVALID, "internal: a Sobolev pass carries 1..3 columns");
  memset(sp, 0, sizeof(*sp));
  sp->ns = nx;
  for (int d = 0; d < nx; ++d) {
    if (x_idx[d] < 0 || x_idx[d] >= c->pi + c->si) return fail(NIF_ERR_INVALID, "Sobolev x_index out of range (0 <= i < pi_dim + si_dim)");
    for (int e = 0; e < d; ++e)
      if (x_idx[e] == x_idx[d]) return fail(NIF_ERR_INVALID, "Sobolev x_index lists a column twice");
  }
  int q = 0;
  for (int d = 0; d < nx; ++d)
    if (x_idx[d] >= c->pi) { sp->seeds[q] = x_idx[d] - c->pi; sp->par[q] = -1; sp->gcol[q] = d; ++q; }
  sp->nsc = q;
  for (int d = 0; d < nx; ++d)
    if (x_idx[d] < c->pi) { sp->seeds[q] = 0; sp->par[q] = x_idx[d]; sp->gcol[q] = d; ++q; sp->any_par = true; }
  for (; q < 3; ++q) { sp->seeds[q] = 0; sp->par[q] = -1; sp->gcol[q] = q; }
  return NIF_OK;
}
// The columns of x_index in groups of <= 3 (the kernels carry up to three tangent streams): the derivative term is a sum over the
// columns, so group k > 0 is one more pass with the primal mse (and every regularisation term) switched off, its [grad | loss]
// added to the first pass's.  y_idx = NULL: every output; otherwise the derivative term covers the listed outputs only
// (gradient.py:207-231).  dydx rows are [so][nx] either way (rows of unlisted outputs are not read into the loss).
static int sobolev_check(nif_ctx* c, const int32_t* x_idx, int32_t nx, const int32_t* y_idx, int32_t ny, unsigned* ymask, int* ny_out) {
  if (!x_idx || nx < 1 || nx > 16) return fail(NIF_ERR_INVALID, "Sobolev training takes 1..16 input columns in x_index");
  { const int rcw = wide_refused(c, "Sobolev step / forward"); if (rcw) return rcw; }
  for (int d = 0; d < nx; ++d) {
    if (x_idx[d] < 0 || x_idx[d] >= c->pi + c->si) return fail(NIF_ERR_INVALID, "Sobolev x_index out of range (0 <= i < pi_dim + si_dim)");
    for (int e = 0; e < d; ++e)
      if (x_idx[e] == x_idx[d]) return fail(NIF_ERR_INVALID, "Sobolev x_index lists a column twice");
  }
  *ymask = 0; *ny_out = 0;
  if (y_idx) {
    if (ny < 1 || ny > c->so) return fail(NIF_ERR_INVALID, "Sobolev y_index: 1..output_dim distinct outputs");
    for (int i = 0; i < ny; ++i) {
      if (y_idx[i] < 0 || y_idx[i] >= c->so) return fail(NIF_ERR_INVALID, "Sobolev y_index out of range");
      if (*ymask & (1u << y_idx[i])) return fail(NIF_ERR_INVALID, "Sobolev y_index lists an output twice");
      *ymask |= 1u << y_idx[i];
    }
    *ny_out = ny;
  }
  return NIF_OK;
}
// Columns per pass of a Sobolev step / forward: three tangent streams where the kernel's working set allows it.  A parameter-column
// stream of the hypernetwork classes keeps 4 x (r x 80) floats of per-wave LDS next to the planes (k_sob.hip launch_sob): at 128
// units and latent_dim 8 three of them exceed the 160 KB by a few KB (fuzz sweep r04, seed 7, case 5) -- the passes then take two
// columns, or one, instead of refusing the shape.  Probed with the query the step itself makes (snet_plan), no launch.
static int sob_cols_per_pass(nif_ctx* c, const int32_t* x_idx, int nx) {
  if (c->kind == NIF_KIND_LASTLAYER) return 3;        // (parameter columns are heads of the epilogue there, not streams)
  if (ensure_packed(c) != NIF_OK) return 3;           // (surfaces again, with its message, in the step)
  for (int gs = 3; gs > 1; --gs) {
    bool ok = true;
    for (int g0 = 0; g0 < nx && ok; g0 += gs) {
      const int ng = nx - g0 < gs ? nx - g0 : gs;
      SobPlan sp;
      if (sobolev_plan(c, x_idx + g0, ng, &sp) != NIF_OK) return 3;
      SNetArgs sa; fill_snet(c, sa, nullptr, c->pi + c->si, c->pi, 64);
      const SobPar spq = sob_par_of(sp);
      ok = launch_sob(sa, true, ng, sp.seeds, nullptr, 0.f, nullptr, nullptr, true, c->st, &spq) >= 0;
    }
    if (ok) return gs;
  }
  return 1;
}

// the first-order Sobolev step behind its entry points' checks and guard; ymask / nys: sobolev_check's
static int sobolev_step(nif_ctx* c, const float* xin, const float* y, const float* dydx, const float* sw, int64_t B, int64_t Bg,
                        const int32_t* x_idx, int32_t nx, unsigned ymask, int nys, float w_jac) {
  int rc = NIF_OK;
  const int gs = sob_cols_per_pass(c, x_idx, nx);
  const int ngroups = (nx + gs - 1) / gs;
  if (ngroups > 1 && !c->sob_acc) { rc = c->sob_acc.alloc(c->P + 1); if (rc) return rc; }
  for (int k = 0; k < ngroups; ++k) {
    const int g0 = gs * k, ng = nx - g0 < gs ? nx - g0 : gs;
    SobPlan sp;
    rc = sobolev_plan(c, x_idx + g0, ng, &sp); if (rc) break;
    for (int q = 0; q < 3; ++q) sp.gcol[q] += g0;
    sp.gstride = nx; sp.nx_all = nx; sp.ny = nys; sp.ymask = ymask; sp.no_primal = k > 0;
    const RegsOff regs_off(c, k > 0);      // the regularisation losses belong to the first pass
    rc = loss_grad_core(c, xin, y, sw, B, Bg, ng, sp.seeds, dydx, w_jac, &sp);
    if (rc) break;
    if (ngroups > 1) {
      if (k == 0) { if (hipMemcpyAsync(c->sob_acc, c->grad, sizeof(float) * (size_t)(c->P + 1), hipMemcpyDeviceToDevice, c->st) != hipSuccess) { rc = fail(NIF_ERR_HIP, "hipMemcpyAsync"); break; } }
      else launch_axpy_cols(c->sob_acc, c->grad, c->P, c->P, c->st);
    }
  }
  if (rc) return rc;
  if (ngroups > 1) HIPCHK(hipMemcpyAsync(c->grad, c->sob_acc, sizeof(float) * (size_t)(c->P + 1), hipMemcpyDeviceToDevice, c->st));
  c->grad_rewritten();
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_sobolev_loss_grad_dev_y(nif_ctx* c, const float* xin, const float* y, const float* dydx, const float* sw,
                                           int64_t B, int64_t Bg, const int32_t* x_idx, int32_t nx, const int32_t* y_idx, int32_t ny,
                                           float w_jac) {
  if (!c || !xin || !y || !dydx || B <= 0 || Bg < B) return fail(NIF_ERR_INVALID, "bad argument");
  unsigned ymask; int nys;
  const int rc = sobolev_check(c, x_idx, nx, y_idx, ny, &ymask, &nys); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  return sobolev_step(c, xin, y, dydx, sw, B, Bg, x_idx, nx, ymask, nys, w_jac);
}
extern "C" int nif_sobolev_loss_grad_dev(nif_ctx* c, const float* xin, const float* y, const float* dydx, const float* sw,
                                         int64_t B, int64_t Bg, const int32_t* x_idx, int32_t nx, float w_jac) {
  if (!c || !xin || !y || !dydx || B <= 0 || Bg < B) return fail(NIF_ERR_INVALID, "bad argument");
  unsigned ymask; int nys;
  const int rc = sobolev_check(c, x_idx, nx, nullptr, 0, &ymask, &nys); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  return sobolev_step(c, xin, y, dydx, sw, B, Bg, x_idx, nx, ymask, nys, w_jac);
}
// Second-order Sobolev step (HessianLayer as a trained output, gradient.py:130-180, :234-261): pass 0 is the first-order step above
// (u, du/dx and every regulariser), then one k_sob<.., HESS> pass per unordered coordinate pair j <= k with the primal and first-order
// terms off; the passes' [grad | loss] add up in sob2_acc
extern "C" int nif_sobolev2_loss_grad_dev(nif_ctx* c, const float* xin, const float* y, const float* dydx, const float* d2ydx2,
                                          const float* sw, int64_t B, int64_t Bg, const int32_t* x_idx, int32_t nx,
                                          const int32_t* y_idx, int32_t ny, float w_jac, float w_hess) {
  if (!c || !xin || !y || !dydx || !d2ydx2 || B <= 0 || Bg < B) return fail(NIF_ERR_INVALID, "bad argument");
  static const char* built = "built: NIFMultiScale (SIREN, with or without resblocks) and NIFMultiScaleLastLayerParameterized, "
                             "coordinate columns in x_index, policy float32";
  if (c->kind == NIF_KIND_NIF) return fail(NIF_ERR_INVALID, std::string("second-order Sobolev step: class NIF is not built (") + built + ")");
  if (c->cfg.mixed_policy != NIF_POLICY_FLOAT32)
    return fail(NIF_ERR_INVALID, std::string("second-order Sobolev step: mixed precision policies are not built (") + built + ")");
  unsigned ymask; int nys;
  int rc = sobolev_check(c, x_idx, nx, y_idx, ny, &ymask, &nys); if (rc) return rc;
  for (int d = 0; d < nx; ++d)
    if (x_idx[d] < c->pi)
      return fail(NIF_ERR_INVALID, std::string("second-order Sobolev step: parameter columns in x_index are not built (") + built + ")");
  if (c->capturing) return fail(NIF_ERR_STATE, "second-order Sobolev step inside a graph capture (not supported: run it uncaptured)");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  rc = sobolev_step(c, xin, y, dydx, sw, B, Bg, x_idx, nx, ymask, nys, w_jac); if (rc) return rc;
  if (!c->sob2_acc) { rc = c->sob2_acc.alloc(c->P + 1); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(c->sob2_acc, c->grad, sizeof(float) * (size_t)(c->P + 1), hipMemcpyDeviceToDevice, c->st));
  {
  const RegsOff regs_off(c, true);      // the regularisation losses belong to pass 0
  for (int j = 0; j < nx && !rc; ++j)
    for (int k = j; k < nx && !rc; ++k) {
      SobPlan sp;
      memset(&sp, 0, sizeof(sp));
      sp.ns = 3; sp.nsc = 3; sp.hess = 1;
      sp.seeds[0] = x_idx[j] - c->pi; sp.seeds[1] = x_idx[k] - c->pi; sp.seeds[2] = 0;
      for (int q = 0; q < 3; ++q) sp.par[q] = -1;
      sp.gcol[0] = j; sp.gcol[1] = k; sp.gcol[2] = 0;
      sp.gstride = nx; sp.nx_all = nx * nx; sp.ny = nys; sp.ymask = ymask; sp.no_primal = 1;
      rc = loss_grad_core(c, xin, y, sw, B, Bg, 3, sp.seeds, d2ydx2, w_hess, &sp);
      if (!rc) launch_axpy_cols(c->sob2_acc, c->grad, c->P, c->P, c->st);
    }
  }
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(c->grad, c->sob2_acc, sizeof(float) * (size_t)(c->P + 1), hipMemcpyDeviceToDevice, c->st));
  c->grad_rewritten();
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
static int sobolev_forward_group(nif_ctx* c, const float* xin, int64_t B, const SobPlan& sp, int nx, float* u, float* dudx);
extern "C" int nif_sobolev_forward_dev(nif_ctx* c, const float* xin, int64_t B, const int32_t* x_idx, int32_t nx, float* u,
                                       float* dudx) {
  if (!c || !xin || !u || !dudx || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  unsigned ymask; int nys;
  int rc = sobolev_check(c, x_idx, nx, nullptr, 0, &ymask, &nys); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  const int gs = sob_cols_per_pass(c, x_idx, nx);
  for (int g0 = 0; g0 < nx; g0 += gs) {      // groups of <= 3 columns, each filling its columns of the [B][so][nx] rows
    const int ng = nx - g0 < gs ? nx - g0 : gs;
    SobPlan sp;
    rc = sobolev_plan(c, x_idx + g0, ng, &sp); if (rc) return rc;
    for (int q = 0; q < 3; ++q) sp.gcol[q] += g0;
    sp.gstride = nx; sp.nx_all = nx;
    rc = sobolev_forward_group(c, xin, B, sp, ng, u, dudx); if (rc) return rc;
  }
  return NIF_OK;
}
static int sobolev_forward_group(nif_ctx* c, const float* xin, int64_t B, const SobPlan& sp, int nx, float* u, float* dudx) {
  int rc = ensure_packed(c); if (rc) return rc;
  rc = ensure_packed32(c); if (rc) return rc;
  if (c->kind != NIF_KIND_LASTLAYER && !c->jac_ok)
    return fail(NIF_ERR_INVALID, "Sobolev path: one weight plane and the small hyper-vectors of this shape exceed the 160 KB LDS of a CU");
  rc = ensure_capacity(c, B, false); if (rc) return rc;
  PNetArgs pa; fill_pnet(c, pa, xin, B);
  launch_pnet(pa, c->NSTB, false, c->st);
  SobPar spar = sob_par_of(sp);
  if (sp.any_par) {       // z' = dz/dp of the parameter columns
    rc = ensure_zt_par(c, pa, (B + 31) / 32, false); if (rc) return rc;
    spar.ZT = c->zt_par;
  }
  if (c->kind == NIF_KIND_LASTLAYER) {
    if (sp.any_par) {       // ... which are heads of the epilogue here
      spar.npar = sp.ns - sp.nsc;
      for (int e = 0; e < spar.npar; ++e) { spar.parc[e] = sp.par[sp.nsc + e]; spar.pcol[e] = sp.gcol[sp.nsc + e]; }
      for (int d = 0; d < 3; ++d) spar.par[d] = -1;
    }
    SNetArgs sl; rc = fill_snet_ll_sob(c, sl, xin, B); if (rc) return rc;
    sl.u_out = u;
    if (launch_sob(sl, false, sp.nsc, sp.seeds, nullptr, 0.f, nullptr, dudx, false, c->st, &spar) < 0)
      return fail(NIF_ERR_INVALID, "Sobolev path: the kernel's working set of this shape does not fit the 160 KB LDS of a CU");
    HIPCHK(hipGetLastError());
    return NIF_OK;
  }
  SNetArgs sa; fill_snet(c, sa, xin, c->pi + c->si, c->pi, B);
  sa.u_out = u;
  if (launch_sob(sa, false, nx, sp.seeds, nullptr, 0.f, nullptr, dudx, false, c->st, &spar) < 0)
    return fail(NIF_ERR_INVALID, "Sobolev path: the kernel's working set of this shape (units, latent_dim, parameter columns) does not fit the 160 KB LDS of a CU");
  HIPCHK(hipGetLastError());
  return NIF_OK;
}

// The term is marked as applied only when one was added: with no regulariser set, a read of the gradient (nif_grad_read) must not keep a
// regulariser that is set afterwards out of the update of the same gradient.  The term lands in grad[P] too: a loss-metric accumulation
// that waits for the next k_small launch takes the loss as it stood at its call, so it runs first.
static int apply_reg(nif_ctx* c) {
  if (c->reg_applied) return NIF_OK;
  const bool wreg = (c->reg_l1 != 0.f || c->reg_l2 != 0.f) && c->reg_hi > c->reg_lo;
  const bool sreg = (c->sreg_l1 != 0.f || c->sreg_l2 != 0.f) && c->kind == NIF_KIND_LASTLAYER;
  if (!wreg && !sreg) return NIF_OK;
  { const int rc = nif_metric_flush(c); if (rc) return rc; }
  if (wreg) launch_reg(c->theta, c->grad, c->reg_lo, c->reg_hi, c->P, c->reg_l1, c->reg_l2, c->st);
  if (sreg) launch_reg(c->theta, c->grad, c->s_first_w, c->ll_bias, c->P, c->sreg_l1, c->sreg_l2, c->st);
  c->reg_applied = true;
  return NIF_OK;
}
// cfg_shape_net["l1_reg" / "l2_reg"] of the last-layer class (nif/model.py:1028-1039, handed to every SIREN / SIREN_ResNet of the
// shared ShapeNet at :1168-1211; siren.py:266-269, :393-398 add them for kernels AND biases): theta[s_first_w, ll_bias) -- first,
// hidden and bottleneck layers, not last_layer_bias (BiasAddLayer has no regulariser, mlp.py:245-262)
extern "C" int nif_set_shapenet_regularizer(nif_ctx* c, float l1, float l2) {
  if (!c || l1 < 0.f || l2 < 0.f) return fail(NIF_ERR_INVALID, "bad argument");
  if ((l1 != 0.f || l2 != 0.f) && c->kind != NIF_KIND_LASTLAYER)
    return fail(NIF_ERR_INVALID, "ShapeNet weight regularisers exist for the last-layer-parameterised class only (the other classes' ShapeNet weights are ParameterNet outputs)");
  if (c->kind == NIF_KIND_LASTLAYER && !(c->s_first_w < c->ll_bias && c->ll_bias <= c->P)) return fail(NIF_ERR_STATE, "ShapeNet parameter range");
  c->sreg_l1 = l1; c->sreg_l2 = l2;
  return NIF_OK;
}
extern "C" int nif_set_regularizer(nif_ctx* c, float l1, float l2, int64_t lo, int64_t hi) {
  if (!c || lo < 0 || hi > c->P || lo > hi || l1 < 0.f || l2 < 0.f) return fail(NIF_ERR_INVALID, "bad argument");
  c->reg_l1 = l1; c->reg_l2 = l2; c->reg_lo = lo; c->reg_hi = hi;
  return NIF_OK;
}
// cfg_parameter_net["jac_reg"] (nif/model.py:353-375 -> JacRegLatentLayer, nif/layers/gradient.py:52-127)
extern "C" int nif_set_jac_regularizer(nif_ctx* c, float l1) {
  if (!c || l1 < 0.f) return fail(NIF_ERR_INVALID, "bad argument");
  if (l1 != 0.f) {
    PNetArgs pa; fill_pnet(c, pa, nullptr, 32);
    if (!pjac_supported(pa)) return fail(NIF_ERR_INVALID, "jac_reg: at most 3 parameter inputs (pi_dim <= 3)");
  }
  c->jac_l1 = l1;
  return NIF_OK;
}
// The regulariser's own pass, on top of the reduced main gradient: loss += l1 mean (dz/dp)^2 and its gradient w.r.t. the
// ParameterNet's first / hidden / bottleneck variables (the hyper layer is downstream of z and does not see it).
// mu_blk != null: the same pass as the adjoint of the Sobolev step's parameter streams -- dL/dz'_d is GIVEN (block mu_blk[d]
// of c->dzt_par, written by k_sob), no loss term
static int jac_reg_pass(nif_ctx* c, const float* xin, long B, long Bg, const int* mu_blk) {
  const int pi = c->pi, grp = pjac_group(), ndmax = pi < grp ? pi : grp;
  const long ntiles = (B + 31) / 32;
  int rc = ensure_capacity(c, ntiles * 32 * (1 + ndmax), true); if (rc) return rc;
  const long need_mu = (long)(1 + ndmax) * ntiles * 32 * c->r;
  rc = c->jac_mu.reserve(c, need_mu); if (rc) return rc;
  rc = ensure_jac_tmp(c); if (rc) return rc;
  const long nlp = (B + 127) / 128;
  rc = c->act_loss.reserve(c, nlp); if (rc) return rc;
  PNetArgs pa; fill_pnet(c, pa, xin, B);
  const float coef = c->jac_l1 / ((float)Bg * (float)c->r * (float)pi);
  // r4: passes over groups of parameter columns (k_pjac carries pjac_group() tangents): loss and gradient are sums over the
  // columns -- every pass reduces its own operand pairs (the primal pair carries the part of lambda that ITS tangents feed)
  for (int c0 = 0; c0 < pi; c0 += grp) {
    const int nd = pi - c0 < grp ? pi - c0 : grp;
    if (mu_blk) { bool any = false; for (int d = 0; d < nd; ++d) any = any || mu_blk[c0 + d] >= 0; if (!any) continue; }
    const int nloss = mu_blk ? launch_pjac_adj(pa, c->dzt_par, mu_blk, c->jac_mu, c->act_loss, c0, nd, c->st)
                             : launch_pjac(pa, coef, c->jac_mu, c->act_loss, c0, nd, c->st);
    GwArgs base = gw_base(c, ntiles, B, c->partial);
    const int cols[3] = {c0, c0 + 1, c0 + 2};
    gw_add_tangents(base, nd, cols);
    const int rows = rows_for(c, base.ntiles);
    gw_pnet_stack(c, base, xin, c->stash_p, c->jac_mu, pa.omega, rows, c->st);
    // the ParameterNet core variables are the first last_w columns of a partial row; column last_w of the result = the loss term
    launch_reduce(c->partial, c->pstride, rows, c->act_loss, nloss, c->jac_tmp, c->last_w, c->st);
    launch_axpy_cols(c->grad, c->jac_tmp, c->last_w, c->P, c->st);
  }
  HIPCHK(hipGetLastError());
  return NIF_OK;
}

// Sobolev step with parameter seeds, the part the main reductions do not see (k_sob_dev.h, PAR).  For a parameter stream d:
//   dL/dM^(k) += w0 sum_p zt'_k h_in nu_d^T , dL/db^(k) += sum_p zt'_k nu_d  (k < r): the SAME reductions as the main step with
//   (h_in, nu_d) as the operand pair and zt' = dz/dp in the latent's place.  They run after the main row reduction, into the
//   same partial rows; only the hyper KERNEL columns are kept (the kernels also fill the constant plane = hyper bias columns
//   with sum h_in nu^T, which zt'_r = 0 excludes).  Then the ParameterNet side: the adjoint of (z, z') for the dL/dz' that
//   k_sob left in c->dzt_par (jac_reg_pass with given mu).
static int sob_par_pass(nif_ctx* c, const float* xin, long B, long Bg, const SobPlan& sp, const SNetArgs& sa) {
  const long ntiles = (B + 31) / 32;
  const int rows = rows_for(c, ntiles);
  { const int rca = ensure_jac_tmp(c); if (rca) return rca; }
  const long kcols = (long)c->r * c->po;                     // the hyper kernel [r][po] = columns last_w .. last_w + r*po
  GwArgs base = gw_base(c, ntiles, B, c->partial);
  gw_add_tangents(base, 0, nullptr);                         // (one block of tiles per launch, Z by tile as in the main step)
  MuBlk mu;
  for (int d = sp.nsc; d < sp.ns; ++d) {
    const int col = sp.par[d];
    mu.blk[col] = d;
    const float* ZTd = c->zt_par + (long)col * ntiles * 32 * c->r;
    if (gw_hyper_snet_stack(c, base, sa, xin, ZTd, 1 + d, ntiles, false, false, rows, c->st) < 0)
      return fail(NIF_ERR_STATE, "internal: bf16 dL/da stash rows without a reader of that form");
    launch_reduce(c->partial + c->last_w, c->pstride, rows, nullptr, 0, c->jac_tmp, kcols, c->st);
    launch_axpy_cols(c->grad + c->last_w, c->jac_tmp, kcols, c->P - c->last_w, c->st);
  }
  HIPCHK(hipGetLastError());
  return jac_reg_pass(c, xin, B, Bg, mu.blk);
}

// compile(loss=...) of the Keras surface (README.md:33 'mse'): the per-element loss of every training / evaluation entry point of this
// context -- 0 'mse', 1 'mae', 2 'huber' (delta 1), 3 'log_cosh' (include/nif_hip.h nif_loss); the Sobolev step applies it to both outputs
extern "C" int nif_set_loss(nif_ctx* c, int32_t kind) {
  if (!c || kind < 0 || kind > 3) return fail(NIF_ERR_INVALID, "nif_set_loss: 0 mse, 1 mae, 2 huber, 3 log_cosh");
  c->loss_kind = kind;
  return NIF_OK;
}
// Keras activity_regularizer of the last ParameterNet layer (nif/model.py:118-125, :226, :659, :731)
extern "C" int nif_set_activity_regularizer(nif_ctx* c, float l1, float l2) {
  if (!c || l1 < 0.f || l2 < 0.f) return fail(NIF_ERR_INVALID, "bad argument");
  if ((l1 != 0.f || l2 != 0.f) && c->kind != NIF_KIND_LASTLAYER && c->r > actreg_max_r()) return fail(NIF_ERR_INVALID, "activity regularisers: latent_dim <= 64");
  c->act_l1 = l2 != 0.f ? 0.f : l1; c->act_l2 = l2;
  return NIF_OK;
}
static int ensure_metric(nif_ctx* c) {
  if (c->metric) return NIF_OK;
  DevBuf<double> m;
  const int rc = m.alloc(2); if (rc) return rc;
  HIPCHK(hipMemsetAsync(m, 0, 2 * sizeof(double), c->st));
  c->metric = std::move(m);
  return NIF_OK;
}
extern "C" int nif_metric_accumulate(nif_ctx* c, float weight) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_METRIC)      // (an earlier accumulation that still waits: first, with the loss it was called for)
  { const int rcm = ensure_metric(c); if (rcm) return rcm; }
  if (c->last_step_small && c->opt_small_step && !c->capturing && !c->comm) {     // behind a small step: rides in the next k_small launch (grad[P] is not
    c->metric_pending = true; c->metric_pending_w = weight;          // touched before that launch's row reduction; every other path flushes)
    return NIF_OK;
  }
  launch_metric(c->grad, c->P, weight, c->metric, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_metric_read(nif_ctx* c, double* sum, double* cnt, int reset) {
  if (!c || !sum || !cnt) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_METRIC)
  double h[2] = {0.0, 0.0};
  if (c->metric) {
    HIPCHK(hipMemcpyAsync(h, c->metric, 2 * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if (reset) HIPCHK(hipMemsetAsync(c->metric, 0, 2 * sizeof(double), c->st));
  }
  *sum = h[0]; *cnt = h[1];
  return NIF_OK;
}
// ---- captured training steps ----------------------------------------------------------------------------------------------------
// Small batches are launch bound (configs[0]: 13 kernels of 3-5 us behind 4-8 us of launch overhead each): between nif_graph_begin
// and nif_graph_end every device-side call of this context (nif_loss_grad_dev, nif_sobolev_loss_grad_dev[_y], nif_adam_step_dev,
// nif_metric_accumulate, nif_gather_rows_dev ...) is RECORDED into a hipGraph instead of executed; nif_graph_launch replays the
// whole sequence -- an epoch of Model.fit -- with one submission.  The batch pointers are baked in (the resident table does not
// move between epochs); the optimizer's hyper-parameters and iteration count live in device memory (OptDev) and are refreshed per launch.
// Everything a step needs must exist before the capture (nif_reserve): a workspace that would have to grow fails the capture.
extern "C" int nif_graph_begin(nif_ctx* c) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  if (c->capturing) return fail(NIF_ERR_STATE, "nif_graph_begin: already capturing");
  if (c->comm) return fail(NIF_ERR_STATE, "nif_graph_begin: not with a communicator attached (the all-reduce is not captured)");
  NIF_ENTER(c, NIF_FLUSH_METRIC)
  c->last_step_small = false;
  int rc = ensure_packed(c); if (rc) return rc;
  if (c->kind != NIF_KIND_LASTLAYER) {      // (a captured small step must find its tables)
    PNetArgs pa; fill_pnet(c, pa, nullptr, 32);
    SNetArgs sa; fill_snet(c, sa, nullptr, c->pi + c->si, c->pi, 32);
    if (small_supported(pa, sa)) { rc = ensure_small_tables(c, pa, sa); if (rc) return rc; }
  }
  { const int rcm = ensure_metric(c); if (rcm) return rcm; }
  if (!c->opt_dev) { rc = c->opt_dev.alloc(1); if (rc) return rc; }
  if (!c->opt_host) { rc = c->opt_host.alloc(1); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(c->st));
  // (ensure_packed above did every first-use initialisation eagerly; the RECORDED sequence must start with the packing of whatever
  // weights the previous replay left behind)
  c->planes_stale();
  HIPCHK(hipStreamBeginCapture(c->st, hipStreamCaptureModeRelaxed));
  c->capturing = true; c->rec = CapInfo(); c->rec.step0 = c->step;
  return NIF_OK;
}
extern "C" int nif_graph_end(nif_ctx* c, int32_t* graph_id) {
  if (!c || !graph_id) return fail(NIF_ERR_INVALID, "null");
  if (!c->capturing) return fail(NIF_ERR_STATE, "nif_graph_end without nif_graph_begin");
  NIF_ENTER(c, NIF_FLUSH_NONE)             // (nothing defers inside a capture, and nothing recorded has run)
  c->capturing = false;
  c->last_step_small = false;              // (set by the RECORDED small steps: no eager one ran, the next nif_metric_accumulate must not wait for a k_small launch)
  c->step = c->rec.step0;                  // nothing has run yet: the recorded steps count when the graph is launched
  c->planes_stale();
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(c->st, &g);
  if (e != hipSuccess || !g) { (void)hipGetLastError(); return fail(NIF_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e)); }
  hipGraphExec_t ex = nullptr;
  e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(NIF_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); }
  c->rec.step0 = 0;      // (the running capture's alone)
  c->graphs.push_back({ex, c->rec});
  *graph_id = (int32_t)c->graphs.size() - 1;
  return NIF_OK;
}
extern "C" int nif_graph_destroy(nif_ctx* c, int32_t graph_id) {
  if (!c || graph_id < 0 || graph_id >= (int32_t)c->graphs.size()) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_NONE)      // (drops an executable: reads nothing a deferred piece would change)
  hipGraphExec_t& ex = c->graphs[graph_id].exec;
  if (ex) { HIPCHK(hipStreamSynchronize(c->st)); (void)hipGraphExecDestroy(ex); ex = nullptr; }
  return NIF_OK;
}

// ---- gradient transform (include/nif_hip.h nif_set_grad_transform; k_gradtf.hip; reference nif/optimizers/gtcf.py:7-67) -------------
static int gt_check(const nif_grad_transform* t) {
  if (t->flags & ~(NIF_GT_CENTRALIZE | NIF_GT_GTCF)) return fail(NIF_ERR_INVALID, "nif_grad_transform: unknown flag bits");
  if (t->reserved[0] || t->reserved[1] || t->reserved[2] || t->reserved[3]) return fail(NIF_ERR_INVALID, "nif_grad_transform: reserved fields must be zero");
  if (!(t->clipnorm >= 0.f) || !(t->clipvalue >= 0.f) || !(t->global_clipnorm >= 0.f))
    return fail(NIF_ERR_INVALID, "nif_grad_transform: clipnorm, clipvalue and global_clipnorm must be >= 0 (0 = off)");
  const int n = (t->clipnorm > 0.f) + (t->clipvalue > 0.f) + (t->global_clipnorm > 0.f);
  if (!(t->flags & NIF_GT_GTCF) && n > 1)
    return fail(NIF_ERR_INVALID, "nif_grad_transform: only one of clipnorm, clipvalue and global_clipnorm (Keras route; NIF_GT_GTCF takes clipnorm and clipvalue)");
  if ((t->flags & NIF_GT_GTCF) && t->global_clipnorm > 0.f)
    return fail(NIF_ERR_INVALID, "nif_grad_transform: NIF_GT_GTCF has no global_clipnorm (its clipnorm is the global norm)");
  return NIF_OK;
}
// the work blocks of the layout: 64 columns x all rows of a matrix, chunks of GT_VEC_CHUNK floats of a vector
static std::vector<GtBlk> gt_blocks(const nif_ctx* c) {
  std::vector<GtBlk> v;
  for (size_t t = 0; t < c->layout.size(); ++t) {
    const nif_tensor_desc& d = c->layout[t];
    const int pb0 = (int)v.size();
    GtBlk b; memset(&b, 0, sizeof(b));
    b.tensor = (int)t; b.pb0 = pb0;
    if (d.cols > 0) {
      for (int c0 = 0; c0 < d.cols; c0 += 64) {
        b.matrix = 1; b.base = (long)d.offset + c0; b.stride = d.cols; b.rows = d.rows; b.nc = d.cols - c0 < 64 ? d.cols - c0 : 64;
        b.lim = (long)(d.rows - 1) * d.cols + b.nc;
        v.push_back(b);
      }
    } else {
      for (long e0 = 0; e0 < d.rows; e0 += GT_VEC_CHUNK) {
        const long len = d.rows - e0 < GT_VEC_CHUNK ? d.rows - e0 : GT_VEC_CHUNK;
        b.matrix = 0; b.base = (long)d.offset + e0; b.stride = 64; b.rows = (int)((len + 63) / 64); b.nc = 64; b.lim = len;
        v.push_back(b);
      }
    }
    for (size_t i = (size_t)pb0; i < v.size(); ++i) v[i].pbn = (int)v.size() - pb0;
  }
  return v;
}
static int gt_launches(const nif_ctx* c) { return c->gt_on ? (c->gt_norm ? 2 : 1) : 0; }
extern "C" int nif_set_grad_transform(nif_ctx* c, const nif_grad_transform* t) {
  nif_grad_transform z; memset(&z, 0, sizeof(z));
  if (t) { const int rc = gt_check(t); if (rc) return rc; z = *t; }      // (the struct is judged first: checkable without a device)
  if (!c) return fail(NIF_ERR_INVALID, "nif_set_grad_transform: null context");
  if (c->capturing) return fail(NIF_ERR_STATE, "nif_set_grad_transform: not inside a graph capture");
  const bool gtcf = (z.flags & NIF_GT_GTCF) != 0;
  const bool on = (z.flags & NIF_GT_CENTRALIZE) || z.clipnorm > 0.f || z.clipvalue > 0.f || z.global_clipnorm > 0.f;
  if (!on && !c->gt_dev) { c->gt = z; c->gt_on = false; c->gt_norm = false; return NIF_OK; }
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));      // (queued steps still read the device copy)
  GtDev d; d.flags = z.flags; d.clipnorm = z.clipnorm; d.clipvalue = z.clipvalue; d.global_clipnorm = z.global_clipnorm;
  if (!c->gt_dev) {
    const std::vector<GtBlk> blks = gt_blocks(c);
    for (const GtBlk& b : blks)
      if (b.base < 0 || b.base + b.lim > c->P) return fail(NIF_ERR_STATE, "internal: gradient-transform block outside the gradient");
    // gt_dev != null says that all four exist and the block table is filled: they join the context together, after the last step that can fail
    DevBuf<GtBlk> blk; DevBuf<float> part, norms; DevBuf<GtDev> dev;
    int rc = blk.alloc((long)blks.size()); if (rc) return rc;
    rc = part.alloc((long)blks.size()); if (rc) return rc;
    rc = norms.alloc((long)c->layout.size() + 1); if (rc) return rc;
    rc = dev.alloc(1); if (rc) return rc;
    HIPCHK(hipMemcpy(blk, blks.data(), sizeof(GtBlk) * blks.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dev, &d, sizeof(d), hipMemcpyHostToDevice));
    c->gt_blk = std::move(blk); c->gt_part = std::move(part); c->gt_norms = std::move(norms); c->gt_dev = std::move(dev);
    c->gt_nblk = (int)blks.size();
  } else HIPCHK(hipMemcpy(c->gt_dev, &d, sizeof(d), hipMemcpyHostToDevice));
  c->gt = z; c->gt_on = on;
  c->gt_norm = on && (gtcf ? z.clipnorm > 0.f : (z.clipnorm > 0.f || z.global_clipnorm > 0.f));
  return NIF_OK;
}
// the configured transform on c->grad (complete: reduced, all-reduced, regulariser added); one launch, two with a norm stage
static void gt_run(nif_ctx* c) {
  launch_gt_reduce(c->grad, c->gt_blk, c->gt_nblk, c->gt_part, c->gt_dev, c->st);
  if (c->gt_norm) launch_gt_apply(c->grad, c->gt_blk, c->gt_nblk, (int)c->layout.size(), c->gt_part, c->gt_norms, c->gt_dev, true, c->st);
  if (c->capturing) c->rec.gt = gt_launches(c);      // (nothing has run yet: graph_replay marks the norms)
  else c->gt_ran = c->gt_norm ? 2 : 1;
}
extern "C" int nif_grad_transform_dev(nif_ctx* c) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  { const int rcr_ = apply_reg(c); if (rcr_) return rcr_; }
  if (c->gt_on) gt_run(c);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_grad_norms(nif_ctx* c, float* per_tensor, int32_t n, float* global) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  if (per_tensor && n != (int32_t)c->layout.size()) return fail(NIF_ERR_INVALID, "nif_grad_norms: n is the tensor count of nif_param_layout");
  if (c->capturing) return fail(NIF_ERR_STATE, "nif_grad_norms: not inside a graph capture");
  if (!c->gt_ran) return fail(NIF_ERR_STATE, "nif_grad_norms: no gradient transform has run on this context");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  if (c->gt_ran == 1) {      // the last transform had no norm stage: its partial sums are there, the norms are formed now
    launch_gt_apply(c->grad, c->gt_blk, c->gt_nblk, (int)c->layout.size(), c->gt_part, c->gt_norms, c->gt_dev, false, c->st);
    HIPCHK(hipGetLastError());
    c->gt_ran = 2;
  }
  if (per_tensor) HIPCHK(hipMemcpyAsync(per_tensor, c->gt_norms, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->st));
  if (global) HIPCHK(hipMemcpyAsync(global, c->gt_norms + c->layout.size(), sizeof(float), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

// ---- optimizer steps (include/nif_hip.h nif_adam_step_dev, nif_opt_step_dev; reference nif/optimizers/external_optimizers.py:322-735) ----
static int opt_check(const nif_opt* o) {
  if (o->kind < NIF_OPT_ADAM || o->kind > NIF_OPT_ADAMAX)
    return fail(NIF_ERR_INVALID, "nif_opt: kind must be NIF_OPT_ADAM, _LION, _ADABELIEF, _SGD, _RMSPROP, _ADAGRAD or _ADAMAX");
  const int allowed = o->kind == NIF_OPT_ADAM ? (NIF_OPT_AMSGRAD | NIF_OPT_DECOUPLED_WD) : o->kind == NIF_OPT_ADABELIEF ? (NIF_OPT_RECTIFY | NIF_OPT_AMSGRAD)
                    : o->kind == NIF_OPT_SGD ? NIF_OPT_NESTEROV : o->kind == NIF_OPT_RMSPROP ? NIF_OPT_CENTERED : 0;
  if (o->flags & ~(NIF_OPT_RECTIFY | NIF_OPT_AMSGRAD | NIF_OPT_NESTEROV | NIF_OPT_CENTERED | NIF_OPT_DECOUPLED_WD))
    return fail(NIF_ERR_INVALID, "nif_opt: unknown flag bits");
  if (o->flags & ~allowed)
    return fail(NIF_ERR_INVALID, "nif_opt: a flag of another kind (RECTIFY: AdaBelief; AMSGRAD: AdaBelief, Adam; NESTEROV: SGD; CENTERED: RMSprop; DECOUPLED_WD: Adam)");
  if (o->kind != NIF_OPT_ADABELIEF && (o->total_steps || o->sma_threshold != 0.f || o->warmup_proportion != 0.f || o->min_lr != 0.f))
    return fail(NIF_ERR_INVALID, "nif_opt: flags, sma_threshold, total_steps, warmup_proportion and min_lr are AdaBelief's");
  if (o->kind == NIF_OPT_ADAM && (o->decay != 0.f || (o->weight_decay != 0.f && !(o->flags & NIF_OPT_DECOUPLED_WD))))
    return fail(NIF_ERR_INVALID, "nif_opt: Adam has no decay / weight_decay on this path (nif_adam); weight_decay needs NIF_OPT_DECOUPLED_WD");
  if (o->kind >= NIF_OPT_SGD && (o->decay != 0.f || o->weight_decay != 0.f))
    return fail(NIF_ERR_INVALID, "nif_opt: SGD, RMSprop, Adagrad and Adamax have no decay / weight_decay");
  if (o->kind == NIF_OPT_SGD && (o->beta2 != 0.f || o->eps != 0.f || !(o->beta1 >= 0.f && o->beta1 <= 1.f)))
    return fail(NIF_ERR_INVALID, "nif_opt: SGD takes momentum in beta1, within [0, 1]; beta2 and eps must be zero");
  if (o->kind == NIF_OPT_RMSPROP && !(o->beta1 >= 0.f && o->beta1 <= 1.f))
    return fail(NIF_ERR_INVALID, "nif_opt: RMSprop takes momentum in beta1, within [0, 1]");
  if (o->kind == NIF_OPT_ADAGRAD ? !(o->init_acc >= 0.f) : o->init_acc != 0.f)
    return fail(NIF_ERR_INVALID, "nif_opt: init_acc is Adagrad's, >= 0");
  if (o->total_steps < 0) return fail(NIF_ERR_INVALID, "nif_opt: total_steps < 0");
  const int sk = o->sched & 0xff, sf = o->sched & ~0xff;
  if (sk > NIF_SCHED_POLYNOMIAL || o->sched < 0 || (sf & ~(NIF_SCHED_STAIRCASE | NIF_SCHED_CYCLE)))
    return fail(NIF_ERR_INVALID, "nif_opt: sched must be a NIF_SCHED_* kind with NIF_SCHED_STAIRCASE / NIF_SCHED_CYCLE");
  if ((sf & NIF_SCHED_STAIRCASE) && sk != NIF_SCHED_EXPONENTIAL && sk != NIF_SCHED_INVERSE_TIME)
    return fail(NIF_ERR_INVALID, "nif_opt: NIF_SCHED_STAIRCASE is ExponentialDecay's and InverseTimeDecay's");
  if ((sf & NIF_SCHED_CYCLE) && sk != NIF_SCHED_POLYNOMIAL) return fail(NIF_ERR_INVALID, "nif_opt: NIF_SCHED_CYCLE is PolynomialDecay's");
  if (sk == NIF_SCHED_NONE && (sf || o->decay_steps || o->sched_a != 0.f || o->sched_b != 0.f))
    return fail(NIF_ERR_INVALID, "nif_opt: decay_steps, sched_a and sched_b must be zero without a schedule");
  if (sk != NIF_SCHED_NONE && o->decay_steps <= 0) return fail(NIF_ERR_INVALID, "nif_opt: a schedule needs decay_steps > 0");
  if (sk != NIF_SCHED_NONE && o->decay != 0.f) return fail(NIF_ERR_INVALID, "nif_opt: the legacy decay and a schedule exclude each other");
  if (sk != NIF_SCHED_POLYNOMIAL && o->sched_b != 0.f) return fail(NIF_ERR_INVALID, "nif_opt: sched_b is PolynomialDecay's power");
  return NIF_OK;
}
// c: the context whose weight-averaging state the step reads (null: none, nif_opt_scalars)
static OptDev opt_dev_of(const nif_ctx* c, const nif_opt* o, long step) {
  OptDev d;
  d.ema_mom = c ? c->ema_mom : 0.f; d.ema_freq = c && c->opt_ema > 0 ? c->opt_ema : 0;
  d.kind = o->kind; d.flags = o->flags; d.lr = o->lr; d.beta1 = o->beta1; d.beta2 = o->beta2; d.eps = o->eps; d.wd = o->weight_decay;
  d.decay = o->decay; d.sma_threshold = o->sma_threshold; d.warmup_proportion = o->warmup_proportion; d.min_lr = o->min_lr;
  d.total_steps = (long)o->total_steps; d.step = step;
  d.sched = o->sched; d.decay_steps = o->decay_steps; d.sched_a = o->sched_a; d.sched_b = o->sched_b;
  return d;
}
// the kernel instantiation of a nif_opt and whether it uses the third slot: what a captured graph is tied to
static int opt_kk(const nif_opt* o) { return kernel_kind(o->kind, o->flags); }
static bool opt_ams(const nif_opt* o) { return third_slot(o->kind, o->flags); }
// Adagrad's accumulator starts at initial_accumulator_value: written when the kind first runs on fresh slots (not part of a capture:
// a replay would write it again)
static int adagrad_fill(nif_ctx* c, float value) {
  if (c->capturing) return fail(NIF_ERR_STATE, "Adagrad's accumulator is not initialised yet: run one eager step or nif_set_opt_state before the capture");
  const std::vector<float> acc((size_t)c->P, value);
  HIPCHK(hipMemcpyAsync(c->m, acc.data(), sizeof(float) * (size_t)c->P, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}
static int ensure_vhat(nif_ctx* c) {
  if (c->vhat) return NIF_OK;
  if (c->capturing) return fail(NIF_ERR_STATE, "the third slot (AMSGrad's vhat, centered RMSprop's a) does not exist yet: run one eager step or nif_set_opt_slot(2, ...) before the capture");
  DevBuf<float> vh;
  const int rc = vh.alloc(c->P); if (rc) return rc;
  HIPCHK(hipMemsetAsync(vh, 0, sizeof(float) * (size_t)c->P, c->st));
  c->vhat = std::move(vh);
  return NIF_OK;
}
// the weight average (slot 3) exists and holds values.  seed: it starts as a device copy of theta as it stands (Keras creates the
// average with the variable's value); else the caller fills it (nif_set_opt_slot)
static int ensure_ema(nif_ctx* c, bool seed) {
  if (c->ema && c->ema_valid) return NIF_OK;
  if (c->capturing) return fail(NIF_ERR_STATE, "the weight average (slot 3) does not exist yet: run one eager step or nif_set_opt_slot(3, ...) before the capture");
  if (!c->ema) {
    DevBuf<float> av;
    const int rc = av.alloc(c->P); if (rc) return rc;
    c->ema = std::move(av);
  }
  if (seed) HIPCHK(hipMemcpyAsync(c->ema, c->theta, sizeof(float) * (size_t)c->P, hipMemcpyDeviceToDevice, c->st));
  c->ema_valid = true;
  return NIF_OK;
}
extern "C" int nif_opt_scalars(const nif_opt* o, int64_t t, double* out) {
  if (!o || !out || t < 1) return fail(NIF_ERR_INVALID, "bad argument");
  const int rc = opt_check(o); if (rc) return rc;
  const OptScalars s = opt_scalars(opt_dev_of(nullptr, o, 0), (long)t);
  out[0] = s.lr; out[1] = s.bc1; out[2] = s.bc2; out[3] = s.r; out[4] = (double)s.div;
  return NIF_OK;
}
// One optimizer step of any kind, after the all-reduce, in one of three forms: fused with the deferred row reduction (tail_can_defer,
// no gradient transform set);
// inside a capture with the scalars from c->opt_dev at replay time (graph_replay refreshes it); else after the flushed reduction and the
// regulariser term.  `who` names the entry point in the error messages.  Its epilogue (nif_ctx::theta_stepped): the packed weight planes
// are stale, and the regulariser term belongs to ONE gradient -- a following step that skips nif_loss_grad_dev (nif_zero_grad on a rank
// whose shard ran out of rows) must add it again, like the ranks that did compute a gradient
static int opt_step(nif_ctx* c, const nif_opt* opt, const char* who) {
  if (!c->have_params) return fail(NIF_ERR_STATE, "parameters not set");
  const bool ams = opt_ams(opt);
  const int kk = opt_kk(opt);
  const bool ema = c->opt_ema != 0;
  if (c->capturing && c->rec.kind >= 0 && (c->rec.kind != kk || c->rec.ams != ams))
    return fail(NIF_ERR_STATE, std::string(who) + ": this capture already holds steps of another optimizer kind / amsgrad flag (one per graph)");
  if (c->capturing && c->rec.kind >= 0 && c->rec.ema != ema)
    return fail(NIF_ERR_STATE, std::string(who) + ": this capture already holds steps recorded with weight averaging (\"ema\") " + (c->rec.ema ? "on" : "off") + " (one setting per graph)");
  if (ams) { const int rc = ensure_vhat(c); if (rc) return rc; }
  if (ema) { const int rc = ensure_ema(c, true); if (rc) return rc; }      // (seeded with theta before this step's update)
  if (opt->kind == NIF_OPT_ADAGRAD && c->slots_fresh && opt->init_acc != 0.f) { const int rc = adagrad_fill(c, opt->init_acc); if (rc) return rc; }
  c->slots_fresh = false;
  // the step's row reduction and the update in ONE launch -- not with a gradient transform set: a norm needs every column of the
  // gradient before any parameter moves
  const bool fused = c->tail_pending && !c->capturing && !c->gt_on && tail_can_defer(c);
  if (fused) {
    c->tail_pending = false;
  } else {
    { const int rct_ = nif_tail_flush(c); if (rct_) return rct_; }
    { const int rcr_ = apply_reg(c); if (rcr_) return rcr_; }
    if (c->gt_on) gt_run(c);
  }
  c->step += 1;
  const OptDev d = opt_dev_of(c, opt, c->step - 1);
  OptArgs a = opt_args(d, opt_scalars(d, c->step));
  a.ema_ow = ema && ema_overwrite(c->step, d.ema_freq) ? 1 : 0;
  float* const av = ema ? (float*)c->ema : nullptr;
  if (fused) {
    launch_reduce_opt(kk, ams, c->partial, c->pstride, c->tail_rows, c->loss_partial, c->tail_nloss, c->grad, c->P, c->theta, c->m,
                      c->v, c->vhat, av, a, c->st);
  } else if (c->capturing) {
    launch_opt_dev(kk, ams, c->theta, c->grad, c->m, c->v, c->vhat, av, c->P, c->opt_dev, c->st);
    c->rec.steps += 1; c->rec.kind = kk; c->rec.ams = ams; c->rec.ema = ema;
  } else {
    ProfScope p_(c, NIF_PROF_ADAM);
    launch_opt(kk, ams, c->theta, c->grad, c->m, c->v, c->vhat, av, c->P, a, c->st);
  }
  HIPCHK(hipGetLastError());
  c->theta_stepped();
  return NIF_OK;
}
static nif_opt opt_of_adam(const nif_adam* a) {
  nif_opt o = {};
  o.kind = NIF_OPT_ADAM; o.lr = a->lr; o.beta1 = a->beta1; o.beta2 = a->beta2; o.eps = a->eps;
  return o;
}
extern "C" int nif_adam_step_dev(nif_ctx* c, const nif_adam* opt) {
  if (!c || !opt) return fail(NIF_ERR_INVALID, "null");
  const nif_opt o = opt_of_adam(opt);
  NIF_ENTER(c, NIF_FLUSH_NONE)      // (the step consumes the tail itself: fused with the update where it can, opt_step)
  return opt_step(c, &o, "nif_adam_step_dev");
}
extern "C" int nif_opt_step_dev(nif_ctx* c, const nif_opt* opt) {
  if (!c || !opt) return fail(NIF_ERR_INVALID, "null");
  const int rc = opt_check(opt); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_NONE)      // (as nif_adam_step_dev)
  return opt_step(c, opt, "nif_opt_step_dev");
}
// what a replay of a graph is refused for by the context's state (the caller has checked the optimizer against g.kind / g.ams)
static int graph_replay_refused(const nif_ctx* c, const CapInfo& g, const char* who) {
  if (c->capturing) return fail(NIF_ERR_STATE, std::string(who) + " while capturing");
  if (gt_launches(c) > g.gt)
    return fail(NIF_ERR_STATE, std::string(who) + ": the context's gradient transform needs launches this graph did not record (set it before the capture)");
  const bool ema = c->opt_ema != 0;
  if (g.kind >= 0 && g.ema != ema)
    return fail(NIF_ERR_STATE, std::string(who) + ": the graph was recorded with weight averaging (\"ema\") " + (g.ema ? "on" : "off") + ", the context has it " + (ema ? "on" : "off") + " (set it before the capture)");
  return NIF_OK;
}
// replays a captured graph with opt's hyper-parameters and the context's iteration count, behind graph_replay_refused and the guard (the
// replay overwrites grad[P]: a deferred accumulation has taken the loss of the step it was called for)
static int graph_replay(nif_ctx* c, const CapGraph& g, const nif_opt* opt) {
  if (c->opt_ema != 0 && g.info.kind >= 0) { const int rce = ensure_ema(c, true); if (rce) return rce; }      // (reset by nif_set_opt_state since the capture: seeded again, at the recorded address)
  HIPCHK(hipStreamSynchronize(c->st));      // (the pinned staging struct is reused: the previous launch's copy must be through)
  *c->opt_host = opt_dev_of(c, opt, c->step);
  HIPCHK(hipMemcpyAsync(c->opt_dev, c->opt_host, sizeof(OptDev), hipMemcpyHostToDevice, c->st));
  HIPCHK(hipGraphLaunch(g.exec, c->st));
  c->step += g.info.steps;
  if (g.info.gt) c->gt_ran = g.info.gt;
  c->theta_stepped();
  return NIF_OK;
}
static bool graph_ok(const nif_ctx* c, int32_t graph_id) { return graph_id >= 0 && graph_id < (int32_t)c->graphs.size() && c->graphs[graph_id].exec; }
extern "C" int nif_graph_launch(nif_ctx* c, int32_t graph_id, const nif_adam* opt) {
  if (!c || !opt || !graph_ok(c, graph_id)) return fail(NIF_ERR_INVALID, "bad argument");
  const CapGraph& g = c->graphs[graph_id];
  if (g.info.kind > OPT_ADAM || g.info.ams)
    return fail(NIF_ERR_STATE, "nif_graph_launch: the graph holds Lion / AdaBelief steps or those of another nif_opt kind (nif_graph_launch_opt with that optimizer)");
  const nif_opt o = opt_of_adam(opt);
  const int rc = graph_replay_refused(c, g.info, "nif_graph_launch"); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_METRIC)
  return graph_replay(c, g, &o);
}
extern "C" int nif_graph_launch_opt(nif_ctx* c, int32_t graph_id, const nif_opt* opt) {
  if (!c || !opt || !graph_ok(c, graph_id)) return fail(NIF_ERR_INVALID, "bad argument");
  int rc = opt_check(opt); if (rc) return rc;
  const CapGraph& g = c->graphs[graph_id];
  if (g.info.kind >= 0 && (g.info.kind != opt_kk(opt) || g.info.ams != opt_ams(opt)))
    return fail(NIF_ERR_INVALID, "nif_graph_launch_opt: the graph was recorded with another optimizer kind / amsgrad flag (or centered / decoupled weight decay flag)");
  rc = graph_replay_refused(c, g.info, "nif_graph_launch_opt"); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_METRIC)
  return graph_replay(c, g, opt);
}
extern "C" int nif_get_opt_slot(nif_ctx* c, int32_t slot, float* host, int64_t n) {
  if (!c || !host || slot < 0 || slot > 3) return fail(NIF_ERR_INVALID, "bad argument (slot: 0 m, 1 v, 2 vhat, 3 weight average)");
  if (n != c->P) return fail(NIF_ERR_INVALID, "parameter count mismatch");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  float* src = slot == 0 ? c->m : slot == 1 ? c->v : slot == 2 ? c->vhat : c->ema;
  if (slot == 3 && !c->ema_valid) src = nullptr;      // (reset by nif_set_opt_state: zeros until the next step seeds it)
  if (!src) { memset(host, 0, sizeof(float) * (size_t)n); return NIF_OK; }
  HIPCHK(hipMemcpyAsync(host, src, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}
extern "C" int nif_set_opt_slot(nif_ctx* c, int32_t slot, const float* host, int64_t n) {
  if (!c || !host || slot < 0 || slot > 3) return fail(NIF_ERR_INVALID, "bad argument (slot: 0 m, 1 v, 2 vhat, 3 weight average)");
  if (n != c->P) return fail(NIF_ERR_INVALID, "parameter count mismatch");
  if (c->capturing) return fail(NIF_ERR_STATE, "nif_set_opt_slot while capturing");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  if (slot == 2) { const int rc = ensure_vhat(c); if (rc) return rc; }
  if (slot == 3) { const int rc = ensure_ema(c, false); if (rc) return rc; }
  float* dst = slot == 0 ? c->m : slot == 1 ? c->v : slot == 2 ? c->vhat : c->ema;
  HIPCHK(hipMemcpyAsync(dst, host, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  if (slot != 3) c->slots_fresh = false;      // (the average is no slot of a kind: Adagrad's accumulator is still to be written)
  return NIF_OK;
}

// ---- low-magnitude pruning (include/nif_hip.h nif_prune_*; k_prune.hip) -----------------------------------------------------------
static void prune_free(nif_ctx* c) {
  c->prune_segs_dev.drop(); c->prune_mask.drop(); c->prune_thr.drop(); c->prune_hist.drop(); c->prune_sel.drop();
  c->prune_segs.clear(); c->prune_nblk = 0; c->prune_lo = 0; c->prune_hi = 0;
}
// what every nif_prune_* call is refused for, in front of its guard (NIF_FLUSH_METRIC throughout: the calls of a pruning callback settle
// everything deferred)
static int prune_refused(const nif_ctx* c, bool need_config) {
  if (c->capturing) return fail(NIF_ERR_STATE, "nif_prune_*: not inside a graph capture");
  if (need_config && c->prune_segs.empty()) return fail(NIF_ERR_STATE, "pruning is not configured (nif_prune_config)");
  return NIF_OK;
}
extern "C" int nif_prune_config(nif_ctx* c, int32_t n, const int64_t* offsets, const int64_t* sizes) {
  if (!c || n < 0 || (n > 0 && (!offsets || !sizes))) return fail(NIF_ERR_INVALID, "bad argument");
  std::vector<PruneSeg> segs((size_t)n);
  long nblk = 0, end = 0;
  for (int i = 0; i < n; ++i) {
    const long off = (long)offsets[i], sz = (long)sizes[i];
    if (off < end || sz < 1 || sz > 0x7fffffffL || off + sz > c->P)
      return fail(NIF_ERR_INVALID, "nif_prune_config: segments must be non-empty, below 2^31 floats, inside theta, increasing and disjoint");
    segs[i].off = off; segs[i].size = sz; segs[i].k = sz; segs[i].blk0 = nblk;
    nblk += (sz + PRUNE_CHUNK - 1) / PRUNE_CHUNK;
    end = off + sz;
  }
  int rc = prune_refused(c, false); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_METRIC)
  HIPCHK(hipStreamSynchronize(c->st));      // (queued work may still read the buffers freed here)
  prune_free(c);
  if (n == 0) return NIF_OK;
  // the five tables join the context together, after the last step that can fail: until then pruning stays unconfigured
  DevBuf<PruneSeg> segs_dev; DevBuf<unsigned char> mask; DevBuf<float> thr; DevBuf<unsigned> hist; DevBuf<PruneSel> sel;
  rc = segs_dev.alloc(n); if (rc) return rc;
  rc = mask.alloc(c->P + 16); if (rc) return rc;
  rc = thr.alloc(n); if (rc) return rc;
  rc = hist.alloc((long)PRUNE_BINS * n); if (rc) return rc;
  rc = sel.alloc(n); if (rc) return rc;
  HIPCHK(hipMemcpy(segs_dev, segs.data(), sizeof(PruneSeg) * (size_t)n, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(mask, 1, (size_t)c->P + 16, c->st));
  HIPCHK(hipMemsetAsync(thr, 0, sizeof(float) * (size_t)n, c->st));
  HIPCHK(hipMemsetAsync(hist, 0, sizeof(unsigned) * PRUNE_BINS * (size_t)n, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  c->prune_segs_dev = std::move(segs_dev); c->prune_mask = std::move(mask); c->prune_thr = std::move(thr);
  c->prune_hist = std::move(hist); c->prune_sel = std::move(sel);
  c->prune_segs = segs; c->prune_nblk = nblk; c->prune_lo = segs.front().off; c->prune_hi = end;
  return NIF_OK;
}
extern "C" int nif_prune_update(nif_ctx* c, const int64_t* k) {
  if (!c || !k) return fail(NIF_ERR_INVALID, "null");
  if (!c->have_params) return fail(NIF_ERR_STATE, "parameters not set");
  int rc = prune_refused(c, true); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_METRIC)
  const int n = (int)c->prune_segs.size();
  for (int i = 0; i < n; ++i)
    if (k[i] < 1 || k[i] > c->prune_segs[i].size) return fail(NIF_ERR_INVALID, "nif_prune_update: 1 <= k <= the segment's size");
  HIPCHK(hipStreamSynchronize(c->st));      // (the previous update's copy of the host table is through before the table changes)
  for (int i = 0; i < n; ++i) c->prune_segs[i].k = (long)k[i];
  HIPCHK(hipMemcpyAsync(c->prune_segs_dev, c->prune_segs.data(), sizeof(PruneSeg) * (size_t)n, hipMemcpyHostToDevice, c->st));
  launch_prune_update(c->theta, c->prune_segs_dev, n, c->prune_nblk, c->prune_hist, c->prune_sel, c->prune_thr, c->prune_mask, c->st);
  HIPCHK(hipGetLastError());
  return NIF_OK;
}
extern "C" int nif_prune_apply(nif_ctx* c) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  if (!c->have_params) return fail(NIF_ERR_STATE, "parameters not set");
  int rc = prune_refused(c, true); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_METRIC)
  launch_prune_apply(c->theta, c->prune_mask, c->prune_lo, c->prune_hi, c->P, c->st);
  HIPCHK(hipGetLastError());
  c->planes_stale();      // (theta changed)
  return NIF_OK;
}
static long prune_total(const nif_ctx* c) {
  long t = 0;
  for (const PruneSeg& s : c->prune_segs) t += s.size;
  return t;
}
extern "C" int nif_get_prune_state(nif_ctx* c, float* masks, int64_t n_mask, float* thr, int32_t n_seg) {
  if (!c || !masks || !thr) return fail(NIF_ERR_INVALID, "null");
  int rc = prune_refused(c, true); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_METRIC)
  if (n_mask != prune_total(c) || n_seg != (int32_t)c->prune_segs.size()) return fail(NIF_ERR_INVALID, "nif_get_prune_state: size mismatch");
  std::vector<unsigned char> h((size_t)c->P);
  HIPCHK(hipMemcpyAsync(h.data(), c->prune_mask, (size_t)c->P, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(thr, c->prune_thr, sizeof(float) * (size_t)n_seg, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  long o = 0;
  for (const PruneSeg& s : c->prune_segs)
    for (long i = 0; i < s.size; ++i) masks[o++] = h[(size_t)(s.off + i)] ? 1.f : 0.f;
  return NIF_OK;
}
extern "C" int nif_set_prune_state(nif_ctx* c, const float* masks, int64_t n_mask, const float* thr, int32_t n_seg) {
  if (!c || !masks || !thr) return fail(NIF_ERR_INVALID, "null");
  int rc = prune_refused(c, true); if (rc) return rc;
  NIF_ENTER(c, NIF_FLUSH_METRIC)
  if (n_mask != prune_total(c) || n_seg != (int32_t)c->prune_segs.size()) return fail(NIF_ERR_INVALID, "nif_set_prune_state: size mismatch");
  std::vector<unsigned char> h((size_t)c->P + 16, 1);
  long o = 0;
  for (const PruneSeg& s : c->prune_segs)
    for (long i = 0; i < s.size; ++i, ++o) {
      if (masks[o] != 0.f && masks[o] != 1.f) return fail(NIF_ERR_INVALID, "nif_set_prune_state: mask values are 0 or 1");
      h[(size_t)(s.off + i)] = masks[o] != 0.f ? 1 : 0;
    }
  HIPCHK(hipMemcpyAsync(c->prune_mask, h.data(), h.size(), hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(c->prune_thr, thr, sizeof(float) * (size_t)n_seg, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}

// A rank whose shard has no rows left for a step still joins the collective: with a zero [grad | loss] buffer.
extern "C" int nif_zero_grad(nif_ctx* c) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_METRIC)      // (a deferred loss-metric accumulation reads grad[P]: before it is cleared)
  c->last_step_small = false;
  HIPCHK(hipMemsetAsync(c->grad, 0, sizeof(float) * (size_t)(c->P + 1), c->st));
  c->grad_rewritten();
  return NIF_OK;
}

// A/B switches (measurement and tests; the defaults are the product path)
// PCI bus id ("0000:c1:00.0") of HIP device `dev`: the host side looks up the device's NUMA node under /sys/bus/pci/devices/ and
// pins the rank's process to that node's cores (the reference leaves placement to TensorFlow's runtime)
extern "C" int nif_device_pci_bus_id(int32_t dev, char* out, int32_t cap) {
  if (!out || cap < 16) return fail(NIF_ERR_INVALID, "bad argument");
  HIPCHK(hipDeviceGetPCIBusId(out, cap, dev));
  return NIF_OK;
}

extern "C" int nif_set_option(nif_ctx* c, const char* key, int32_t value) {
  if (!c || !key) return fail(NIF_ERR_INVALID, "null");
  if (strcmp(key, "fuse_gw") == 0) { c->opt_fuse_gw = value != 0; return NIF_OK; }   // 0: k_snet4 + k_gw_* instead of the fused-gradient kernel
  if (strcmp(key, "s6_shape_generic") == 0) { c->opt_s6_shape_generic = value != 0; return NIF_OK; }   // 1: k_snet6<.., 0, 0> on a si = so = 1 net too (A/B, tests)
  if (strcmp(key, "fuse_tail") == 0) { c->opt_fuse_tail = value != 0; return NIF_OK; }     // 0: the row reduction runs inside nif_loss_grad_dev (A/B, tests)
  if (strcmp(key, "small_step") == 0) { c->opt_small_step = value != 0; return NIF_OK; }   // 0: small batches on the tile kernels too (A/B, tests)
  if (strcmp(key, "fp32_mfma") == 0) {      // 1: every product on the f32-input MFMAs (k_snet3) instead of the bf16 splits
    c->opt_fp32_mfma = value != 0;
    c->planes_stale();
    return NIF_OK;
  }
  if (strcmp(key, "snapshot_image_bytes") == 0) {      // nif_forward_snapshots*: bytes of combined nets held at once (0: the default; tests lower it)
    if (value < 0) return fail(NIF_ERR_INVALID, "nif_set_option(\"snapshot_image_bytes\"): >= 0");
    c->opt_snap_bytes = value;
    return NIF_OK;
  }
  if (strcmp(key, "side_pnet") == 0) { c->opt_side_pnet = value != 0; return NIF_OK; }   // ParameterNet adjoint on the second stream
  if (strcmp(key, "pipe_chunk") == 0) { c->opt_pipe_chunk = value; return NIF_OK; }   // points per chunk, 0 = off, -1 = default
  if (strcmp(key, "pipe_wgs") == 0) { c->opt_pipe_wgs = value; return NIF_OK; }       // workgroups of the fused kernel per chunk
  // weight averaging behind every optimizer step of the context (Keras' use_ema; read by opt_step / graph_replay at step time)
  const bool k_ema = strcmp(key, "ema") == 0;
  if (k_ema || strcmp(key, "ema_momentum_bits") == 0) {
    if (c->capturing) return fail(NIF_ERR_STATE, std::string("nif_set_option(\"") + key + "\"): not inside a graph capture");
    if (k_ema) {
      if (value < -1) return fail(NIF_ERR_INVALID, "nif_set_option(\"ema\"): 0 off, -1 on, f >= 1 on and overwrite every f steps");
      c->opt_ema = value;
      return NIF_OK;
    }
    float mom; memcpy(&mom, &value, sizeof(mom));
    if (!(mom >= 0.f && mom <= 1.f)) return fail(NIF_ERR_INVALID, "nif_set_option(\"ema_momentum_bits\"): the bit pattern of a float32 within [0, 1]");
    c->ema_mom = mom;
    return NIF_OK;
  }
  return fail(NIF_ERR_INVALID, std::string("unknown option ") + key);
}

// The one read-out of [grad | loss] to the host, behind the caller's tail flush; either pointer may be NULL.  with_reg: the
// weight-regulariser term is added first (once per gradient: apply_reg)
static int grad_to_host(nif_ctx* c, float* loss, float* grad, bool with_reg) {
  if (with_reg) { const int rcr_ = apply_reg(c); if (rcr_) return rcr_; }
  if (grad) HIPCHK(hipMemcpyAsync(grad, c->grad, sizeof(float) * (size_t)c->P, hipMemcpyDeviceToHost, c->st));
  if (loss) HIPCHK(hipMemcpyAsync(loss, c->grad + c->P, sizeof(float), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return NIF_OK;
}
// the read-out half of nif_loss_and_grad for callers that keep the dataset resident (L-BFGS closure)
extern "C" int nif_grad_read(nif_ctx* c, float* loss, float* grad) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  return grad_to_host(c, loss, grad, true);
}
extern "C" int nif_last_loss(nif_ctx* c, float* loss) {
  if (!c || !loss) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  return grad_to_host(c, loss, nullptr, false);
}

static int stage_batch(nif_ctx* c, const float* xin, const float* y, const float* sw, long B) {
  HIPCHK(hipStreamSynchronize(c->st));
  int rc = stage(c, c->d_a, xin, B * (c->pi + c->si)); if (rc) return rc;
  rc = stage(c, c->d_b, y, B * c->so); if (rc) return rc;
  if (sw) { rc = stage(c, c->d_c, sw, B); if (rc) return rc; }
  return NIF_OK;
}
int nif_stage_batch(nif_ctx* c, const float* xin, const float* y, const float* sw, int64_t B, float** dx, float** dy, float** dsw) {
  int rc = stage_batch(c, xin, y, sw, B); if (rc) return rc;
  *dx = c->d_a; *dy = c->d_b; *dsw = sw ? c->d_c : nullptr;
  return NIF_OK;
}

extern "C" int nif_loss_and_grad(nif_ctx* c, const float* xin, const float* y, const float* sw, int64_t B, float* loss,
                                 float* grad) {
  if (!c || !xin || !y || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  int rc = stage_batch(c, xin, y, sw, B); if (rc) return rc;
  rc = loss_grad_core(c, c->d_a, c->d_b, sw ? c->d_c : nullptr, B, B, 0, nullptr, nullptr, 0.f); if (rc) return rc;
  return nif_grad_read(c, loss, grad);      // (through the guard again: the step may have left its row reduction pending)
}

extern "C" int nif_train_step(nif_ctx* c, const float* xin, const float* y, const float* sw, int64_t B,
                              const nif_adam* opt, float* loss) {
  if (!c || !xin || !y || !opt || B <= 0) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  int rc = stage_batch(c, xin, y, sw, B); if (rc) return rc;
  rc = loss_grad_core(c, c->d_a, c->d_b, sw ? c->d_c : nullptr, B, B, 0, nullptr, nullptr, 0.f); if (rc) return rc;
  const nif_opt o = opt_of_adam(opt);
  rc = opt_step(c, &o, "nif_adam_step_dev"); if (rc) return rc;      // (consumes the step's row reduction)
  return grad_to_host(c, loss, nullptr, false);
}

// ------------------------------------------------------------------------------------------
// measurement
// ------------------------------------------------------------------------------------------
static int drain_profile(nif_ctx* c) {
  HIPCHK(hipStreamSynchronize(c->st));
  for (auto& r : c->recs) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
    c->prof_ms[r.id] += ms; c->prof_cnt[r.id] += 1;
    c->ev_pool.push_back(r.a); c->ev_pool.push_back(r.b);
  }
  c->recs.clear();
  return NIF_OK;
}
extern "C" int nif_profile_enable(nif_ctx* c, int on) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  int rc = drain_profile(c); if (rc) return rc;
  c->prof_on = on != 0;
  return NIF_OK;
}
extern "C" int nif_profile_read(nif_ctx* c, float* ms, int64_t* cnt, int n, int reset) {
  if (!c || !ms || !cnt || n < NIF_PROF_N) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  int rc = drain_profile(c); if (rc) return rc;
  for (int i = 0; i < NIF_PROF_N; ++i) { ms[i] = (float)c->prof_ms[i]; cnt[i] = c->prof_cnt[i]; }
  if (reset) for (int i = 0; i < NIF_PROF_N; ++i) { c->prof_ms[i] = 0; c->prof_cnt[i] = 0; }
  return NIF_OK;
}
extern "C" int nif_debug_timeline(nif_ctx* c, int64_t* out, int32_t n_pairs) {
  if (!c || n_pairs < 0 || n_pairs > 2048) return fail(NIF_ERR_INVALID, "bad argument");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipStreamSynchronize(c->st));
  if (!c->tl) {
    DevBuf<long long> tl;
    const int rc = tl.alloc(4096); if (rc) return rc;
    HIPCHK(hipMemset(tl, 0, 4096 * sizeof(long long)));
    c->tl = std::move(tl);
    return NIF_OK;   // first call arms the buffer
  }
  if (out && n_pairs > 0) HIPCHK(hipMemcpy(out, c->tl, sizeof(long long) * 2 * n_pairs, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(c->tl, 0, 4096 * sizeof(long long)));
  return NIF_OK;
}
extern "C" int nif_timer_start(nif_ctx* c) {
  if (!c) return fail(NIF_ERR_INVALID, "null");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  if (!c->t0) { HIPCHK(hipEventCreate(&c->t0)); HIPCHK(hipEventCreate(&c->t1)); }
  HIPCHK(hipEventRecord(c->t0, c->st));
  return NIF_OK;
}
extern "C" int nif_timer_stop(nif_ctx* c, float* ms) {
  if (!c || !ms || !c->t0) return fail(NIF_ERR_INVALID, "timer not started");
  NIF_ENTER(c, NIF_FLUSH_TAIL)
  HIPCHK(hipEventRecord(c->t1, c->st));
  HIPCHK(hipEventSynchronize(c->t1));
  HIPCHK(hipEventElapsedTime(ms, c->t0, c->t1));
  return NIF_OK;
}
