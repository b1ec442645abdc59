// nif_ctx.h -- the context object behind the opaque nif_ctx* of include/nif_hip.h, shared by the translation units
// that implement the C-ABI (nif_api.hip: orchestration; nif_comm.hip: RCCL).
#pragma once
#include "../../include/nif_hip.h"
#include "nif_internal.h"
#include <string>
#include <vector>

int nif_fail(int code, const std::string& msg);   // sets the thread-local message behind nif_last_error()
static inline int fail(int code, const std::string& msg) { return nif_fail(code, msg); }
#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      (void)hipGetLastError(); /* HIP >= 7 keeps the last failure until it is read: drain it, or the next launch check of a   \
                                  caller that recovered (fit()'s host-shuffle fallback after a failed hipMalloc) reports it */ \
      return fail(NIF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    }                                                                                             \
  } while (0)

struct nif_ctx;
// The one owner of a device allocation (Pinned: of a pinned host block): move-only, frees in its destructor, converts to T* so that
// launch arguments read as with a raw pointer.  n is the element count it was allocated with -- the capacity; there is no second field.
// Exact sizes, no geometric growth, contents not kept.  After a failed allocation the buffer is empty (p null, n 0): the call can be repeated.
template <class T, bool Pinned = false>
struct DevBuf {
  T* p = nullptr; long n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { drop(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
  ~DevBuf() { drop(); }
  operator T*() const { return p; }
  void drop() {      // no stream synchronisation of its own: for buffers nothing queued can read (locals, teardown, after a failure)
    if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr; n = 0;
  }
  int alloc(long count) {      // a fresh block of exactly `count` elements for a buffer that is empty (first use, set-up built into locals)
    drop();
    T* q = nullptr;
    if (Pinned) HIPCHK(hipHostMalloc(&q, sizeof(T) * (size_t)count));
    else HIPCHK(hipMalloc(&q, sizeof(T) * (size_t)count));
    p = q; n = count;
    return NIF_OK;
  }
  int release(nif_ctx* c);                 // the context's streams drained, then freed
  int reserve(nif_ctx* c, long count);     // nothing (no synchronisation either) when count <= n; else release + alloc
};

struct NifF64;      // state of the double-precision L-BFGS closure (k_f64.hip), allocated at its first use
// What a capture (nif_graph_begin .. nif_graph_end) recorded: a replay accounts for it, and a graph is replayed only under the optimizer
// kind, amsgrad flag and weight-averaging setting it holds
struct CapInfo {
  int steps = 0;        // optimizer steps: a replay advances the iteration count by them
  int kind = -1;        // kernel kind of those steps (-1: no update step) ...
  bool ams = false;     // ... and whether they use the third slot
  bool ema = false;     // recorded with the weight average (nif_set_option "ema")
  int gt = 0;           // gradient-transform launches (0 none, 1 k_gt_reduce, 2 both)
  long step0 = 0;       // the running capture only: the iteration count at nif_graph_begin (nothing runs until a replay)
};
struct CapGraph { hipGraphExec_t exec; CapInfo info; };      // exec null: destroyed (nif_graph_destroy), the id stays taken

struct nif_ctx {
  nif_cfg cfg;
  NifF64* f64 = nullptr;
  int dev = 0;
  hipStream_t st = nullptr;
  // derived sizes
  int kind, pi, si, so, n, L, nst, lst, r, nh, nm, NB, NSTB;
  long po, P;
  std::vector<nif_tensor_desc> layout;
  // theta offsets
  long first_w, first_b, hid_w[NIF_MAX_HID], hid_b[NIF_MAX_HID], hid_w2[NIF_MAX_HID], hid_b2[NIF_MAX_HID];
  long bott_w, bott_b, last_w, last_b;
  // last-layer class: shared-weight SIREN ShapeNet (model.py:1147-1217) + last_layer_bias
  long s_first_w = 0, s_first_b = 0, s_hid_w[NIF_MAX_HID], s_hid_b[NIF_MAX_HID], s_hid_w2[NIF_MAX_HID], s_hid_b2[NIF_MAX_HID];
  long s_bott_w = 0, s_bott_b = 0, ll_bias = 0;
  int RB = 1;   // ZL rows per tile = 32*RB
  // device state
  DevBuf<float> theta, grad, m, v;
  long step = 0;
  bool have_params = false, packed = false, packed32 = false, packed_p32 = false, use_snet3 = false, use_snet4 = false;
  bool jac_ok = false;        // JacobianLayer / HessianLayer kernels take this shape (jac_supported)
  DevBuf<char> sWF4, sWB4;   // bf16-split planes of the hidden hyper-matrices (k_snet4)
  DevBuf<char> sWF4x, sWB4x; // k_snet6 (r5): exact-product HALF (hi, lo) planes of the hidden hyper-matrices (k_pack16b mode 3)
  DevBuf<float> sWscale;                   //   and their powers of two [matrix][plane]
  DevBuf<char> sWF4h, sWB4h; // the policies' compact plane set (one bf16 / half plane per block: k_snet4 / k_snet6<.., PR>)
  bool use_ll4 = false;                    // last-layer class: dense ShapeNet on k_snet4
  DevBuf<float> ll_slots;                  // its parameters in k_snet4's slot order (launch_ll_slots)
  DevBuf<char> ll_wpf, ll_wpb;   // phi layer as bf16-split MFMA operands (launch_pack_phi)
  DevBuf<f32x4> pWF, pWB, sWF, sWB, lWF, lWB;
  // workspaces: cap is the capacity in points of the point workspaces (Z .. DZL) and, where they exist, of the stashes (their slot
  // strides derive from it); every other buffer's capacity is its own n
  long cap = 0;
  DevBuf<float> stash_s, stash_p, Z, DZ, DU, ZL;
  long slot_s = 0, slot_p = 0;
  DevBuf<float> partial; long pstride = 0;     // [rows_cap()][pstride] partial gradient | loss rows; pstride is fixed by P (nif_create)
  int rows_cap() const { return (int)(partial.n / pstride); }
  DevBuf<float> loss_partial;
  DevBuf<float> dring;
  DevBuf<long long> tl;      // timeline stamps (measurement builds)
  float reg_l1 = 0.f, reg_l2 = 0.f; long reg_lo = 0, reg_hi = 0; bool reg_applied = false;
  float sreg_l1 = 0.f, sreg_l2 = 0.f;   // last-layer class: cfg_shape_net l1_reg / l2_reg over the shared ShapeNet's kernels and biases [s_first_w, ll_bias)
  DevBuf<double> metric;     // device {sum, count}
  // activity regulariser of the ParameterNet output (nif_set_activity_regularizer): L2 wins over L1 like in the reference
  bool ll_packed32 = false;     // last-layer class under k_sob at n > 96: f32-input MFMA planes of the shared hidden matrices in sWF / sWB
  DevBuf<float> zt_par, dzt_par;
  DevBuf<float> dat_par, ztl_par;   // last-layer class: dL/da', z' in latent-row layout   // Sobolev with parameter seeds: dz/dp, dL/d(dz/dp)
  float jac_l1 = 0.f; DevBuf<float> jac_mu, jac_tmp;   // latent Jacobian regulariser (k_pjac)
  // captured training steps (nif_graph_*): the finished graphs, the record of the running capture, and the device-side optimizer
  // state a replay refreshes (with its pinned staging copy)
  std::vector<CapGraph> graphs; bool capturing = false; CapInfo rec;
  DevBuf<OptDev> opt_dev; DevBuf<OptDev, true> opt_host;
  DevBuf<float> vhat;          // the third optimizer slot (amsgrad's vhat, centered RMSprop's a), allocated on first use
  bool slots_fresh = true;     // m, v are zero and the iteration count 0: Adagrad's first step writes its initial accumulator
  // weight averaging behind every optimizer step (Keras' use_ema; nif_set_option "ema" / "ema_momentum_bits"): opt_ema 0 off, -1 on,
  // f >= 1 on and theta overwritten by the average every f steps.  ema is optimizer slot 3, allocated on first use and never freed
  // (captured graphs hold its address); ema_valid false: the next step (or replay) seeds it with theta (nif_set_opt_state resets it).
  int opt_ema = 0; float ema_mom = 0.99f; DevBuf<float> ema; bool ema_valid = false;
  // magnitude pruning (nif_prune_*): the segment table (host copy: the k of the last update), its span [prune_lo, prune_hi), a byte mask
  // over the whole of theta (1 outside the segments), the thresholds and the select's histograms / per-segment state
  std::vector<PruneSeg> prune_segs; long prune_nblk = 0, prune_lo = 0, prune_hi = 0;
  DevBuf<PruneSeg> prune_segs_dev; DevBuf<unsigned char> prune_mask; DevBuf<float> prune_thr;
  DevBuf<unsigned> prune_hist; DevBuf<PruneSel> prune_sel;
  // gradient transform (nif_set_grad_transform): the configured struct, whether any stage is on / a norm stage is on, the work-block
  // table, one partial sum of squares per block, the norms [tensors | global], and the struct's device copy; all built at the first
  // non-zero set.  gt_ran: 0 no transform has run, 1 the last one ran without a norm stage (norms not formed yet), 2 with.
  nif_grad_transform gt = {}; bool gt_on = false, gt_norm = false; int gt_ran = 0;
  DevBuf<GtBlk> gt_blk; int gt_nblk = 0; DevBuf<float> gt_part, gt_norms; DevBuf<GtDev> gt_dev;
  bool ll_mlp_packed = false;        // last-layer class: the f32 planes of the 32-point MLP kernels are current
  int loss_kind = 0;                 // NIF_LOSS_* (nif_set_loss)
  DevBuf<float> sob2_acc;            // [grad | loss] summed over the passes of a second-order Sobolev step (nif_sobolev2_loss_grad_dev)
  DevBuf<float> sob_acc;             // [grad | loss] summed over the column groups of a Sobolev step with more than three x_index columns
  float act_l1 = 0.f, act_l2 = 0.f; DevBuf<float> act_part, act_loss;
  DevBuf<float> PHI, DPHI, DA, DZL;
  // last-layer class at 129..512 units (k_wide.hip, decided at nif_create): the layers' activations of a forward pass / dL/da of an
  // adjoint sweep alternate between the two halves of wide_act [2][n][cap]; a training step keeps sin and cos of every layer's phase
  // in wide_stash [2 (nh + 1)][n][cap] (slot l: sin of layer l, slot nh + 1 + l: its cos).  Both grow in ensure_capacity
  bool use_wide = false;
  DevBuf<float> wide_act, wide_stash;
  // profiling: (group id, start, stop) event triples recorded on st
  bool prof_on = false;
  std::vector<hipEvent_t> ev_pool;
  struct Rec { int id; hipEvent_t a, b; };
  std::vector<Rec> recs;
  double prof_ms[NIF_PROF_N] = {0};
  long prof_cnt[NIF_PROF_N] = {0};
  hipEvent_t t0 = nullptr, t1 = nullptr;
  // staging for the host-pointer API
  DevBuf<float> d_a, d_b, d_c, d_d;
  // the snapshot calls (nif_forward_snapshots*, nif_snapshot_derivatives*, nif_snapshot_param_derivatives*; nif_api.hip SnapPlan):
  // [offsets | latent rows | the call's extra head rows | table, or the combined nets of one chunk of snapshots: slot vectors and
  // packed planes] of one call, rebuilt by every call.  opt_snap_bytes: the chunk's budget (nif_set_option "snapshot_image_bytes",
  // 0 = the default).  snap_io: the staging of the two derivative calls' host-pointer entries, [rows | .. | outputs] (calls on a
  // context are serial; the forward and encode entries stage through d_a .. d_d and enc_S)
  DevBuf<float> snap, snap_io; long opt_snap_bytes = 0;
  // per-snapshot normal equations (nif_snapshot_normal_eq*, k_encode.hip): [tile_start | offsets] of one call and the padded operands
  // [Z | unit pattern | xpad | dydx | u] of one chunk of snapshots (bounded by the same budget), rebuilt by every call; enc_S stages
  // the host-pointer entry's result
  DevBuf<float> enc; DevBuf<double> enc_S;
  // snapshot-wise derivatives (nif_snapshot_derivatives*): sd_tmp takes the second-order output of an order-1 call on the routes that
  // run the second-order kernels anyway.  (The first-order parameter derivatives keep everything in `snap` and the point workspaces;
  // their second order, nif_snapshot_param_second_derivatives*, takes it for the last-layer route's rows over every output and for
  // HessianLayer's results on the table route.)
  DevBuf<float> sd_tmp;
  // the snapshot-wise training step (nif_snapshot_loss_grad*, k_snapfit.hip): every mesh tile's share of dL/da, [mesh tiles][T][r]
  DevBuf<float> sf_dap;
  // sensor placement (nif_select_sensors*, k_sensors.hip): the partial rows (int64) | partial scores | Q [K][r] | scores | residual
  DevBuf<float> sens;
  // RCCL communicator of this context (nif_comm.hip): one rank = one ctx = one GPU
  void* comm = nullptr; int comm_rank = 0, comm_world = 1;
  DevBuf<float> comm_scratch;      // 64 B device scratch for barrier()
  // two-stream chunk pipeline of the training step (nif_api.hip: loss_grad_core)
  hipStream_t st2 = nullptr; hipEvent_t ev_start = nullptr, ev_done = nullptr; std::vector<hipEvent_t> ev_chunk;
  DevBuf<float> chunk_grad;                            // [chunks][pstride]: per-chunk gradient | loss rows
  bool opt_side_pnet = false;                          // whole-batch step: ParameterNet adjoint on st2 next to the gradient reductions
  long opt_pipe_chunk = -1; int opt_pipe_wgs = 512;    // points per chunk (-1 default, 0 off); fused-kernel workgroups per chunk
  // shard streaming (nif_h2d_async): a copy stream and, per staging slot, 'copy landed' / 'slot consumed' events
  hipStream_t st_copy = nullptr; hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_consumed[2] = {nullptr, nullptr};
  bool opt_fp32_mfma = false;      // nif_set_option("fp32_mfma"): A/B switch, default from NIF_FP32_MFMA
  DevBuf<int> small_idx, small_desc;                       // k_small's tables (offsets only), built at the first small step
  bool metric_pending = false; float metric_pending_w = 0.f;   // a nif_metric_accumulate deferred into the next k_small launch
  bool last_step_small = false;
  // r6: the row reduction of a plain step may wait for its consumer -- the optimizer step then runs it fused with the update (one launch
  // less per step); what else consumes it says so at the door (nif_enter).  nif_set_option("fuse_tail") / NIF_FUSE_TAIL
  bool tail_pending = false; int tail_rows = 0, tail_nloss = 0; bool opt_fuse_tail = true;
  bool opt_small_step = true;      // nif_set_option("small_step"): batches <= NIF_SMALL_MAX_B points of a net k_small takes run on it (one launch for loss + gradient); default from NIF_SMALL_STEP
  bool opt_fuse_gw = true;         // nif_set_option("fuse_gw"): ShapeNet weight gradients inside the training kernel (k_snet6) where it has the shape; default from NIF_FUSE_GW
  bool opt_s6_shape_generic = false;      // nif_set_option("s6_shape_generic"): k_snet6's run-time si / so form on a one-coordinate, one-output net too (A/B, tests)
  // the invalidations, each the one statement of what it clears
  void planes_stale() { packed = false; packed32 = false; packed_p32 = false; }      // theta (or what the planes are packed for) changed
  void theta_stepped() { planes_stale(); reg_applied = false; }      // an optimizer step or replay: the regulariser term belongs to ONE gradient
  void grad_rewritten() { reg_applied = false; }      // [grad | loss] holds a new step's sums (or zeros): the old gradient's term is gone
  nif_ctx() = default;
  nif_ctx(const nif_ctx&) = delete;
  ~nif_ctx();      // streams, events, graph executables, the communicator and the float64 state; then the buffers free themselves (nif_api.hip)
};

template <class T, bool Pinned> int DevBuf<T, Pinned>::release(nif_ctx* c) {
  HIPCHK(hipStreamSynchronize(c->st));
  if (c->st2) HIPCHK(hipStreamSynchronize(c->st2));
  drop();
  return NIF_OK;
}
template <class T, bool Pinned> int DevBuf<T, Pinned>::reserve(nif_ctx* c, long count) {
  if (count <= n) return NIF_OK;
  const int rc = release(c); if (rc) return rc;
  return alloc(count);
}

// RAII-ish helper: records an event pair around a kernel group when profiling is on
struct ProfScope {
  nif_ctx* c; int id; hipEvent_t a = nullptr, b = nullptr;
  hipStream_t s;
  ProfScope(nif_ctx* c_, int id_, hipStream_t s_ = nullptr) : c(c_), id(id_), s(s_ ? s_ : c_->st) {
    if (!c->prof_on || c->capturing) return;      // (an event recorded into a capture is a graph node: it never holds a time, and reading it fails)
    auto get = [&]() { hipEvent_t e; if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); } else { (void)hipEventCreate(&e); } return e; };
    a = get(); b = get();
    (void)hipEventRecord(a, s);
  }
  ~ProfScope() {
    if (!a) return;
    (void)hipEventRecord(b, s);
    c->recs.push_back({id, a, b});
  }
};

// The door of the C-ABI (DESIGN "Deferred state"): every extern "C" function that touches device state of a context passes it once,
// behind its argument and state refusals -- the context's device selected, then the deferred pieces run that the entry point names:
//   NIF_FLUSH_NONE    neither: it works on buffers of its own, consumes the tail itself (the optimizer steps) or ends / drops a capture
//   NIF_FLUSH_TAIL    the row reduction: it reads or rewrites [grad | loss], the partial rows, theta or the stream's order
//   NIF_FLUSH_METRIC  and the loss-metric accumulation: it rewrites grad[P] without a k_small launch, or reads the metric
enum nif_flush { NIF_FLUSH_NONE, NIF_FLUSH_TAIL, NIF_FLUSH_METRIC };
int nif_enter(nif_ctx* c, nif_flush what);
#define NIF_ENTER(c_, what_) { const int rce_ = nif_enter(c_, what_); if (rce_) return rce_; }
// The two pieces of work behind it (nif_api.hip).  Besides nif_enter only their consumers inside a guarded call run them: the optimizer
// step that cannot fuse the tail, the tile path of a step and apply_reg (both rewrite grad[P]), and nif_metric_flush the tail
int nif_tail_flush(nif_ctx* c);        // the deferred row reduction of the last plain step (nif_ctx::tail_pending)
int nif_metric_flush(nif_ctx* c);      // a nif_metric_accumulate that waits for the next k_small launch (nif_ctx::metric_pending)
// host batch -> this context's staging buffers (asynchronous H2D on c->st); used by the host-pointer entry points
int nif_stage_batch(nif_ctx* c, const float* xin, const float* y, const float* sw, int64_t B, float** dx, float** dy, float** dsw);
void nif_f64_release(nif_ctx* c);      // deletes the state of the double-precision path (k_f64.hip; ~nif_ctx)
