// The executors' shared enqueue helpers: one launch helper per layer kind on
// a plan's core, the weight-gradient arena and branch ordering of Ctx, the
// U-Net's branch stream and its hipGraph cache.
#include "exec.h"

namespace hcu {

// ---- Ctx ----

// HCU_WGF_DEFER=0: finalize each layer right after its weight gradient (A/B)
static bool defer_wgf() {
  static const bool on = !(getenv("HCU_WGF_DEFER") && getenv("HCU_WGF_DEFER")[0] == '0');
  return on;
}

int Ctx::pend_wgf(const WGradFinalize &f) {
  pend.push_back(f);
  return defer_wgf() ? 0 : flush_wgf();
}

int Ctx::flush_wgf() {
  int e = 0;
  // HCU_DEBUG_NO_WGF=1 drops every weight-gradient finalize: WRONG gradients,
  // a timing probe only (what the finalizes cost a step)
  static const bool no_wgf = getenv("HCU_DEBUG_NO_WGF") && getenv("HCU_DEBUG_NO_WGF")[0] == '1';
  if (!pend.empty() && !no_wgf) e = launch_wgrad_finalize_batch(pend.data(), (int)pend.size(), wstream());
  pend.clear();
  wp_off = 0;
  return e;
}

// A request the whole arena cannot hold is refused: the plan sizes the arena
// from the same job records that make the requests (ScratchNeed::arena).
int Ctx::slab(size_t floats, float *&ptr) {
  if (floats > p.wpart_floats)
    return fail(HCU_ERR_WORKSPACE, "weight-gradient slab of " + std::to_string(floats) +
                                       " floats exceeds the plan's arena of " +
                                       std::to_string(p.wpart_floats) + " floats");
  const size_t need = (floats + 63) / 64 * 64;
  if (wp_off + need > p.wpart_floats || pend.size() >= 64)
    if (int e = flush_wgf()) return e;
  ptr = fptr(sc, p.wpart_off) + wp_off;
  wp_off += need;
  return 0;
}

int Ctx::alloc(int &slot) {
  slot = next_slot;
  next_slot = (next_slot + 1) % p.nbuf;
  if (split && (slot_read & (1u << slot))) HCU_HIP(hipStreamWaitEvent(s, br->ev_slot[slot], 0));
  return HCU_OK;
}

int Ctx::fork() {
  if (!split) return HCU_OK;
  const ChainRec &r = chain_rec();
  if (r.ev == br->ev_chain && r.s == s && r.n > chain_n0) {
    // the chain's last kernel carries ev_chain as its stop event (HCU_LAUNCH)
    HCU_HIP(hipStreamWaitEvent(ws, br->ev_chain, 0));
    return HCU_OK;
  }
  hipEvent_t ev = br->next_marker();
  HCU_HIP(hipEventRecord(ev, s));
  HCU_HIP(hipStreamWaitEvent(ws, ev, 0));
  return HCU_OK;
}

void Ctx::arm_chain() {
  if (!split || !br->ev_chain) return;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;   // captured graphs keep their markers
  if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return;
  }
  ChainRec &r = chain_rec();
  r.s = s;
  r.ev = br->ev_chain;
  chain_n0 = r.n;
  armed = true;
}

int Ctx::read_done(int slot) {
  if (!split || slot < 0 || p.no_reuse) return HCU_OK;   // no_reuse: never rewritten
  HCU_HIP(hipEventRecord(br->ev_slot[slot], ws));
  slot_read |= 1u << slot;
  return HCU_OK;
}

int Ctx::join() {
  if (!split) return HCU_OK;
  hipEvent_t ev = br->next_marker();
  HCU_HIP(hipEventRecord(ev, ws));
  HCU_HIP(hipStreamWaitEvent(s, ev, 0));
  return HCU_OK;
}

// ---- the branch ----

void Branch::destroy() {
  if (side) (void)hipStreamDestroy(side);
  for (hipEvent_t *e : {&ev_fork, &ev_join, &ev_chain, &ev_prep})
    if (*e) (void)hipEventDestroy(*e);
  for (hipEvent_t &e : ev_slot)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t &e : ev_fork_ring)
    if (e) (void)hipEventDestroy(e);
  side = nullptr;
  ev_fork = ev_join = ev_chain = ev_prep = nullptr;
  for (hipEvent_t &e : ev_slot) e = nullptr;
  for (hipEvent_t &e : ev_fork_ring) e = nullptr;
}

int Branch::ensure(int dev) {
  if (side && side_device == dev) return HCU_OK;
  destroy();
  // (stream priority of the branch, either way, measured no effect in round 3)
  HCU_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
  side_device = dev;
  for (hipEvent_t *e : {&ev_fork, &ev_join, &ev_chain, &ev_prep})
    HCU_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  for (hipEvent_t &e : ev_slot) HCU_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (hipEvent_t &e : ev_fork_ring) HCU_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return HCU_OK;
}

bool side_enabled() {   // HCU_SIDE=0 keeps the whole backward on one stream (A/B, debugging)
  static const bool on = [] {
    const char *e = getenv("HCU_SIDE");
    return !(e && e[0] == '0');
  }();
  return on;
}

// ---- the graph cache ----

GraphCache::~GraphCache() {
  for (Graph &g : graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (cap_stream) (void)hipStreamDestroy(cap_stream);
}

int GraphCache::begin_capture(int dev) {
  if (!cap_stream || cap_device != dev) {
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    cap_stream = nullptr;
    HCU_HIP(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
    cap_device = dev;
  }
  HCU_HIP(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
  return HCU_OK;
}

int GraphCache::end_capture(int e, const std::vector<uintptr_t> &key, hipStream_t s, Branch &br) {
  hipGraph_t graph = nullptr;
  const hipError_t ce = hipStreamEndCapture(cap_stream, &graph);
  if (e || ce != hipSuccess) {
    if (graph) (void)hipGraphDestroy(graph);
    // A failure after the backward forked its weight-gradient branch leaves
    // the branch stream in an invalidated capture: recreate it on next use.
    br.destroy();
    if (e) return e;
    return fail(HCU_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
  }
  hipGraphExec_t exec = nullptr;
  const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ie != hipSuccess)
    return fail(HCU_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
  if (graphs.size() >= 8) {
    auto lru = std::min_element(graphs.begin(), graphs.end(),
                                [](const auto &a, const auto &b) { return a.used < b.used; });
    (void)hipGraphExecDestroy(lru->exec);
    graphs.erase(lru);
  }
  graphs.push_back({key, exec, ++gclock});
  HCU_HIP(hipGraphLaunch(exec, s));
  return HCU_OK;
}

// ---- layer helpers ----

int check_forward_tensors(const PlanCore &p, const hcu_unet_tensors *t) {
  if (!t || !t->x || !t->out || !t->params || !t->saved || !t->scratch)
    return fail(HCU_ERR_INVALID, "null argument");
  if (t->x_dtype != HCU_F32 && t->x_dtype != HCU_F16 && !(t->x_dtype == HCU_BF16 && p.es == 2))
    return fail(HCU_ERR_INVALID, "unsupported input dtype for this plan");
  return 0;
}

// The planned convolution `plan` bound to its operands: the input (with the
// BatchNorm scale / shift its staging applies, or null), the weight image, the
// bias, the output, the epilogue's statistics rows (or null) and the K-split
// partials (kernels that do not split ignore them).
GConvArgs bind_conv(const GConvArgs &plan, const float *in, const float *in_scale, const float *in_shift,
                    const float *w, const float *bias, float *out, float *stats, float *partial) {
  GConvArgs a = plan;
  a.in = in;
  a.in_scale = in_scale;
  a.in_shift = in_shift;
  a.w = w;
  a.bias = bias;
  a.out = out;
  a.stats = stats;
  a.partial = partial;
  return a;
}

// Binds and launches (the sites without a fused BatchNorm backward, fuse_bnbwd).
int run_conv(const GConvArgs &plan, const float *in, const float *in_scale, const float *in_shift,
             const float *w, const float *bias, float *out, float *stats, float *partial, hipStream_t s) {
  return launch_conv_any(bind_conv(plan, in, in_scale, in_shift, w, bias, out, stats, partial), s);
}

// ConvTranspose3d forward of `u` into U, its full output (a chain crops a
// padded layer's afterwards): the phase-folded GEMM, else one launch per phase.
int convt_forward(const Ctx &c, const ConvTLayer &u, const float *in, const float *in_scale,
                  const float *in_shift, float *U) {
  const float *bias = c.param(u.b_off);
  if (u.fused)
    return run_conv(u.fwdf, in, in_scale, in_shift, c.image(u.wf_off), bias, U, nullptr, c.kpart(), c.s);
  for (size_t ph = 0; ph < u.phases.size(); ++ph)
    if (int e = run_conv(u.phases[ph], in, in_scale, in_shift, c.image(u.wph_off[ph]), bias, U, nullptr,
                         c.kpart(), c.s))
      return e;
  return 0;
}

// The pointwise kernel (pwconv.hip) of the 1x1x1 layer L: its forward (in = x,
// out = y) or its input gradient (in = dy, out = dx; no bias).
PwArgs pw_args(const ConvLayer &L, bool dgrad, const float *in, const float *w, const float *bias, float *out) {
  PwArgs a{};
  a.in = reinterpret_cast<const uint16_t *>(in);
  a.w = w;
  a.bias = dgrad ? nullptr : bias;
  a.out = reinterpret_cast<uint16_t *>(out);
  a.nvox = L.out.vox();
  a.ICs = dgrad ? L.out.Cs : L.in.Cs;
  a.OCs = dgrad ? L.in.Cs : L.out.Cs;
  a.Cin = L.Cin_g;
  a.Cout = L.Cout;
  a.part_c = L.part_c;
  a.part_cs = L.part_cs;
  a.dgrad = dgrad ? 1 : 0;
  return a;
}

// in_fmt > 0 (the first layer, UnetPlan::ncx_first): `in` is the
// caller's NCXYZ input volume, read by the conv's own halo staging, which also
// writes the channels-last copy xcl_out (when not null).
int conv_forward(const Ctx &c, const ConvLayer &L, const float *in, const float *isc,
                 const float *ish, int training, int in_fmt, float *xcl_out) {
  HCU_HIP(hipGetLastError());
  tag(L.name, "fwd");
  // (in_fmt: the weight is read in the PyTorch layout by the NCXYZ staging)
  GConvArgs a = bind_conv(L.fwd, in, isc, ish, in_fmt ? c.P + L.w_off : c.image(L.wf_off), c.param(L.b_off),
                          c.fptr(c.sv, L.y_off), training ? c.part() : nullptr, c.kpart());
  a.in_fmt = in_fmt;
  a.in_c = in_fmt ? L.in.C : 0;
  a.xcl = xcl_out;
  const BNCoef coef = coef_at(c.sv, L.bn);
  if (int e = launch_conv_any(a, c.s)) return e;
  return launch_bn_fwd_finalize(c.part(), gconv_rows(L.fwd), L.fwd.CoutW, L.bn.C, L.bn.Cs,
                                L.bn.count, c.P + L.bn.gamma, c.P + L.bn.beta,
                                c.t.bn_running_mean[L.bn.index], c.t.bn_running_var[L.bn.index],
                                c.t.bn_num_batches_tracked[L.bn.index], c.p.bn_eps,
                                c.p.bn_momentum, training, coef, c.s);
}

// Sets up the dgrad epilogue that also performs the BatchNorm+ReLU backward
// reduction of layer `bnl` (whose output the gradient is for); false when the
// planned kernel cannot.
bool fuse_bnbwd(Ctx &c, GConvArgs &a, const ConvLayer *bnl) {
  static const bool off = getenv("HCU_NO_BNFUSE") != nullptr;   // A/B debugging
  if (off || !bnl || !conv_family(a).bnbwd) return false;
  const BNCoef coef = coef_at(c.sv, bnl->bn);
  a.bn_y = c.fptr(c.sv, bnl->y_off);
  a.bn_scale = coef.scale;
  a.bn_shift = coef.shift;
  a.bn_mean = coef.mean;
  a.bn_invstd = coef.invstd;
  a.stats = c.part();
  return true;
}

// Finalize and apply of a BatchNorm backward whose reduction rows are in
// c.part(): dz -> dY of bnl in place.
int finish_bn(const Ctx &c, const ConvLayer &bnl, int R, int W, float *dz, int training, int accumulate) {
  const BNCoef coef = coef_at(c.sv, bnl.bn);
  if (int e = launch_bn_bwd_finalize(c.part(), R, bnl.bn.C, bnl.bn.Cs, W, bnl.bn.count, coef,
                                     c.G + bnl.bn.gamma, c.G + bnl.bn.beta, training, accumulate, c.s))
    return e;
  return launch_bn_bwd_apply(dz, c.fptr(c.sv, bnl.y_off), coef, bnl.out.vox(), bnl.out.Cs, c.s, c.bf());
}

// Input gradient dP of the ConvTranspose3d `u` from dU.  With `bnl`, the
// layer that produced u's input, its BatchNorm+ReLU backward is fused into the
// kernel where the planned one can (fuse_bnbwd): dP then leaves as bnl's
// d(pre-BN y).  fused: whether that happened (else the caller's to run).
int convt_dgrad(Ctx &c, const ConvTLayer &u, const float *dU, float *dP, const ConvLayer *bnl, int training,
                int accumulate, bool &fused) {
  GConvArgs a = bind_conv(u.dgrad, dU, nullptr, nullptr, c.image(u.wd_off), nullptr, dP, nullptr, c.kpart());
  fused = fuse_bnbwd(c, a, bnl);
  if (int e = launch_conv_any(a, c.s)) return e;
  if (!fused) return 0;
  tag(bnl->name, "bnbwd");
  return finish_bn(c, *bnl, gconv_rows(a), a.CoutW, dP, training, accumulate);
}

// Runs one planned weight gradient on the branch stream: takes its slab,
// launches the kernel (the pointwise form for a 1x1x1 job whose input carries
// no BatchNorm+ReLU) and queues the finalize into dw / db for the next flush
// (Ctx::slab / end of backward).
int run_wgrad(Ctx &c, const WGradJob &j, const float *A, const float *a_scale, const float *a_shift,
              const float *G, float *dw, float *db, int accumulate) {
  WGradFinalize f = j.f;
  float *slab = nullptr;
  if (j.pw_blocks && !a_scale) {
    if (int e = c.slab(j.pw_slab, slab)) return e;
    f.partial = slab;
    f.KB = j.pw_blocks;
    const PwWgArgs pa = pw_wgrad_args(f, A, G, wgrad_gvox(j.w), j.w.ACs, j.w.GCs);
    if (int e = launch_pw_wgrad(pa, j.pw_blocks, c.wstream())) return e;
  } else {
    if (int e = c.slab(j.slab, slab)) return e;
    WGradArgs w = j.w;
    w.A = A;
    w.a_scale = a_scale;
    w.a_shift = a_shift;
    w.G = G;
    w.partial = slab;
    if (int e = launch_wgrad(w, c.wstream())) return e;
    f.partial = slab;
  }
  f.dw = dw;
  f.db = db;
  f.accumulate = accumulate;
  return c.pend_wgf(f);
}

// A bias gradient from column-sum rows [R][W] (mode 2) or forward-statistics
// rows (mode 4), summed with the batched finalizes.
WGradFinalize wgf_colsum(int mode, const float *rows, int R, int W, int Cout, float *db, int accumulate) {
  WGradFinalize f{};
  f.partial = rows;
  f.db = db;
  f.KB = R;
  f.Mtot = 1;
  f.Ntot = W;
  f.mode = mode;
  f.Cout = Cout;
  f.accumulate = accumulate;
  return f;
}

// The weight-gradient half of conv_backward (forked onto the branch).
int conv_wgrad(Ctx &c, const ConvLayer &L, const float *A, const float *asc, const float *ash,
               const float *dy, int dy_slot, int accumulate) {
  tag(L.name, "wgrad");
  if (int e = c.fork()) return e;
  if (int e = run_wgrad(c, L.wg, A, asc, ash, dy, c.G + L.w_off, c.grad(L.b_off), accumulate))
    return e;
  return c.read_done(dy_slot);
}

// Weight/bias gradient and (optionally) input gradient of one Conv3d layer.
// dy holds dY of L.  With `bnl`, the input gradient leaves as dz of layer bnl
// (its BatchNorm+ReLU backward fused into the dgrad) and *bn_done is set.
// With `colsum` (and no bnl) the input gradient's kernel also writes its
// per-workgroup statistics rows there (gconv_rows x CoutW of {S1, S2, K, n}):
// the column sums of dA, finalized as the bias gradient of the layer that
// produced A (a ConvTranspose3d: no separate reduction pass over dA).
// wg_late: the weight gradient is forked after the input gradient's
// convolution is enqueued (and before its BatchNorm finalize), so the
// branch's kernel does not start beside it (HCU_L0_ORDER, level 0 A/B).
int conv_backward(Ctx &c, const ConvLayer &L, const float *A, const float *asc,
                  const float *ash, const float *dy, int dy_slot, float *dA, int accumulate,
                  const ConvLayer *bnl, int training, bool *bn_done, float *colsum, bool wg_late) {
  if (!wg_late || !dA)
    if (int e = conv_wgrad(c, L, A, asc, ash, dy, dy_slot, accumulate)) return e;
  if (!dA) return 0;
  tag(L.name, "dgrad");
  if (L.pw && !bnl && !colsum) {   // (the chains' non-BatchNorm 1x1x1 convolutions)
    if (int e = launch_pw(pw_args(L, true, dy, c.P + L.w_off, nullptr, dA), c.s)) return e;
    // (wg_late is not reached here today: its one caller, the U-Net's level-0 conv2, passes bnl)
    return wg_late ? conv_wgrad(c, L, A, asc, ash, dy, dy_slot, accumulate) : 0;
  }
  // (statistics rows: colsum, unless the fused BatchNorm backward takes them)
  GConvArgs a = bind_conv(L.dgrad, dy, nullptr, nullptr, c.image(L.wd_off), nullptr, dA, colsum, c.kpart());
  const bool fused = fuse_bnbwd(c, a, bnl);
  if (int e = launch_conv_any(a, c.s)) return e;
  if (wg_late)
    if (int e = conv_wgrad(c, L, A, asc, ash, dy, dy_slot, accumulate)) return e;
  if (!fused) return 0;
  tag(bnl->name, "bnbwd");
  if (int e = finish_bn(c, *bnl, gconv_rows(a), a.CoutW, dA, training, accumulate)) return e;
  if (bn_done) *bn_done = true;
  return 0;
}

// BatchNorm+ReLU backward for layer L: dbuf holds d(post-activation) on entry
// and d(pre-BN y) on exit (unless pool_dP is given, in
// which case dbuf is produced from the max-pool gradient).
int bn_backward(const Ctx &c, const ConvLayer &L, float *dbuf, const float *pool_dP,
                const int *pool_k, int training, int accumulate) {
  tag(L.name, "bnbwd");
  const BNCoef coef = coef_at(c.sv, L.bn);
  const float *y = c.fptr(c.sv, L.y_off);
  const int64_t nvox = L.out.vox();
  const int R = bwd_rows(nvox, L.out.Cs);
  if (pool_dP) {
    if (int e = launch_bn_bwd_reduce_pool(pool_dP, y, coef, dbuf, L.out.B, L.out.X, L.out.Y,
                                          L.out.Z, L.out.Cs, pool_k[0], pool_k[1], pool_k[2],
                                          c.part(), R, c.s, c.bf()))
      return e;
  } else {
    if (int e = launch_bn_bwd_reduce_dense(dbuf, y, coef, nvox, L.out.Cs, c.part(), R, c.s,
                                           c.bf()))
      return e;
  }
  return finish_bn(c, L, R, L.bn.Cs, dbuf, training, accumulate);
}

}  // namespace hcu
