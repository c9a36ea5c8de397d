// Layer chains (include/hcunet.h, hcu_chain_*): a sequence of Conv3d [+ BN +
// ReLU] / MaxPool3d / ConvTranspose3d [+ cat(U, U)] ops with the network
// executor's kernels and fusions: BatchNorm+ReLU applied while the consumer
// stages its operand, BatchNorm statistics in the producing conv's epilogue,
// the BatchNorm backward reduction in the consumer dgrad's epilogue or fused
// with the max-pool backward.  Single stream, direct launches.
#include "exec.h"

using namespace hcu;

namespace {

struct ChainOp {
  int kind = 0;                  // HCU_CHAIN_CONV / POOL / CONVT
  bool bn_relu = false, fold = false;
  ConvLayer conv;
  ConvTLayer ct;
  int pk[3] = {1, 1, 1};
  Dims pooled;
  size_t pool_off = 0;
  int crop[3] = {0, 0, 0};       // ConvTranspose3d padding: crop of the full output (ConvTLayer::full)
  size_t xs_off = 0;             // s2b conv: the sub-lattice input (saved for the weight gradient)
};

struct ChainPlan : hcu_unet_plan {
  ChainPlan() : hcu_unet_plan(true) {}
  std::vector<ChainOp> chain;
  bool in_cl = false, out_cl = false;   // chain boundaries in the executor's layout (hcu_chain_spec)
  size_t ufull_off = 0, sub_off[3] = {};   // scratch: full ConvTranspose3d output, sub-lattice temporaries
  size_t max_sub = 0, max_ufull = 0;
};

// The handle as a chain plan; null (and the error set) for a null handle or a U-Net's.
const ChainPlan *as_chain(const hcu_unet_plan *p) {
  if (p && p->is_chain) return static_cast<const ChainPlan *>(p);
  fail(HCU_ERR_INVALID, "not a chain plan");
  return nullptr;
}

int build_chain(ChainPlan &p, const hcu_chain_spec &cs) {
  if (cs.n_ops < 1 || cs.n_ops > HCU_CHAIN_MAX_OPS) return fail(HCU_ERR_INVALID, "chain: 1..16 ops");
  if (cs.compute_dtype != HCU_F32 && cs.compute_dtype != HCU_BF16)
    return fail(HCU_ERR_INVALID, "compute_dtype must be HCU_F32 or HCU_BF16");
  if (cs.in_channels < 1) return fail(HCU_ERR_INVALID, "chain: in_channels must be positive");
  if (p.B < 1 || p.X < 1 || p.Y < 1 || p.Z < 1) return fail(HCU_ERR_SHAPE, "empty input");
  p.es = cs.compute_dtype == HCU_BF16 ? 2 : 4;
  p.bn_eps = cs.bn_eps;
  p.bn_momentum = cs.bn_momentum;
  const bool bf = p.es == 2;
  Region saved;
  p.xin = mkdims(p.B, p.X, p.Y, p.Z, cs.in_channels, p.es);
  p.in_cl = cs.in_cl != 0;
  p.out_cl = cs.out_cl != 0;
  if (cs.in_part_channels > 0) {
    if (!p.in_cl) return fail(HCU_ERR_INVALID, "chain: in_part_channels needs in_cl");
    if (cs.in_channels % cs.in_part_channels)
      return fail(HCU_ERR_INVALID, "chain: in_channels must be a multiple of in_part_channels");
    if (cs.ops[0].kind != HCU_CHAIN_CONV || cs.ops[0].groups != 1 || cs.ops[0].cat_fold)
      return fail(HCU_ERR_UNSUPPORTED, "chain: an input of channel parts needs a first Conv3d, groups 1");
    p.xin.part_c = cs.in_part_channels;
    p.xin.Cs = (cs.in_channels / cs.in_part_channels) * round_up(cs.in_part_channels, bf ? 8 : 4);
  }
  if (p.out_cl) {
    const hcu_chain_op &l = cs.ops[cs.n_ops - 1];
    if (l.kind != HCU_CHAIN_CONV || l.bn_relu)
      return fail(HCU_ERR_UNSUPPORTED, "chain: out_cl needs a last Conv3d without BatchNorm");
  }
  // (in_cl: the caller's tensor is the first op's input, nothing is copied)
  p.xcl_off = p.in_cl ? 0 : saved.take_floats(p.xin.floats());
  p.max_act = p.xin.floats();
  p.chain.assign(cs.n_ops, ChainOp{});
  // (the op list has its final size: the core's forward-order views)
  for (int i = 0; i < cs.n_ops; ++i) {
    if (cs.ops[i].kind == HCU_CHAIN_CONV) p.convs.push_back(&p.chain[i].conv);
    if (cs.ops[i].kind == HCU_CHAIN_CONVT) p.convts.push_back(&p.chain[i].ct);
  }
  Dims cur = p.xin;
  int prev = -1;
  bool prev_bn = false;
  int bn_index = 0;
  for (int i = 0; i < cs.n_ops; ++i) {
    const hcu_chain_op &s = cs.ops[i];
    ChainOp &o = p.chain[i];
    o.kind = s.kind;
    const std::string nm = "c" + std::to_string(i);
    if (s.kind == HCU_CHAIN_CONV) {
      o.bn_relu = s.bn_relu != 0;
      o.fold = s.cat_fold != 0;
      if (o.fold && prev != HCU_CHAIN_CONVT)
        return fail(HCU_ERR_INVALID, "chain: cat_fold needs a preceding ConvTranspose3d");
      const int cin_total = o.fold ? 2 * cur.C : cur.C;
      const int fold_mod = o.fold ? cur.C : cin_total;
      ConvLayer &L = o.conv;
      L.name = nm;
      if (int e = setup_conv(L, cur, s.out_channels, s.groups, fold_mod, cin_total, s.k, s.dil, "Conv3d",
                             true, s.stride, s.pad))
        return e;
      if (L.s2b && o.bn_relu)
        return fail(HCU_ERR_UNSUPPORTED, "chain: BatchNorm after a sub-lattice (large dilated) Conv3d");
      L.w_off = s.w_off;
      L.b_off = s.b_off;
      if (L.s2b) {
        o.xs_off = saved.take_floats(L.sub_in.floats());
        p.max_sub = std::max({p.max_sub, L.sub_in.floats(), L.sub_out.floats()});
      }
      // (out_cl: the last conv writes the caller's tensor and, without a
      // BatchNorm, its backward never reads y: no saved buffer)
      L.y_off = p.out_cl && i + 1 == cs.n_ops ? 0 : saved.take_floats(L.out.floats());
      L.bn.on = o.bn_relu;
      if (o.bn_relu) {
        L.bn.coef_off = saved.take_floats((size_t)6 * L.bn.Cs);
        L.bn.gamma = s.gamma_off;
        L.bn.beta = s.beta_off;
        L.bn.index = bn_index++;
      }
      track_conv(p, L);
      cur = L.out;
      prev_bn = o.bn_relu;
    } else if (s.kind == HCU_CHAIN_POOL) {
      if (!(prev == HCU_CHAIN_CONV && prev_bn))
        return fail(HCU_ERR_UNSUPPORTED, "chain: MaxPool3d must follow Conv3d + BatchNorm3d + ReLU");
      for (int d = 0; d < 3; ++d) {
        o.pk[d] = s.k[d];
        if (s.k[d] < 1) return fail(HCU_ERR_INVALID, "chain: bad pool kernel");
      }
      const int px = cur.X / o.pk[0], py = cur.Y / o.pk[1], pz = cur.Z / o.pk[2];
      if (px < 1 || py < 1 || pz < 1) return fail(HCU_ERR_SHAPE, "max_pool3d: Output size is too small");
      o.pooled = mkdims(p.B, px, py, pz, cur.C, p.es);
      o.pool_off = saved.take_floats(o.pooled.floats());
      p.max_act = std::max(p.max_act, o.pooled.floats());
      cur = o.pooled;
      prev_bn = false;
    } else if (s.kind == HCU_CHAIN_CONVT) {
      for (int d = 0; d < 3; ++d)
        if (s.dil[d] > 1) return fail(HCU_ERR_UNSUPPORTED, "ConvTranspose3d: dilation must be 1");
      if (s.groups > 1) return fail(HCU_ERR_UNSUPPORTED, "ConvTranspose3d: groups must be 1");
      ConvTLayer &u = o.ct;
      u.name = nm;
      const bool swap = bf && !prev_bn && !getenv("HCU_CONVT_NOSWAP");
      if (int e = setup_convt(u, cur, s.out_channels, s.k, s.stride, s.pad, swap, p.need)) return e;
      u.w_off = s.w_off;
      u.b_off = s.b_off;
      for (int d = 0; d < 3; ++d) o.crop[d] = s.pad[d];
      // (a cropped layer's forward writes the full output into scratch)
      if (o.crop[0] || o.crop[1] || o.crop[2]) p.max_ufull = std::max(p.max_ufull, u.full.floats());
      u.u_off = saved.take_floats(u.out.floats());
      p.max_act = std::max(p.max_act, u.out.floats());
      cur = u.out;
      prev_bn = false;
    } else {
      return fail(HCU_ERR_INVALID, "chain: unknown op kind");
    }
    prev = s.kind;
  }
  p.outd = cur;
  p.n_bn = bn_index;
  // weight re-layouts (one batched launch per forward), the last range of
  // `saved` (or the caller's image buffer: hcu_chain_forward_images)
  const size_t img0 = saved.off;
  p.prep_jobs.clear();
  for (ChainOp &o : p.chain) {
    if (o.kind == HCU_CHAIN_CONV) conv_prep(p, saved, o.conv);
    if (o.kind == HCU_CHAIN_CONVT) convt_prep(p, saved, o.ct);
  }
  split_prep(p);
  p.img_lo = img0;
  p.img_bytes = saved.off - img0;
  p.saved_bytes = saved.off;
  Region scratch = layout_scratch(p, HCU_NBUF_RING, (size_t)1 << 20, false);
  p.ufull_off = scratch.take_floats(p.max_ufull);
  for (size_t &o : p.sub_off) o = scratch.take_floats(p.max_sub);
  p.scratch_bytes = scratch.off;
  plan_log(p);
  return 0;
}

// Activation entering each op: (tensor, BatchNorm scale, shift) -- the
// producer's BatchNorm+ReLU is applied by the consumer while it loads.
struct ChainAct {
  const float *x = nullptr, *sc = nullptr, *sh = nullptr;
};

std::vector<ChainAct> chain_inputs(const ChainPlan &p, char *sv, const void *x, ChainAct *out_act) {
  std::vector<ChainAct> in(p.chain.size());
  ChainAct a;
  a.x = p.in_cl ? reinterpret_cast<const float *>(x) : reinterpret_cast<const float *>(sv + p.xcl_off);
  for (size_t i = 0; i < p.chain.size(); ++i) {
    const ChainOp &o = p.chain[i];
    in[i] = a;
    if (o.kind == HCU_CHAIN_CONV) {
      a.x = reinterpret_cast<const float *>(sv + o.conv.y_off);
      if (o.bn_relu) {
        const BNCoef cf = coef_at(sv, o.conv.bn);
        a.sc = cf.scale;
        a.sh = cf.shift;
      } else {
        a.sc = a.sh = nullptr;
      }
    } else if (o.kind == HCU_CHAIN_POOL) {
      a = ChainAct{reinterpret_cast<const float *>(sv + o.pool_off), nullptr, nullptr};
    } else {
      a = ChainAct{reinterpret_cast<const float *>(sv + o.ct.u_off), nullptr, nullptr};
    }
  }
  if (out_act) *out_act = a;
  return in;
}

// images: the caller's weight-image buffer (img_bytes) or null (in `saved`);
// images_current: 1 = it holds this plan's forward images of the current
// parameters, 2 = also the input-gradient ones (no re-layout then).
int enqueue_chain_forward(const ChainPlan &p, const hcu_unet_tensors *t, int training, hipStream_t s,
                          void *images = nullptr, int images_current = 0) {
  Ctx c(p, *t, s, nullptr, images);
  const int es = p.es, bf = c.bf();
  tag(std::string("chain"), "fwd");
  if (!p.in_cl)
    if (int e = launch_to_cl(t->x, c.fptr(c.sv, p.xcl_off), p.B, p.xin.C, p.xin.Cs, p.xin.vox() / p.B, s, bf,
                             t->x_dtype))
      return e;
  const std::vector<PrepJob> &jobs = training ? p.prep_jobs : p.prep_fwd;
  if (!jobs.empty() && images_current < (training ? 2 : 1))
    if (int e = c.prep(jobs, s)) return e;
  ChainAct last;
  const std::vector<ChainAct> in = chain_inputs(p, c.sv, t->x, &last);
  for (size_t i = 0; i < p.chain.size(); ++i) {
    const ChainOp &o = p.chain[i];
    const ChainAct &a = in[i];
    if (o.kind == HCU_CHAIN_CONV) {
      const ConvLayer &L = o.conv;
      // (out_cl: the last conv writes the caller's tensor; no op of this chain reads it back)
      float *y = p.out_cl && i + 1 == p.chain.size() ? t->out : c.fptr(c.sv, L.y_off);
      if (L.s2b) {
        float *xs = c.fptr(c.sv, o.xs_off), *ys = c.fptr(c.sc, p.sub_off[0]);
        const int sd[3] = {L.sub_in.X, L.sub_in.Y, L.sub_in.Z}, so[3] = {L.sub_out.X, L.sub_out.Y, L.sub_out.Z};
        tag(L.name, "fwd");
        if (int e = launch_s2b(a.x, a.sc, a.sh, xs, p.B, L.in.X, L.in.Y, L.in.Z, L.in.Cs, es, L.L3, sd, s))
          return e;
        if (int e = run_conv(L.fwd, xs, nullptr, nullptr, c.image(L.wf_off), c.param(L.b_off), ys, nullptr,
                             c.kpart(), s))
          return e;
        if (int e = launch_b2s(ys, y, p.B, L.out.X, L.out.Y, L.out.Z, L.out.Cs, es, L.L3, so, s)) return e;
      } else if (o.bn_relu) {
        if (int e = conv_forward(c, L, a.x, a.sc, a.sh, training)) return e;
      } else if (L.pw && !a.sc) {
        tag(L.name, "fwd");
        if (int e = launch_pw(pw_args(L, false, a.x, c.P + L.w_off, c.param(L.b_off), y), s)) return e;
      } else {
        tag(L.name, "fwd");
        if (int e = run_conv(L.fwd, a.x, a.sc, a.sh, c.image(L.wf_off), c.param(L.b_off), y, nullptr,
                             c.kpart(), s))
          return e;
      }
    } else if (o.kind == HCU_CHAIN_POOL) {
      const ConvLayer &P = p.chain[i - 1].conv;
      tag(P.name, "pool");
      if (int e = launch_maxpool_fwd(a.x, a.sc, a.sh, c.fptr(c.sv, o.pool_off), p.B, P.out.X, P.out.Y,
                                     P.out.Z, P.out.Cs, o.pk[0], o.pk[1], o.pk[2], s, bf))
        return e;
    } else {
      const ConvTLayer &u = o.ct;
      tag(u.name, "fwd");
      const bool crop = o.crop[0] || o.crop[1] || o.crop[2];
      float *U = crop ? c.fptr(c.sc, p.ufull_off) : c.fptr(c.sv, u.u_off);
      if (int e = convt_forward(c, u, a.x, a.sc, a.sh, U)) return e;
      if (crop) {
        const int sd[3] = {u.full.X, u.full.Y, u.full.Z}, dd[3] = {u.out.X, u.out.Y, u.out.Z};
        if (int e = launch_crop_cl(U, c.fptr(c.sv, u.u_off), p.B, sd, dd, o.crop, u.out.Cs, es, s)) return e;
      }
    }
  }
  tag(std::string("chain"), "out");
  if (!p.out_cl)
    if (int e = launch_from_cl_act(last.x, last.sc, last.sh, t->out, p.B, p.outd.C, p.outd.Cs,
                                   p.outd.vox() / p.B, s, bf))
      return e;
  if (training && p.n_bn && t->bn_num_batches_tracked)
    if (int e = launch_bn_count_increment(t->bn_num_batches_tracked, p.n_bn, s)) return e;
  if (timing_on()) timing_set_tag("");
  return HCU_OK;
}

int enqueue_chain_backward(const ChainPlan &p, const hcu_unet_tensors *t, const float *dout, float *dx,
                           int training, int accumulate, hipStream_t s, void *images = nullptr,
                           int images_current = 0) {
  Ctx c(p, *t, s, nullptr, images);
  const int es = p.es, bf = c.bf();
  const int n = (int)p.chain.size();
  const std::vector<ChainAct> in = chain_inputs(p, c.sv, t->x, nullptr);
  // an eval-mode forward prepared only the forward weight images
  if (!training && !p.prep_bwd.empty() && images_current < 2)
    if (int e = c.prep(p.prep_bwd, s)) return e;
  int cur = 0;
  if (int e = c.alloc(cur)) return e;
  tag(std::string("chain"), "bwd");
  // out_cl: dout is already in the layout (and the precision) of the gradient
  // slots, and the last op (a Conv3d without BatchNorm) only reads its output
  // gradient, so it reads the caller's tensor in place (a chain's backward
  // runs on `s` alone: every read is ordered before the caller's next use of
  // that memory on `s`).
  if (!p.out_cl)
    if (int e = launch_to_cl(dout, c.buf(cur), p.B, p.outd.C, p.outd.Cs, p.outd.vox() / p.B, s, bf, HCU_F32))
      return e;
  bool pre = false;   // buf(cur) already holds d(pre-BatchNorm y) of op i
  // Where op i's input gradient goes: a fresh slot, or for op 0 of an in_cl
  // chain the caller's dx, which is in the input's layout.
  auto take_dA = [&](int i, int &slot, float *&dA) -> int {
    dA = dx;
    if (i == 0 && p.in_cl) return 0;
    if (int e = c.alloc(slot)) return e;
    dA = c.buf(slot);
    return 0;
  };
  // Hands op i's input gradient on: op 0's to the caller's dx (a layout pass
  // unless it was written there), any other's becomes the current slot.
  auto pass_dA = [&](int i, const float *dA, int slot, bool is_pre) -> int {
    if (i == 0)
      return p.in_cl ? 0 : launch_from_cl(dA, dx, p.B, p.xin.C, p.xin.Cs, p.xin.vox() / p.B, s, bf);
    cur = slot;
    pre = is_pre;
    return 0;
  };
  for (int i = n - 1; i >= 0; --i) {
    const ChainOp &o = p.chain[i];
    const ChainAct &a = in[i];
    // the output gradient of op i
    float *dY = p.out_cl && i == n - 1 ? const_cast<float *>(dout) : c.buf(cur);
    const bool need_dA = i > 0 || dx != nullptr;
    const ChainOp *pr = i > 0 ? &p.chain[i - 1] : nullptr;
    if (o.kind == HCU_CHAIN_CONV) {
      const ConvLayer &L = o.conv;
      if (o.bn_relu && !pre)
        if (int e = bn_backward(c, L, c.buf(cur), nullptr, nullptr, training, accumulate)) return e;
      int sa = -1;
      float *dA = nullptr;
      if (need_dA) {
        if (!L.has_dgrad) return fail(HCU_ERR_UNSUPPORTED, "input gradient of a strided Conv3d");
        if (int e = take_dA(i, sa, dA)) return e;
      }
      bool done = false;
      if (L.s2b) {
        float *dys = c.fptr(c.sc, p.sub_off[1]), *dxs = c.fptr(c.sc, p.sub_off[2]);
        const int sd[3] = {L.sub_in.X, L.sub_in.Y, L.sub_in.Z}, so[3] = {L.sub_out.X, L.sub_out.Y, L.sub_out.Z};
        tag(L.name, "wgrad");
        if (int e = launch_s2b(dY, nullptr, nullptr, dys, p.B, L.out.X, L.out.Y, L.out.Z, L.out.Cs, es,
                               L.L3, so, s))
          return e;
        if (int e = conv_backward(c, L, c.fptr(c.sv, o.xs_off), nullptr, nullptr, dys, cur,
                                  need_dA ? dxs : nullptr, accumulate))
          return e;
        if (need_dA)
          if (int e = launch_b2s(dxs, dA, p.B, L.in.X, L.in.Y, L.in.Z, L.in.Cs, es, L.L3, sd, s)) return e;
      } else {
        const ConvLayer *bnl = (pr && pr->kind == HCU_CHAIN_CONV && pr->bn_relu) ? &pr->conv : nullptr;
        if (int e = conv_backward(c, L, a.x, a.sc, a.sh, dY, cur, dA, accumulate, bnl, training, &done))
          return e;
      }
      if (!need_dA) continue;
      if (int e = pass_dA(i, dA, sa, done)) return e;
    } else if (o.kind == HCU_CHAIN_POOL) {
      const ConvLayer &P = pr->conv;
      int sp = 0;
      if (int e = c.alloc(sp)) return e;
      if (int e = bn_backward(c, P, c.buf(sp), c.buf(cur), o.pk, training, accumulate)) return e;
      cur = sp;
      pre = true;
    } else {
      const ConvTLayer &u = o.ct;
      float *dU = c.buf(cur);
      tag(u.name, "wgrad");
      if (u.b_off >= 0) {
        const int R = chansum_rows(u.out.vox(), u.out.Cs);
        float *cs = nullptr;
        if (int e = c.slab((size_t)R * u.out.Cs, cs)) return e;
        if (int e = launch_chansum(dU, u.out.vox(), u.out.Cs, cs, R, s, bf)) return e;
        if (int e = c.pend_wgf(wgf_colsum(2, cs, R, u.out.Cs, u.Cout, c.G + u.b_off, accumulate))) return e;
      }
      if (u.wgs.on && !a.sc) {   // rows (tap, co) over dU, columns ci over x
        if (int e = run_wgrad(c, u.wgs, dU, nullptr, nullptr, a.x, c.G + u.w_off, nullptr, accumulate))
          return e;
      } else if (int e = run_wgrad(c, u.wg, a.x, a.sc, a.sh, dU, c.G + u.w_off, nullptr, accumulate)) {
        return e;
      }
      if (!need_dA) continue;
      tag(u.name, "dgrad");
      int sd = 0;
      float *dP = nullptr;
      if (int e = take_dA(i, sd, dP)) return e;
      const ConvLayer *bnl = (pr && pr->kind == HCU_CHAIN_CONV && pr->bn_relu) ? &pr->conv : nullptr;
      bool fused = false;
      if (int e = convt_dgrad(c, u, dU, dP, bnl, training, accumulate, fused)) return e;
      if (int e = pass_dA(i, dP, sd, fused)) return e;
    }
  }
  tag(std::string("wgrad"), "finalize");
  if (int e = c.flush_wgf()) return e;
  if (timing_on()) timing_set_tag("");
  return HCU_OK;
}

// The checks of a chain forward, then the enqueue.
int chain_forward(const ChainPlan *p, const hcu_unet_tensors *t, int training, hcu_stream_t stream, void *images,
                  int images_current) {
  if (int e = check_forward_tensors(*p, t)) return e;
  if (p->in_cl && t->x_dtype != (p->es == 2 ? HCU_BF16 : HCU_F32))
    return fail(HCU_ERR_INVALID, "chain: a channels-last input must be of the compute dtype");
  if (training)
    if (int e = check_bn_counts(*p)) return e;
  if (p->n_bn && (!t->bn_running_mean || !t->bn_running_var))
    return fail(HCU_ERR_INVALID, "BatchNorm running statistics missing");
  return enqueue_chain_forward(*p, t, training, (hipStream_t)stream, images, images_current);
}

}  // namespace

extern "C" {

int hcu_chain_plan_create(const hcu_chain_spec *spec, int B, int X, int Y, int Z, hcu_unet_plan **out) {
  if (!spec || !out) return fail(HCU_ERR_INVALID, "null argument");
  return create_plan<ChainPlan>(B, X, Y, Z, out, [&](ChainPlan &p) { return build_chain(p, *spec); });
}

int hcu_chain_plan_query(const hcu_unet_plan *plan, int64_t *out_shape, int *n_bn, size_t *saved_bytes,
                         size_t *scratch_bytes) {
  const ChainPlan *p = as_chain(plan);
  if (!p) return HCU_ERR_INVALID;
  if (out_shape) {
    out_shape[0] = p->B;
    out_shape[1] = p->outd.C;
    out_shape[2] = p->outd.X;
    out_shape[3] = p->outd.Y;
    out_shape[4] = p->outd.Z;
  }
  if (n_bn) *n_bn = p->n_bn;
  if (saved_bytes) *saved_bytes = p->saved_bytes;
  if (scratch_bytes) *scratch_bytes = p->scratch_bytes;
  return HCU_OK;
}

int hcu_chain_forward(const hcu_unet_plan *plan, const hcu_unet_tensors *t, int training, hcu_stream_t stream) {
  const ChainPlan *p = as_chain(plan);
  if (!p) return HCU_ERR_INVALID;
  return chain_forward(p, t, training, stream, nullptr, 0);
}

int hcu_chain_backward(const hcu_unet_plan *p, const hcu_unet_tensors *t, const float *dout, float *dx,
                       int training, int accumulate, hcu_stream_t stream) {
  return hcu_chain_backward_images(p, t, dout, dx, training, accumulate, stream, nullptr, 0);
}

size_t hcu_chain_weight_image_bytes(const hcu_unet_plan *plan) {
  const ChainPlan *p = as_chain(plan);
  return p ? p->img_bytes : 0;
}

int hcu_chain_forward_images(const hcu_unet_plan *plan, const hcu_unet_tensors *t, int training,
                             hcu_stream_t stream, void *images, int images_current) {
  const ChainPlan *p = as_chain(plan);
  if (!p) return HCU_ERR_INVALID;
  if (!images) return fail(HCU_ERR_INVALID, "null weight-image buffer");
  if (images_current < 0 || images_current > 2) return fail(HCU_ERR_INVALID, "images_current must be 0, 1 or 2");
  return chain_forward(p, t, training, stream, images, images_current);
}

int hcu_chain_backward_images(const hcu_unet_plan *plan, const hcu_unet_tensors *t, const float *dout, float *dx,
                              int training, int accumulate, hcu_stream_t stream, void *images,
                              int images_current) {
  const ChainPlan *p = as_chain(plan);
  if (!p) return HCU_ERR_INVALID;
  if (!t || !dout || !t->grads || !t->params || !t->saved || !t->scratch)
    return fail(HCU_ERR_INVALID, "null argument");
  return enqueue_chain_backward(*p, t, dout, dx, training, accumulate, (hipStream_t)stream, images, images_current);
}

}  // extern "C"
