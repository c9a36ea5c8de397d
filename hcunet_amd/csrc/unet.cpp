// Native executor for the 3D U-Net training hot path: the U-Net plan, its
// builder, and the forward / backward that enqueue one fixed kernel sequence
// on the caller's stream (no allocation, no host sync: capturable into a
// hipGraph).  The backward runs its weight gradients on a branch stream; a
// small plan's forward is replayed from a captured graph (exec.h).
//
// The decoder's cat(U, U) (crop returns U itself, hcat/unet.py:311-312,
// 319-340) is folded into Up.conv1's weights: conv(cat(U,U), W) ==
// conv(U, W[:, :C] + W[:, C:]) (per group), halving that layer's work; the
// weight gradient is scattered back to both halves.
#include "exec.h"

using namespace hcu;

namespace {

struct UnetPlan : hcu_unet_plan {
  UnetPlan() : hcu_unet_plan(false) {}
  hcu_unet_spec spec;
  int L = 0;
  int flags = 0;       // HCU_PLAN_FORWARD_ONLY: activations in two ping-pong buffers
  std::vector<ConvLayer> dc1, dc2, uc1, uc2;
  // the first convolution stages the NCXYZ input itself (conv8, or bconv
  // with one channel group; <= 4 input channels, groups 1): no channels-last
  // layout pass, and its kernel reads t->x
  bool ncx_first = false;
  std::vector<Dims> pooled;
  std::vector<size_t> pool_off;
  std::vector<ConvTLayer> up;
  int64_t oc_w = 0, oc_b = 0;
  int Co = 0;
  int64_t n_params = 0;
  // per decoder level: the column-sum rows of dU (the up_conv bias gradient)
  // written by the folded conv1's input-gradient kernel
  size_t colsum_off[HCU_MAX_LEVELS] = {};
  double fwd_flops = 0.0;   // forward convolution FLOPs (graph replay only below 100 GFLOP)
  // data-parallel overlap (hcu_unet_set_grad_events): caller-owned events the
  // backward records when the decoder's / the deep encoder levels' gradients are final
  hipEvent_t grad_ev[2] = {nullptr, nullptr};
  int grad_deep = -1;
  // (used through the const handle the entry points take; the graph cache is
  // destroyed before the branch)
  mutable Branch branch;
  mutable GraphCache graphs;
};

// The handle as a U-Net plan; null for a null handle or a chain's.
const UnetPlan *as_unet(const hcu_unet_plan *p) {
  return p && !p->is_chain ? static_cast<const UnetPlan *>(p) : nullptr;
}

int build_plan(UnetPlan &p) {
  const hcu_unet_spec &s = p.spec;
  const int L = s.levels;
  if (L < 2 || L > HCU_MAX_LEVELS)
    return fail(HCU_ERR_INVALID, "The Number of Features must be at least 2");
  for (int i = 0; i + 1 < L; ++i)
    if (s.features[i] * 2 != s.features[i + 1])
      return fail(HCU_ERR_INVALID, "Feature Sizes must be multiples of two from each other");
  if (s.in_channels < 1 || s.out_channels < 1 || s.features[0] < 1)
    return fail(HCU_ERR_INVALID, "channel counts must be positive");
  if (p.B < 1 || p.X < 1 || p.Y < 1 || p.Z < 1) return fail(HCU_ERR_SHAPE, "empty input");
  for (int i = 0; i < 3; ++i)
    if (s.pool_k[i] < 1 || s.up_k[i] < 1 || s.up_s[i] < 1)
      return fail(HCU_ERR_INVALID, "bad pool/upsample kernel");
  p.L = L;
  p.bn_eps = s.bn_eps;
  p.bn_momentum = s.bn_momentum;
  p.dc1.resize(L);
  p.dc2.resize(L);
  p.pooled.resize(L);
  p.pool_off.resize(L);
  p.up.resize(L - 1);
  p.uc1.resize(L - 1);
  p.uc2.resize(L - 1);
  // (the vectors have their final size: the core's forward-order views)
  for (int i = 0; i < L; ++i) p.convs.insert(p.convs.end(), {&p.dc1[i], &p.dc2[i]});
  for (int j = 0; j < L - 1; ++j) {
    p.convts.push_back(&p.up[j]);
    p.convs.insert(p.convs.end(), {&p.uc1[j], &p.uc2[j]});
  }

  // Parameter offsets in Unet_Constructor.parameters() order (hcat/unet.py:87-123:
  // out_conv, then down_steps[i].{conv1,conv2,batch1,batch2}, then
  // up_steps[j].{conv1,conv2,up_conv,batch1,batch2}).
  int64_t off = 0;
  const int f0 = s.features[0];
  p.Co = s.out_channels;
  p.oc_w = off; off += (int64_t)p.Co * f0;
  p.oc_b = off; off += p.Co;
  const int T1 = s.k1[0] * s.k1[1] * s.k1[2], T2 = s.k2[0] * s.k2[1] * s.k2[2];
  const int Tu = s.up_k[0] * s.up_k[1] * s.up_k[2];
  int bn_index = 0;
  for (int i = 0; i < L; ++i) {
    const int cin = i == 0 ? s.in_channels : s.features[i - 1];
    const int f = s.features[i];
    if (cin % s.g1 || f % s.g1 || f % s.g2)
      return fail(HCU_ERR_INVALID, "in_channels/out_channels must be divisible by groups");
    ConvLayer &c1 = p.dc1[i], &c2 = p.dc2[i];
    c1.name = "d" + std::to_string(i) + ".c1";
    c2.name = "d" + std::to_string(i) + ".c2";
    c1.w_off = off; off += (int64_t)f * (cin / s.g1) * T1;
    c1.b_off = off; off += f;
    c2.w_off = off; off += (int64_t)f * (f / s.g2) * T2;
    c2.b_off = off; off += f;
    c1.bn.gamma = off; off += f;
    c1.bn.beta = off; off += f;
    c2.bn.gamma = off; off += f;
    c2.bn.beta = off; off += f;
    c1.bn.index = bn_index++;
    c2.bn.index = bn_index++;
  }
  for (int j = 0; j < L - 1; ++j) {
    const int f = s.features[L - 1 - j], o = s.features[L - 2 - j];
    if (f % s.g1 || o % s.g1 || o % s.g2)
      return fail(HCU_ERR_INVALID, "in_channels/out_channels must be divisible by groups");
    ConvLayer &c1 = p.uc1[j], &c2 = p.uc2[j];
    ConvTLayer &u = p.up[j];
    c1.name = "u" + std::to_string(j) + ".c1";
    c2.name = "u" + std::to_string(j) + ".c2";
    u.name = "u" + std::to_string(j) + ".up";
    c1.w_off = off; off += (int64_t)o * (f / s.g1) * T1;
    c1.b_off = off; off += o;
    c2.w_off = off; off += (int64_t)o * (o / s.g2) * T2;
    c2.b_off = off; off += o;
    u.w_off = off; off += (int64_t)f * o * Tu;
    u.b_off = off; off += o;
    c1.bn.gamma = off; off += o;
    c1.bn.beta = off; off += o;
    c2.bn.gamma = off; off += o;
    c2.bn.beta = off; off += o;
    c1.bn.index = bn_index++;
    c2.bn.index = bn_index++;
  }
  for (ConvLayer *c : p.convs) c->bn.on = true;
  p.n_params = off;
  p.n_bn = bn_index;

  // Shapes, forward order.
  Region saved;
  // Activation tensors in forward order.  A forward-only plan keeps none of them
  // for a backward: every forward op reads only the tensor the previous op
  // wrote (the skip tensors are shape checks only, hcat/unet.py:309-315), so
  // they alternate between two buffers of the largest activation.
  const bool fwd_only = (p.flags & HCU_PLAN_FORWARD_ONLY) != 0;
  std::vector<std::pair<size_t *, size_t>> acts;
  auto act_take = [&](size_t floats, size_t &off) {
    if (fwd_only)
      acts.emplace_back(&off, floats);
    else
      off = saved.take_floats(floats);
  };
  if (s.compute_dtype != HCU_F32 && s.compute_dtype != HCU_BF16)
    return fail(HCU_ERR_INVALID, "compute_dtype must be HCU_F32 or HCU_BF16");
  p.es = s.compute_dtype == HCU_BF16 ? 2 : 4;
  p.xin = mkdims(p.B, p.X, p.Y, p.Z, s.in_channels, p.es);
  act_take(p.xin.floats(), p.xcl_off);
  p.max_act = p.xin.floats();
  Dims cur = p.xin;
  for (int i = 0; i < L; ++i) {
    const int cin = cur.C, f = s.features[i];
    if (int e = setup_conv(p.dc1[i], cur, f, s.g1, cin, cin, s.k1, s.d1, "down conv1")) return e;
    if (int e = setup_conv(p.dc2[i], p.dc1[i].out, f, s.g2, f, f, s.k2, s.d2, "down conv2")) return e;
    for (ConvLayer *c : {&p.dc1[i], &p.dc2[i]}) {
      act_take(c->out.floats(), c->y_off);
      c->bn.coef_off = saved.take_floats((size_t)6 * c->bn.Cs);
      track_conv(p, *c);
    }
    cur = p.dc2[i].out;
    if (i < L - 1) {
      const int px = cur.X / s.pool_k[0], py = cur.Y / s.pool_k[1], pz = cur.Z / s.pool_k[2];
      if (px < 1 || py < 1 || pz < 1)
        return fail(HCU_ERR_SHAPE, "max_pool3d: Output size is too small");
      p.pooled[i] = mkdims(p.B, px, py, pz, f, p.es);
      act_take(p.pooled[i].floats(), p.pool_off[i]);
      p.max_act = std::max(p.max_act, p.pooled[i].floats());
      cur = p.pooled[i];
    }
  }
  for (int j = 0; j < L - 1; ++j) {
    const int level = L - 2 - j;
    const int f = s.features[L - 1 - j], o = s.features[L - 2 - j];
    ConvTLayer &u = p.up[j];
    if (int e = setup_convt(u, cur, o, s.up_k, s.up_s, nullptr, false, p.need)) return e;
    const Dims &skip = p.dc2[level].out;
    if (u.out.X > skip.X || u.out.Y > skip.Y || u.out.Z > skip.Z)
      return fail(HCU_ERR_SHAPE,
                  "Sizes of tensors must match except in dimension 1 (upsampled " +
                      std::to_string(u.out.X) + "x" + std::to_string(u.out.Y) + "x" +
                      std::to_string(u.out.Z) + " exceeds skip " + std::to_string(skip.X) + "x" +
                      std::to_string(skip.Y) + "x" + std::to_string(skip.Z) + ")");
    act_take(u.out.floats(), u.u_off);
    p.max_act = std::max(p.max_act, u.out.floats());
    // conv1 consumes cat(U, U): fold (cat channels 2*o, effective o)
    if (int e = setup_conv(p.uc1[j], u.out, o, s.g1, o, f, s.k1, s.d1, "up conv1")) return e;
    if (int e = setup_conv(p.uc2[j], p.uc1[j].out, o, s.g2, o, o, s.k2, s.d2, "up conv2")) return e;
    for (ConvLayer *c : {&p.uc1[j], &p.uc2[j]}) {
      act_take(c->out.floats(), c->y_off);
      c->bn.coef_off = saved.take_floats((size_t)6 * c->bn.Cs);
      track_conv(p, *c);
    }
    cur = p.uc2[j].out;
  }
  if (p.Co > 4) return fail(HCU_ERR_UNSUPPORTED, "out_channels > 4 is not supported yet");
  {
    // The first convolution reads the NCXYZ volume itself in fp32 plans; bf16
    // plans keep the separate channels-last pass (to_cl_vox) ahead of it: the
    // NCXYZ gather issues one 4-byte load per channel plane and element, and
    // config 3 ran 6.345-6.349 ms/step with it against 6.269-6.275 without
    // (interleaved, round 6).  HCU_NCX=0 / 1 forces either (A/B).
    static const int ncx_env = getenv("HCU_NCX") ? (getenv("HCU_NCX")[0] == '1' ? 1 : 0) : -1;
    const bool ncx_on = ncx_env >= 0 ? ncx_env == 1 : p.es == 4;
    const GConvArgs &f = p.dc1[0].fwd;
    const auto ncx_ok = conv_family(f).ncx_ok;
    p.ncx_first = ncx_on && s.in_channels <= 4 && s.g1 == 1 && ncx_ok && ncx_ok(f);
  }
  p.outd = mkdims(p.B, cur.X, cur.Y, cur.Z, p.Co, 4);
  {
    const int R = outconv_bwd_rows(cur.vox(), cur.Cs);
    p.need.rows((size_t)R * cur.Cs * 2 + (size_t)R * (p.Co * cur.Cs + p.Co) + 64);
  }
  p.prep_jobs.clear();
  for (int i = 0; i < L; ++i) {
    conv_prep(p, saved, p.dc1[i]);
    conv_prep(p, saved, p.dc2[i]);
  }
  for (int j = 0; j + 1 < L; ++j) {
    conv_prep(p, saved, p.uc1[j]);
    conv_prep(p, saved, p.uc2[j]);
    convt_prep(p, saved, p.up[j]);
  }
  split_prep(p);
  if (fwd_only) {
    size_t mx = 1;
    for (const auto &a : acts) mx = std::max(mx, a.second);
    const size_t pp[2] = {saved.take_floats(mx), saved.take_floats(mx)};
    for (size_t k = 0; k < acts.size(); ++k) *acts[k].first = pp[k & 1];
  }
  p.saved_bytes = saved.off;
  // forward convolution FLOPs: decides graph replay vs direct launches
  p.fwd_flops = 0.0;
  for (const ConvLayer *cl : p.convs)
    p.fwd_flops += 2.0 * cl->fwd.B * cl->fwd.OX * cl->fwd.OY * cl->fwd.OZ * (double)cl->Cout * cl->Cin_g * cl->T;

  // a U-Net backward allocates 1 + 3 slots per decoder level + at most 3 per
  // encoder level: one slot each when that stays within 32 slots and 24 GB
  const int need = 1 + 3 * (L - 1) + 3 * L;
  p.no_reuse = !fwd_only && need <= HCU_NBUF && (double)need * p.max_act * 4.0 <= 24e9;
  Region scratch = layout_scratch(p, p.no_reuse ? need : HCU_NBUF_RING, (size_t)8 << 20, fwd_only);
  for (int j = 0; j + 1 < L; ++j)
    p.colsum_off[j] = scratch.take_floats(fwd_only ? 0 : (size_t)gconv_rows(p.uc1[j].dgrad) * p.uc1[j].dgrad.CoutW * 4);
  p.scratch_bytes = scratch.off;
  plan_log(p);
  return 0;
}

// hipGraph replay of the captured sequences vs direct launches.  On MI355X /
// ROCm 7 a replayed kernel node costs ~1.5 us more on the GPU than a direct
// launch (config 3: 7.24 vs 7.10 ms per step), but a direct launch costs the
// host ~10 us: at config 2 (2.3 ms of GPU work, 1.7 ms of host enqueue) direct
// launches ran 2.31..3.34 ms per step depending on host jitter, graphs a
// steady 2.51..2.58.  So: graphs for the forward of plans under 100 GFLOP,
// direct launches otherwise; HCU_GRAPHS=0 / 1 forces either everywhere.
int graphs_forced() {
  static const int v = [] {
    const char *e = getenv("HCU_GRAPHS");
    return e ? (e[0] == '1' ? 1 : 0) : -1;
  }();
  return v;
}
// The backward (two streams joined by events) replays slower still: a graph
// of it cost 0.17 ms per config-2 step against direct launches (forward-only
// graph 2.39 ms/step vs both graphed 2.56, three interleaved A/B runs), so by
// default only a small plan's forward is replayed.
bool graphs_for(const UnetPlan &p, bool backward) {
  const int f = graphs_forced();
  if (f >= 0) return f == 1;
  return !backward && p.fwd_flops < 100e9;
}

void append_bn_key(std::vector<uintptr_t> &key, const UnetPlan &p, const hcu_unet_tensors *t) {
  for (int i = 0; i < p.n_bn; ++i) {
    key.push_back(t->bn_running_mean ? (uintptr_t)t->bn_running_mean[i] : 0);
    key.push_back(t->bn_running_var ? (uintptr_t)t->bn_running_var[i] : 0);
    key.push_back(t->bn_num_batches_tracked ? (uintptr_t)t->bn_num_batches_tracked[i] : 0);
  }
}

// Replays the plan's captured sequence for `key` (key[0]: 0 forward, 1
// backward); direct launches when graphs are off or per-launch timing is on.
template <class F>
int run_graphed(const UnetPlan &p, const std::vector<uintptr_t> &key, hipStream_t s, F enqueue) {
  if (!graphs_for(p, key[0] != 0) || timing_on()) return enqueue(s);
  return p.graphs.run(key, s, p.branch, enqueue);
}

// part: 0 = the whole forward; 1 = its head (the input's channels-last
// layout, or with ncx_first the first convolution reading the NCXYZ input
// itself, and its BatchNorm finalize): the launches that read t->x, issued
// directly ahead of a replayed graph of part 2 = the rest, so a new input
// tensor every step (a data loader) does not key a new graph.
int enqueue_forward(const UnetPlan &p, const hcu_unet_tensors *t, int training, hipStream_t stream,
                    int part = 0, bool split = false) {
  Ctx c(p, *t, stream, split ? &p.branch : nullptr);
  const hcu_unet_spec &s = p.spec;
  float *xcl = c.fptr(c.sv, p.xcl_off);
  if (part != 2) {
    tag(std::string("in"), "fwd");
    if (!p.ncx_first) {
      if (int e = launch_to_cl(t->x, xcl, p.B, p.xin.C, p.xin.Cs, p.xin.vox() / p.B, c.s, c.bf(),
                               t->x_dtype))
        return e;
    } else {
      // NCXYZ input staged by the first conv; the channels-last copy only
      // where a backward will read it
      const int fmt = t->x_dtype == HCU_F16 ? 2 : t->x_dtype == HCU_BF16 ? 3 : 1;
      float *xo = (p.flags & HCU_PLAN_FORWARD_ONLY) ? nullptr : xcl;
      if (int e = conv_forward(c, p.dc1[0], t->x, nullptr, nullptr, training, fmt, xo)) return e;
    }
    if (part == 1) return HCU_OK;
  }
  tag(std::string("prep"), "fwd");
  // training forwards lay out the input-gradient weight images too; laying
  // them out on the backward's branch instead measured equal on config 3 and
  // ~10 us slower on config 2.  A split forward (hcu_unet_forward) lays out
  // level 0's forward images on the chain and every other image on the
  // branch, which the chain waits for only before level 1.
  const size_t n0 = std::min<size_t>(2, p.prep_fwd.size());   // d0.c1, d0.c2 (job order)
  hipEvent_t ev_rest = nullptr;
  if (split && training) {
    if (int e = c.fork()) return e;
    if (p.prep_fwd.size() > n0) {
      if (int e = c.prep(p.prep_fwd.data() + n0, p.prep_fwd.size() - n0, c.ws)) return e;
      ev_rest = p.branch.next_marker();
      HCU_HIP(hipEventRecord(ev_rest, c.ws));
    }
    if (!p.prep_bwd.empty())
      if (int e = c.prep(p.prep_bwd, c.ws)) return e;
    if (int e = c.prep(p.prep_fwd.data(), n0, c.s)) return e;
  } else {
    if (training && !p.prep_bwd.empty()) {
      if (int e = c.fork()) return e;
      if (int e = c.prep(p.prep_bwd, c.wstream())) return e;
    }
    if (int e = c.prep(p.prep_fwd, c.s)) return e;
  }
  const float *src = xcl;
  const float *ssc = nullptr, *ssh = nullptr;
  for (int i = 0; i < p.L; ++i) {
    const ConvLayer &c1 = p.dc1[i], &c2 = p.dc2[i];
    if (i == 1 && ev_rest) HCU_HIP(hipStreamWaitEvent(c.s, ev_rest, 0));
    if (!(i == 0 && p.ncx_first))   // (else: run in the head)
      if (int e = conv_forward(c, c1, src, ssc, ssh, training)) return e;
    const BNCoef b1 = coef_at(c.sv, c1.bn);
    if (int e = conv_forward(c, c2, c.fptr(c.sv, c1.y_off), b1.scale, b1.shift, training)) return e;
    const BNCoef b2 = coef_at(c.sv, c2.bn);
    if (i < p.L - 1) {
      float *pp = c.fptr(c.sv, p.pool_off[i]);
      tag(c2.name, "pool");
      if (int e = launch_maxpool_fwd(c.fptr(c.sv, c2.y_off), b2.scale, b2.shift, pp, p.B,
                                     c2.out.X, c2.out.Y, c2.out.Z, c2.out.Cs, s.pool_k[0],
                                     s.pool_k[1], s.pool_k[2], c.s, c.bf()))
        return e;
      src = pp;
      ssc = ssh = nullptr;
    } else {
      src = c.fptr(c.sv, c2.y_off);
      ssc = b2.scale;
      ssh = b2.shift;
    }
  }
  for (int j = 0; j < p.L - 1; ++j) {
    const ConvTLayer &u = p.up[j];
    tag(u.name, "fwd");
    float *U = c.fptr(c.sv, u.u_off);
    if (int e = convt_forward(c, u, src, ssc, ssh, U)) return e;
    const ConvLayer &c1 = p.uc1[j], &c2 = p.uc2[j];
    if (int e = conv_forward(c, c1, U, nullptr, nullptr, training)) return e;
    const BNCoef b1 = coef_at(c.sv, c1.bn);
    if (int e = conv_forward(c, c2, c.fptr(c.sv, c1.y_off), b1.scale, b1.shift, training)) return e;
    const BNCoef b2 = coef_at(c.sv, c2.bn);
    src = c.fptr(c.sv, c2.y_off);
    ssc = b2.scale;
    ssh = b2.shift;
  }
  const ConvLayer &last = p.L > 1 ? p.uc2[p.L - 2] : p.dc2[0];
  tag(std::string("out"), "fwd");
  if (int e = launch_outconv_fwd(src, coef_at(c.sv, last.bn), c.P + p.oc_w, c.P + p.oc_b, t->out,
                                 p.B, last.out.vox() / p.B, last.out.C, last.out.Cs, p.Co, c.s,
                                 c.bf()))
    return e;
  if (training && t->bn_num_batches_tracked)
    if (int e = launch_bn_count_increment(t->bn_num_batches_tracked, p.n_bn, c.s)) return e;
  if (int e = c.join()) return e;
  if (timing_on()) timing_set_tag("");
  return HCU_OK;
}

int enqueue_backward(const UnetPlan &p, const hcu_unet_tensors *t, const float *dout, float *dx,
                     int training, int accumulate, hipStream_t stream, bool split, bool record_grad_events) {
  const hcu_unet_spec &s = p.spec;
  Ctx c(p, *t, stream, split ? &p.branch : nullptr);
  c.arm_chain();
  // an eval-mode forward prepared only the forward weight images: the
  // input-gradient images are laid out here
  if (!training && !p.prep_bwd.empty())
    if (int e = c.prep(p.prep_bwd, c.s)) return e;
  int cur = 0;  // slot holding the current d(pre-BN y)
  if (int e = c.alloc(cur)) return e;

  // out_conv + last BatchNorm
  const ConvLayer &last = p.uc2[p.L - 2];
  tag(std::string("out"), "bwd");
  {
    const BNCoef coef = coef_at(c.sv, last.bn);
    const int64_t nvox = last.out.vox();
    const int R = outconv_bwd_rows(nvox, last.out.Cs);
    float *part_bn = c.part();
    float *part_oc = part_bn + (size_t)R * last.out.Cs * 2;
    if (int e = launch_outconv_bwd(dout, c.fptr(c.sv, last.y_off), coef, c.P + p.oc_w, c.buf(cur),
                                   p.B, nvox / p.B, last.out.C, last.out.Cs, p.Co, part_bn, part_oc,
                                   R, c.s, c.bf()))
      return e;
    if (int e = launch_outconv_wfinalize(part_oc, R, p.Co, last.out.C, last.out.Cs, c.G + p.oc_w,
                                         c.G + p.oc_b, accumulate, c.s))
      return e;
    if (int e = finish_bn(c, last, R, last.bn.Cs, c.buf(cur), training, accumulate)) return e;
  }
  // decoder, last to first
  for (int j = p.L - 2; j >= 0; --j) {
    const ConvLayer &c1 = p.uc1[j], &c2 = p.uc2[j];
    const ConvTLayer &u = p.up[j];
    const BNCoef b1 = coef_at(c.sv, c1.bn);
    const float *U = c.fptr(c.sv, u.u_off);
    int sb = 0, su = 0, sd = 0;
    // conv2 (+ BatchNorm/ReLU backward of conv1, fused into its dgrad when possible)
    if (int e = c.alloc(sb)) return e;
    float *A = c.buf(cur), *Bf = c.buf(sb);
    bool done1 = false;
    if (int e = conv_backward(c, c2, c.fptr(c.sv, c1.y_off), b1.scale, b1.shift, A, cur, Bf,
                              accumulate, &c1, training, &done1))
      return e;
    if (!done1)
      if (int e = bn_backward(c, c1, Bf, nullptr, nullptr, training, accumulate)) return e;
    // conv1 (folded cat): dU into a fresh slot; its input-gradient kernel also
    // writes the column-sum rows of dU, the up_conv bias gradient
    if (int e = c.alloc(su)) return e;
    float *dU = c.buf(su);
    const int cs_rows = gconv_rows(c1.dgrad), cs_w = c1.dgrad.CoutW;
    // (its own scratch region per level: written by the chain, read by the
    // deferred finalize on the branch -- never a recycled slab of the arena,
    // whose previous readers run on the branch)
    float *csr = c.fptr(c.sc, p.colsum_off[j]);
    if (int e = conv_backward(c, c1, U, nullptr, nullptr, Bf, sb, dU, accumulate, nullptr, training, nullptr, csr))
      return e;
    // up_conv: bias and weight gradients on the branch, input gradient on the chain
    const ConvLayer &prev = j == 0 ? p.dc2[p.L - 1] : p.uc2[j - 1];
    const BNCoef bp = coef_at(c.sv, prev.bn);
    tag(u.name, "wgrad");
    if (int e = c.fork()) return e;
    // the bias: column sums of dU, with the batched finalizes
    if (int e = c.pend_wgf(wgf_colsum(4, csr, cs_rows, cs_w, u.Cout, c.G + u.b_off, accumulate))) return e;
    // the weight gradient: in one launch (WGradArgs::nph, wgrad3) where planned, else per tap
    if (int e = run_wgrad(c, u.wgp.on ? u.wgp : u.wg, c.fptr(c.sv, prev.y_off), bp.scale, bp.shift, dU,
                          c.G + u.w_off, nullptr, accumulate))
      return e;
    if (int e = c.read_done(su)) return e;
    tag(u.name, "dgrad");
    if (int e = c.alloc(sd)) return e;
    bool fused = false;
    if (int e = convt_dgrad(c, u, dU, c.buf(sd), &prev, training, accumulate, fused)) return e;
    if (!fused)
      if (int e = bn_backward(c, prev, c.buf(sd), nullptr, nullptr, training, accumulate)) return e;
    cur = sd;
  }
  // Data-parallel overlap: every gradient of a finished group is written by
  // the finalizes pending on the branch and by kernels the main chain issued
  // before this point; the branch flushes, joins the chain (fork) and records.
  // (not in a captured backward: a record inside stream capture is only a
  // capture dependency, a replay would never record the caller's events)
  auto grads_ready = [&](hipEvent_t ev) -> int {
    if (!ev || !record_grad_events) return 0;
    if (int e = c.flush_wgf()) return e;
    if (int e = c.fork()) return e;
    HCU_HIP(hipEventRecord(ev, c.wstream()));
    return 0;
  };
  if (int e = grads_ready(p.grad_ev[0])) return e;   // up_steps + out_conv
  // encoder, bottleneck to first
  for (int i = p.L - 1; i >= 0; --i) {
    const ConvLayer &c1 = p.dc1[i], &c2 = p.dc2[i];
    const BNCoef b1 = coef_at(c.sv, c1.bn);
    int sb = 0, sa = -1;
    if (int e = c.alloc(sb)) return e;
    float *A = c.buf(cur), *Bf = c.buf(sb);
    bool done1 = false;
    static const int l0_order = getenv("HCU_L0_ORDER") ? atoi(getenv("HCU_L0_ORDER")) : 0;
    if (int e = conv_backward(c, c2, c.fptr(c.sv, c1.y_off), b1.scale, b1.shift, A, cur, Bf,
                              accumulate, &c1, training, &done1, nullptr, i == 0 && l0_order == 1))
      return e;
    if (!done1)
      if (int e = bn_backward(c, c1, Bf, nullptr, nullptr, training, accumulate)) return e;
    const float *in = i == 0 ? c.fptr(c.sv, p.xcl_off) : c.fptr(c.sv, p.pool_off[i - 1]);
    float *dIn = nullptr;
    if (i > 0 || dx) {
      if (int e = c.alloc(sa)) return e;
      dIn = c.buf(sa);
    }
    if (int e = conv_backward(c, c1, in, nullptr, nullptr, Bf, sb, dIn, accumulate, nullptr, training))
      return e;
    if (i > 0) {
      // dIn = d(pooled): produce d(pre-BN y2_{i-1}) into a fresh slot
      int sp = 0;
      if (int e = c.alloc(sp)) return e;
      if (int e = bn_backward(c, p.dc2[i - 1], c.buf(sp), dIn, s.pool_k, training, accumulate))
        return e;
      cur = sp;
    } else if (dx) {
      if (int e = launch_from_cl(dIn, dx, p.B, p.xin.C, p.xin.Cs, p.xin.vox() / p.B, c.s, c.bf()))
        return e;
    }
    // levels >= i: both convs' weight gradients and every BatchNorm of theirs
    // (dc2[i]'s in level i+1's pooled backward, or the decoder's) are final
    if (i == p.grad_deep && i > 0)
      if (int e = grads_ready(p.grad_ev[1])) return e;
  }
  tag(std::string("wgrad"), "finalize");
  if (int e = c.fork()) return e;   // (the last weight gradient may have run half on the chain)
  if (int e = c.flush_wgf()) return e;
  if (int e = c.join()) return e;
  if (timing_on()) timing_set_tag("");
  return HCU_OK;
}

// Takes the branch for this call when `split`: one user of its stream and
// events at a time, created on the current device.
int take_branch(const UnetPlan &p, bool split, std::unique_lock<std::mutex> &lk) {
  if (!split) return HCU_OK;
  lk.lock();
  int dev = 0;
  HCU_HIP(hipGetDevice(&dev));
  return p.branch.ensure(dev);
}

}  // namespace

extern "C" {

int hcu_unet_plan_create(const hcu_unet_spec *spec, int B, int X, int Y, int Z,
                         hcu_unet_plan **out) {
  return hcu_unet_plan_create_ex(spec, B, X, Y, Z, 0, out);
}

int hcu_unet_plan_create_ex(const hcu_unet_spec *spec, int B, int X, int Y, int Z, int flags,
                            hcu_unet_plan **out) {
  if (!spec || !out) return fail(HCU_ERR_INVALID, "null argument");
  if (flags & ~HCU_PLAN_FORWARD_ONLY) return fail(HCU_ERR_INVALID, "unknown plan flags");
  return create_plan<UnetPlan>(B, X, Y, Z, out, [&](UnetPlan &p) {
    p.flags = flags;
    p.spec = *spec;
    bconv_tuning((flags & HCU_PLAN_FORWARD_ONLY) == 0);
    const int e = build_plan(p);
    bconv_tuning(true);
    return e;
  });
}

void hcu_unet_plan_destroy(hcu_unet_plan *plan) { delete plan; }

int hcu_unet_plan_query(const hcu_unet_plan *p, int64_t *out_shape, int64_t *n_params, int *n_bn,
                        size_t *saved_bytes, size_t *scratch_bytes) {
  if (!p) return fail(HCU_ERR_INVALID, "null plan");
  const UnetPlan *u = as_unet(p);   // (a chain: no out-conv channels, no parameter count)
  if (out_shape) {
    out_shape[0] = p->B;
    out_shape[1] = u ? u->Co : 0;
    out_shape[2] = p->outd.X;
    out_shape[3] = p->outd.Y;
    out_shape[4] = p->outd.Z;
  }
  if (n_params) *n_params = u ? u->n_params : 0;
  if (n_bn) *n_bn = p->n_bn;
  if (saved_bytes) *saved_bytes = p->saved_bytes;
  if (scratch_bytes) *scratch_bytes = p->scratch_bytes;
  return HCU_OK;
}

int hcu_unet_set_grad_events(hcu_unet_plan *plan, void *ev_decoder, void *ev_deep, int deep_level) {
  if (!as_unet(plan)) return fail(HCU_ERR_INVALID, "hcu_unet_set_grad_events: U-Net plan required");
  UnetPlan *p = static_cast<UnetPlan *>(plan);
  if (ev_deep && (deep_level < 1 || deep_level >= p->L))
    return fail(HCU_ERR_INVALID, "hcu_unet_set_grad_events: deep_level must be in [1, levels)");
  std::lock_guard<std::mutex> lk(p->branch.mu);   // enqueue_backward reads them under the same lock
  p->grad_ev[0] = (hipEvent_t)ev_decoder;
  p->grad_ev[1] = (hipEvent_t)ev_deep;
  p->grad_deep = ev_deep ? deep_level : -1;
  return HCU_OK;
}

// 1 when hcu_unet_backward records the events set by hcu_unet_set_grad_events
// (a direct-launch backward), 0 when it does not (a backward replayed from a
// captured graph: the caller must then reduce after the whole backward).
int hcu_unet_grad_events_live(const hcu_unet_plan *plan) {
  const UnetPlan *p = as_unet(plan);
  if (!p) return 0;
  return (graphs_for(*p, true) && !timing_on()) ? 0 : 1;
}

int hcu_event_create(void **ev) {
  if (!ev) return fail(HCU_ERR_INVALID, "null argument");
  hipEvent_t e = nullptr;
  HCU_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  *ev = e;
  return HCU_OK;
}

int hcu_event_destroy(void *ev) {
  if (ev) HCU_HIP(hipEventDestroy((hipEvent_t)ev));
  return HCU_OK;
}

int hcu_stream_wait_event(hcu_stream_t stream, void *ev) {
  if (!ev) return fail(HCU_ERR_INVALID, "null event");
  HCU_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0));
  return HCU_OK;
}

int hcu_unet_plan_bn_layers(const hcu_unet_plan *plan, hcu_bn_layer_info *out, int max) {
  if (plan && plan->is_chain) return -fail(HCU_ERR_INVALID, "hcu_unet_plan_bn_layers: U-Net plan required");
  if (!plan) return -fail(HCU_ERR_INVALID, "null plan");
  std::vector<const ConvLayer *> ls(plan->n_bn, nullptr);
  for (const ConvLayer *L : plan->convs) ls[L->bn.index] = L;
  for (int i = 0; i < plan->n_bn && i < max && out; ++i) {
    const ConvLayer &L = *ls[i];
    hcu_bn_layer_info r{};
    r.y_offset = (int64_t)L.y_off;
    r.coef_offset = (int64_t)L.bn.coef_off;
    r.B = L.out.B;
    r.X = L.out.X;
    r.Y = L.out.Y;
    r.Z = L.out.Z;
    r.C = L.out.C;
    r.Cs = L.out.Cs;
    r.elem_bytes = L.out.es;
    out[i] = r;
  }
  return plan->n_bn;
}

int hcu_unet_forward(const hcu_unet_plan *plan, const hcu_unet_tensors *t, int training,
                     hcu_stream_t stream) {
  HostProfScope prof(0);
  if (plan && plan->is_chain) return fail(HCU_ERR_INVALID, "hcu_unet_forward: U-Net plan required");
  if (!plan) return fail(HCU_ERR_INVALID, "null argument");
  const UnetPlan &p = *as_unet(plan);
  if (int e = check_forward_tensors(p, t)) return e;
  if (training)
    if (int e = check_bn_counts(p)) return e;
  // The input layout change runs ahead of the captured sequence, so a fresh
  // input tensor every step (a data loader) does not key a new graph.
  // Large parameter sets lay out their deeper weight images on the branch
  // stream while level 0 runs (Ctx in enqueue_forward).  Interleaved A/B, 3
  // runs: config 3 (11.6 M parameters) 6.418-6.434 vs 6.448-6.453 ms/step;
  // config 2 (0.7 M, ~23 us of re-layout) 2.103-2.129 vs 2.058-2.071: there
  // the branch's kernels slow level 0 more than the overlap returns.
  // (HCU_SPLIT_FWD_PARAMS: the parameter count from which the split applies;
  // tests lower it to run the split on a small network)
  static const int64_t split_min = getenv("HCU_SPLIT_FWD_PARAMS") ? atoll(getenv("HCU_SPLIT_FWD_PARAMS"))
                                                                  : (int64_t)4 << 20;
  const bool split = p.n_params >= split_min && training && side_enabled() && !timing_on() &&
                     p.prep_fwd.size() > 2;
  std::unique_lock<std::mutex> lk(p.branch.mu, std::defer_lock);
  if (int e = take_branch(p, split, lk)) return e;
  if (graphs_for(p, false) && !timing_on()) {
    if (int e = enqueue_forward(p, t, training, (hipStream_t)stream, 1, split)) return e;
    std::vector<uintptr_t> key = {0, (uintptr_t)t->out, (uintptr_t)t->params, (uintptr_t)t->saved,
                                  (uintptr_t)t->scratch, (uintptr_t)training, (uintptr_t)split};
    append_bn_key(key, p, t);
    return run_graphed(p, key, (hipStream_t)stream,
                       [&](hipStream_t s) { return enqueue_forward(p, t, training, s, 2, split); });
  }
  return enqueue_forward(p, t, training, (hipStream_t)stream, 0, split);
}

int hcu_unet_backward(const hcu_unet_plan *plan, const hcu_unet_tensors *t, const float *dout,
                      float *dx, int training, int accumulate, hcu_stream_t stream) {
  if (plan && plan->is_chain) return fail(HCU_ERR_INVALID, "hcu_unet_backward: U-Net plan required");
  if (!plan || !t || !dout || !t->grads || !t->params || !t->saved || !t->scratch)
    return fail(HCU_ERR_INVALID, "null argument");
  const UnetPlan &p = *as_unet(plan);
  if (p.flags & HCU_PLAN_FORWARD_ONLY)
    return fail(HCU_ERR_INVALID, "backward through a forward-only plan (its activations are not kept)");
  std::vector<uintptr_t> key = {1, (uintptr_t)t->params, (uintptr_t)t->grads,
                                (uintptr_t)t->saved, (uintptr_t)t->scratch, (uintptr_t)dout,
                                (uintptr_t)dx, (uintptr_t)training, (uintptr_t)accumulate};
  // Per-launch timing attributes kernel time to layers: keep it serial.
  const bool split = side_enabled() && !timing_on();
  std::unique_lock<std::mutex> lk(p.branch.mu, std::defer_lock);
  if (int e = take_branch(p, split, lk)) return e;
  key.push_back((uintptr_t)split);
  const bool live = graphs_for(p, true) && !timing_on() ? false : true;
  HostProfScope prof(1);
  return run_graphed(p, key, (hipStream_t)stream, [&](hipStream_t s) {
    return enqueue_backward(p, t, dout, dx, training, accumulate, s, split, live);
  });
}

}  // extern "C"
