// Per-op entry points (channels-last), sharing the executor's layer setup:
// one Conv3d / ConvTranspose3d forward, input gradient or weight gradient on
// the caller's scratch, and the max-pool forward.
#include "exec.h"

using namespace hcu;

namespace {

struct OpPlan {
  ConvLayer conv;
  ConvTLayer ct;
  ScratchNeed need;
  size_t wprep_off = 0, part_off = 0, kpart_off = 0, scratch_bytes = 0;
};

int make_op(const hcu_conv_desc *d, OpPlan &op) {
  if (!d) return fail(HCU_ERR_INVALID, "null descriptor");
  if (d->dtype != HCU_F32 && d->dtype != HCU_BF16) return fail(HCU_ERR_INVALID, "bad dtype");
  const Dims in = mkdims(d->B, d->X, d->Y, d->Z, d->Cin, d->dtype == HCU_BF16 ? 2 : 4);
  if (!d->transposed) {
    for (int i = 0; i < 3; ++i)
      if (d->stride[i] != 1) return fail(HCU_ERR_UNSUPPORTED, "Conv3d: only stride 1 (valid) is supported");
    if (int e = setup_conv(op.conv, in, d->Cout, d->groups, d->Cin, d->Cin, d->k, d->dil, "conv3d"))
      return e;
    // (the per-op weight gradient always runs the planned kernel, never the pointwise form)
    op.conv.wg.pw_blocks = 0;
    op.conv.wg.pw_slab = 0;
    op.need.conv(op.conv.fwd);
    op.need.conv(op.conv.dgrad);
    op.need.job(op.conv.wg);
  } else {
    if (d->groups != 1) return fail(HCU_ERR_UNSUPPORTED, "ConvTranspose3d: groups must be 1");
    for (int i = 0; i < 3; ++i)
      if (d->dil[i] != 1) return fail(HCU_ERR_UNSUPPORTED, "ConvTranspose3d: dilation must be 1");
    if (int e = setup_convt(op.ct, in, d->Cout, d->k, d->stride, nullptr, false, op.need)) return e;
  }
  Region r;
  op.wprep_off = r.take_floats(op.need.wprep);
  op.part_off = r.take_floats(op.need.part);
  op.kpart_off = r.take_floats(std::max<size_t>(op.need.kpart, 1));
  op.scratch_bytes = r.off;
  return 0;
}

// One layer's weight re-layout (a plan's job record, prep_job) from the weight
// `w` into the image `dst`.
int prep_one(const PrepJob &j, const float *w, float *dst, hipStream_t s) {
  return launch_prep_all(w, dst, &j, 1, s);
}

int check_scratch(const OpPlan &op, void *scratch, size_t bytes) {
  if (bytes < op.scratch_bytes || (!scratch && op.scratch_bytes))
    return fail(HCU_ERR_WORKSPACE, "scratch workspace too small: need " + std::to_string(op.scratch_bytes));
  return 0;
}

}  // namespace

extern "C" {

size_t hcu_conv_scratch_bytes(const hcu_conv_desc *d) {
  OpPlan op;
  if (make_op(d, op)) return 0;
  return op.scratch_bytes;
}

int hcu_conv_out_dims(const hcu_conv_desc *d, int *out) {
  OpPlan op;
  if (int e = make_op(d, op)) return e;
  const Dims &o = d->transposed ? op.ct.out : op.conv.out;
  out[0] = o.X;
  out[1] = o.Y;
  out[2] = o.Z;
  return HCU_OK;
}

int hcu_conv_fwd_cl(const hcu_conv_desc *d, const float *x, const float *w, const float *bias,
                    float *y, void *scratch, size_t scratch_bytes, hcu_stream_t stream) {
  OpPlan op;
  if (int e = make_op(d, op)) return e;
  if (int e = check_scratch(op, scratch, scratch_bytes)) return e;
  hipStream_t s = (hipStream_t)stream;
  float *wprep = reinterpret_cast<float *>((char *)scratch + op.wprep_off);
  float *kpart = reinterpret_cast<float *>((char *)scratch + op.kpart_off);
  if (!d->transposed) {
    if (int e = prep_one(conv_fwd_job(op.conv), w, wprep, s)) return e;
    return run_conv(op.conv.fwd, x, nullptr, nullptr, wprep, bias, y, nullptr, kpart, s);
  }
  const ConvTLayer &u = op.ct;
  if (u.fused) {
    if (int e = prep_one(convt_fused_job(u), w, wprep, s)) return e;
    return run_conv(u.fwdf, x, nullptr, nullptr, wprep, bias, y, nullptr, kpart, s);
  }
  // (every phase's image goes through the one scratch buffer, just ahead of its launch)
  for (size_t ph = 0; ph < u.phases.size(); ++ph) {
    if (int e = prep_one(convt_phase_job(u, ph), w, wprep, s)) return e;
    if (int e = run_conv(u.phases[ph], x, nullptr, nullptr, wprep, bias, y, nullptr, kpart, s)) return e;
  }
  return HCU_OK;
}

int hcu_conv_dgrad_cl(const hcu_conv_desc *d, const float *dy, const float *w, float *dx,
                      void *scratch, size_t scratch_bytes, hcu_stream_t stream) {
  OpPlan op;
  if (int e = make_op(d, op)) return e;
  if (int e = check_scratch(op, scratch, scratch_bytes)) return e;
  hipStream_t s = (hipStream_t)stream;
  float *wprep = reinterpret_cast<float *>((char *)scratch + op.wprep_off);
  float *kpart = reinterpret_cast<float *>((char *)scratch + op.kpart_off);
  if (int e = prep_one(d->transposed ? convt_dgrad_job(op.ct) : conv_dgrad_job(op.conv), w, wprep, s)) return e;
  return run_conv(d->transposed ? op.ct.dgrad : op.conv.dgrad, dy, nullptr, nullptr, wprep, nullptr, dx, nullptr,
                  kpart, s);
}

int hcu_conv_wgrad_cl(const hcu_conv_desc *d, const float *x, const float *dy, float *dw,
                      float *dbias, void *scratch, size_t scratch_bytes, hcu_stream_t stream) {
  OpPlan op;
  if (int e = make_op(d, op)) return e;
  if (int e = check_scratch(op, scratch, scratch_bytes)) return e;
  hipStream_t s = (hipStream_t)stream;
  float *part = reinterpret_cast<float *>((char *)scratch + op.part_off);
  // the planned job on the caller's scratch, finalized at once
  const WGradJob &j = d->transposed ? op.ct.wg : op.conv.wg;
  WGradArgs w = j.w;
  w.A = x;
  w.G = dy;
  w.partial = part;
  if (int e = launch_wgrad(w, s)) return e;
  WGradFinalize f = j.f;
  f.partial = part;
  f.dw = dw;
  f.db = d->transposed ? nullptr : dbias;
  if (int e = launch_wgrad_finalize(f, s)) return e;
  if (d->transposed && dbias) {
    const ConvTLayer &u = op.ct;
    const int R = chansum_rows(u.out.vox(), u.out.Cs);
    if (int e = launch_chansum(dy, u.out.vox(), u.out.Cs, part, R, s, u.out.es == 2)) return e;
    if (int e = launch_reduce_partials(part, R, u.out.Cs, u.Cout, dbias, 0, s)) return e;
  }
  return HCU_OK;
}

int hcu_maxpool_fwd_cl(int B, int C, int X, int Y, int Z, const int *k, const float *x, float *y,
                       hcu_stream_t stream) {
  if (!k || k[0] < 1 || k[1] < 1 || k[2] < 1) return fail(HCU_ERR_INVALID, "bad pool kernel");
  if (X / k[0] < 1 || Y / k[1] < 1 || Z / k[2] < 1)
    return fail(HCU_ERR_SHAPE, "max_pool3d: Output size is too small");
  return launch_maxpool_fwd(x, nullptr, nullptr, y, B, X, Y, Z, round_up(C, 4), k[0], k[1], k[2],
                            (hipStream_t)stream);
}

}  // extern "C"
