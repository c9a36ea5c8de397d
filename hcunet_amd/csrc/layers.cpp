// Layer planning for the executor's plans and the per-op entry points: the
// shapes, kernel arguments and weight-gradient jobs of one Conv3d /
// ConvTranspose3d layer, its weight re-layout jobs, what it asks of scratch,
// the scratch layout both plan kinds share, and the plan log.  Runs without a
// device.
#include "plan.h"

namespace hcu {

Dims mkdims(int B, int X, int Y, int Z, int C, int es) {
  Dims d;
  d.B = B;
  d.X = X;
  d.Y = Y;
  d.Z = Z;
  d.C = C;
  d.es = es;
  d.Cs = round_up(C, es == 2 ? 8 : 4);
  return d;
}

namespace {

// The job of a planned kernel `w` with the finalize shape `f`.
WGradJob wgrad_job(const WGradArgs &w, WGradFinalize f) {
  WGradJob j;
  j.w = w;
  f.KB = w.KB;
  f.Mtot = w.Mtot;
  f.Ntot = w.Ntot;
  j.f = f;
  j.on = true;
  j.slab = wgrad_partial_floats(w);
  return j;
}

// bf16 Conv3d weight gradients store slab rows of real input channels and
// columns of real output channels only (WGradArgs::ACr / GCr): RDCNet's
// 10-channel tensors sit in 16-slot strides.  Inputs made of channel parts
// keep every packed slot (finalize maps torch channels to packed slots).
// (The fp32 planner clears both.)
void compact_slab(WGradArgs &w, const ConvLayer &L) {
  if (L.part_c == 0 && L.groups == 1) w.ACr = L.E;
  w.GCr = L.Cout;
}

// An input made of channel parts (Dims::part_c): every packed channel e of
// the input stride is a GEMM row (the padding ones get zero weights), and
// e maps to torch channel (e / part_cs) * part_c + e % part_cs.
void set_parts(ConvLayer &L, const Dims &in) {
  L.part_c = in.part_c;
  L.part_cs = in.part_c ? round_up(in.part_c, in.es == 2 ? 8 : 4) : 0;
  if (in.part_c) L.E = in.Cs;
}

// The weight-gradient job of a Conv3d layer whose kernel is planned in `w`.
WGradJob conv_wgrad_job(const ConvLayer &L, const WGradArgs &w) {
  return wgrad_job(w, wgf_conv(L.T, L.Cout, L.Cin_g, L.groups, L.fold_mod, L.part_c, L.part_cs,
                               wgrad_slab_acs(w)));
}

}  // namespace

GConvArgs gconv_conv_fwd(const Dims &in, const Dims &out, const int K[3], const int D[3], int Cout) {
  GConvArgs a{};
  a.B = in.B;
  a.IX = in.X; a.IY = in.Y; a.IZ = in.Z; a.ICs = in.Cs;
  a.OX = out.X; a.OY = out.Y; a.OZ = out.Z;
  a.SX = out.X; a.SY = out.Y; a.SZ = out.Z; a.OCs = out.Cs; a.Cout = Cout;
  a.osx = a.osy = a.osz = 1;
  a.KX = K[0]; a.KY = K[1]; a.KZ = K[2];
  a.sx = a.sy = a.sz = 1;
  a.dx = D[0]; a.dy = D[1]; a.dz = D[2];
  return a;
}

GConvArgs gconv_conv_dgrad(const Dims &in, const Dims &out, const int K[3], const int D[3], int E) {
  GConvArgs a{};
  a.B = in.B;
  a.IX = out.X; a.IY = out.Y; a.IZ = out.Z; a.ICs = out.Cs;
  a.OX = in.X; a.OY = in.Y; a.OZ = in.Z;
  a.SX = in.X; a.SY = in.Y; a.SZ = in.Z; a.OCs = in.Cs; a.Cout = E;
  a.osx = a.osy = a.osz = 1;
  a.KX = K[0]; a.KY = K[1]; a.KZ = K[2];
  a.sx = a.sy = a.sz = 1;
  a.dx = D[0]; a.dy = D[1]; a.dz = D[2];
  a.px = D[0] * (K[0] - 1); a.py = D[1] * (K[1] - 1); a.pz = D[2] * (K[2] - 1);
  return a;
}

WGradArgs wgrad_conv(const Dims &in, const Dims &out, const int K[3], const int D[3]) {
  WGradArgs w{};
  w.B = in.B;
  w.AX = in.X; w.AY = in.Y; w.AZ = in.Z; w.ACs = in.Cs;
  w.GX = out.X; w.GY = out.Y; w.GZ = out.Z; w.GCs = out.Cs;
  w.PX = out.X; w.PY = out.Y; w.PZ = out.Z;
  w.KX = K[0]; w.KY = K[1]; w.KZ = K[2];
  w.asx = w.asy = w.asz = 1;
  w.adx = D[0]; w.ady = D[1]; w.adz = D[2];
  w.gsx = w.gsy = w.gsz = 1;
  w.taps_rows = 1;
  w.bias_row = 1;
  return w;
}

// A bf16 1x1x1 Conv3d (stride 1, no padding, one group, no cat fold) takes the
// streaming pointwise kernels for its forward and input gradient when its
// input carries no BatchNorm+ReLU (checked at launch) and it has none itself
// (the chain's non-BatchNorm branch).  HCU_PW=0: bconv everywhere (A/B).
void set_pw(ConvLayer &L, const Dims &in, int cin_total) {
  static const bool off = getenv("HCU_PW") && getenv("HCU_PW")[0] == '0';
  L.pw = false;
  if (off || in.es != 2 || L.groups != 1 || L.fold_mod < cin_total) return;
  for (int i = 0; i < 3; ++i)
    if (L.K[i] != 1 || L.S[i] != 1 || L.P[i] != 0) return;
  L.pw = pw_supported(in.Cs, L.out.Cs, L.Cout, false) &&
         (!L.has_dgrad || pw_supported(in.Cs, L.out.Cs, L.Cout, true));
  // (the slab layout is bwgrad's taps_rows one, planned in L.wg)
  WGradJob &j = L.wg;
  if (j.w.taps_rows && j.w.ACs == in.Cs && j.w.GCs == L.out.Cs &&
      pw_wgrad_supported(in.Cs, L.out.Cs)) {
    j.pw_blocks = pw_wgrad_blocks(wgrad_gvox(j.w));
    j.pw_slab = (size_t)j.pw_blocks * j.w.Mtot * j.w.Ntot;
  }
}

// Conv3d, optionally with stride / zero padding (nn.Conv3d(..., stride, padding),
// the r_unet.py layers; null: stride 1, no padding -- the U-Net is valid):
// out = floor((in + 2P - D(K-1) - 1) / S) + 1.  Forward: o*S + t*D - P; input
// gradient (stride 1): the full correlation with padding D(K-1) - P; weight
// gradient: A offset o*S + t*D - P.
// sublattice (layer chains, the only executor of that form): a dilated kernel
// whose halo does not fit the kernels' LDS may be planned on the dilation
// sub-lattices (s2b), so every planner runs before an error is returned.
// Without it the first planner's error is returned as it stands.
int setup_conv(ConvLayer &L, const Dims &in, int Cout, int groups, int fold_mod, int cin_total,
               const int K[3], const int D[3], const char *name, bool sublattice, const int *S,
               const int *P) {
  for (int i = 0; i < 3; ++i) {
    L.K[i] = K[i];
    L.D[i] = D[i];
    L.S[i] = S ? S[i] : 1;
    L.P[i] = P ? P[i] : 0;
    if (K[i] < 1 || D[i] < 1) return fail(HCU_ERR_INVALID, std::string(name) + ": bad kernel/dilation");
    if (L.S[i] < 1 || L.P[i] < 0) return fail(HCU_ERR_INVALID, std::string(name) + ": bad stride/padding");
  }
  if (groups < 1 || cin_total % groups || Cout % groups)
    return fail(HCU_ERR_INVALID, std::string(name) + ": channels must be divisible by groups");
  L.Cout = Cout;
  L.groups = groups;
  L.Cin_g = cin_total / groups;
  L.fold_mod = fold_mod;
  L.E = std::min(fold_mod, cin_total);
  set_parts(L, in);
  L.T = L.K[0] * L.K[1] * L.K[2];
  L.in = in;
  int o[3];
  const int iv[3] = {in.X, in.Y, in.Z};
  for (int i = 0; i < 3; ++i) {
    const int span = iv[i] + 2 * L.P[i] - L.D[i] * (L.K[i] - 1);
    if (span < 1)
      return fail(HCU_ERR_SHAPE, std::string(name) + ": Calculated padded input size per channel: (" +
                                     std::to_string(in.X + 2 * L.P[0]) + " x " + std::to_string(in.Y + 2 * L.P[1]) +
                                     " x " + std::to_string(in.Z + 2 * L.P[2]) +
                                     "). Kernel size can't be greater than actual input size");
    o[i] = (span - 1) / L.S[i] + 1;
  }
  L.out = mkdims(in.B, o[0], o[1], o[2], Cout, in.es);
  L.has_dgrad = L.S[0] == 1 && L.S[1] == 1 && L.S[2] == 1;
  L.s2b = false;
  // direct form
  {
    GConvArgs f = gconv_conv_fwd(in, L.out, L.K, L.D, Cout);
    f.sx = L.S[0]; f.sy = L.S[1]; f.sz = L.S[2];
    f.px = L.P[0]; f.py = L.P[1]; f.pz = L.P[2];
    const int ef = plan_conv(f, in.es, kTargetBlocks);
    if (ef && !sublattice) return ef;
    int ed = 0;
    GConvArgs dg{};
    if (L.has_dgrad) {
      dg = gconv_conv_dgrad(in, L.out, L.K, L.D, L.E);
      dg.px = L.D[0] * (L.K[0] - 1) - L.P[0];
      dg.py = L.D[1] * (L.K[1] - 1) - L.P[1];
      dg.pz = L.D[2] * (L.K[2] - 1) - L.P[2];
      if (dg.px < 0 || dg.py < 0 || dg.pz < 0)
        return fail(HCU_ERR_UNSUPPORTED, std::string(name) + ": padding larger than dilation*(kernel-1)");
      ed = plan_conv(dg, in.es, kTargetBlocks);
      if (ed && !sublattice) return ed;
    }
    WGradArgs w = wgrad_conv(in, L.out, L.K, L.D);
    w.asx = L.S[0]; w.asy = L.S[1]; w.asz = L.S[2];
    w.apx = L.P[0]; w.apy = L.P[1]; w.apz = L.P[2];
    compact_slab(w, L);
    const int ew = plan_wgrad_any(w, in.es, kTargetBlocks);
    const bool dil = L.D[0] > 1 || L.D[1] > 1 || L.D[2] > 1;
    if (!ef && !ed && !ew) {
      L.fwd = f;
      L.dgrad = dg;
      L.wg = conv_wgrad_job(L, w);
    } else if (!sublattice || !dil || !L.has_dgrad) {
      return ef ? ef : ed ? ed : ew;
    } else {
      L.s2b = true;
    }
  }
  if (L.s2b) {
    // dilation sub-lattices: output o = r + D*o' reads input r + D*(o' + t - P/D)
    int sub_i[3], sub_o[3], Pd[3];
    const int one[3] = {1, 1, 1};
    int nlat = 1;
    for (int i = 0; i < 3; ++i) {
      if (L.P[i] % L.D[i])
        return fail(HCU_ERR_UNSUPPORTED, std::string(name) + ": dilated convolution too large for one tile "
                                                             "and padding not a multiple of the dilation");
      L.L3[i] = L.D[i];
      nlat *= L.D[i];
      Pd[i] = L.P[i] / L.D[i];
      sub_i[i] = cdiv(iv[i], L.D[i]);
      sub_o[i] = sub_i[i] + 2 * Pd[i] - (L.K[i] - 1);
      if (sub_o[i] < cdiv(o[i], L.D[i]))
        return fail(HCU_ERR_UNSUPPORTED, std::string(name) + ": sub-lattice output too small");
    }
    L.sub_in = mkdims(in.B * nlat, sub_i[0], sub_i[1], sub_i[2], in.C, in.es);
    L.sub_in.Cs = in.Cs;
    L.sub_in.part_c = in.part_c;
    L.sub_out = mkdims(in.B * nlat, sub_o[0], sub_o[1], sub_o[2], Cout, in.es);
    L.fwd = gconv_conv_fwd(L.sub_in, L.sub_out, L.K, one, Cout);
    L.fwd.px = Pd[0]; L.fwd.py = Pd[1]; L.fwd.pz = Pd[2];
    if (int e = plan_conv(L.fwd, in.es, kTargetBlocks)) return e;
    L.dgrad = gconv_conv_dgrad(L.sub_in, L.sub_out, L.K, one, L.E);
    L.dgrad.px = (L.K[0] - 1) - Pd[0];
    L.dgrad.py = (L.K[1] - 1) - Pd[1];
    L.dgrad.pz = (L.K[2] - 1) - Pd[2];
    if (int e = plan_conv(L.dgrad, in.es, kTargetBlocks)) return e;
    WGradArgs w = wgrad_conv(L.sub_in, L.sub_out, L.K, one);
    w.apx = Pd[0]; w.apy = Pd[1]; w.apz = Pd[2];
    compact_slab(w, L);
    if (int e = plan_wgrad_any(w, in.es, kTargetBlocks)) return e;
    L.wg = conv_wgrad_job(L, w);
  }
  L.bn.C = Cout;
  L.bn.Cs = L.out.Cs;
  L.bn.count = (double)L.out.vox();
  set_pw(L, in, cin_total);
  return 0;
}

// pad (layer chains; null: none): ConvTranspose3d padding, the crop of the full
// output.  The forward writes the full output (into scratch) and crops it;
// the backward reads the cropped gradient at offset pad (zero outside it).
// swap: also plan the swapped weight-gradient form (ConvTLayer::wgs).
int setup_convt(ConvTLayer &u, const Dims &cur, int o, const int K[3], const int S[3],
                const int *pad, bool swap, ScratchNeed &need) {
  const int f = cur.C;
  u.Cin = f;
  u.Cout = o;
  u.T = K[0] * K[1] * K[2];
  for (int d = 0; d < 3; ++d) {
    u.K[d] = K[d];
    u.S[d] = S[d];
    if (K[d] < 1 || S[d] < 1) return fail(HCU_ERR_INVALID, "ConvTranspose3d: bad kernel/stride");
  }
  u.in = cur;
  const int ux = (cur.X - 1) * u.S[0] + u.K[0], uy = (cur.Y - 1) * u.S[1] + u.K[1],
            uz = (cur.Z - 1) * u.S[2] + u.K[2];
  u.full = mkdims(cur.B, ux, uy, uz, o, cur.es);
  const int P[3] = {pad ? pad[0] : 0, pad ? pad[1] : 0, pad ? pad[2] : 0};
  for (int d = 0; d < 3; ++d)
    if (P[d] < 0) return fail(HCU_ERR_INVALID, "ConvTranspose3d: negative padding");
  const int cx = ux - 2 * P[0], cy = uy - 2 * P[1], cz = uz - 2 * P[2];   // the cropped output
  if (cx < 1 || cy < 1 || cz < 1) return fail(HCU_ERR_SHAPE, "ConvTranspose3d: output size is too small");
  u.out = mkdims(cur.B, cx, cy, cz, o, cur.es);
  const bool bf = cur.es == 2;
  u.phases.clear();
  u.pJ.clear();
  const int nph = u.S[0] * u.S[1] * u.S[2];
  u.fused = u.K[0] % u.S[0] == 0 && u.K[1] % u.S[1] == 0 && u.K[2] % u.S[2] == 0;
  if (bf && !u.fused)
    return fail(HCU_ERR_UNSUPPORTED,
                "ConvTranspose3d with kernel % stride != 0 is not supported on the bf16 path");
  if (u.fused) {
    const int Jx = u.K[0] / u.S[0], Jy = u.K[1] / u.S[1], Jz = u.K[2] / u.S[2];
    GConvArgs a{};
    a.B = cur.B;
    a.IX = cur.X; a.IY = cur.Y; a.IZ = cur.Z; a.ICs = cur.Cs;
    a.OX = cur.X + Jx - 1; a.OY = cur.Y + Jy - 1; a.OZ = cur.Z + Jz - 1;
    a.SX = ux; a.SY = uy; a.SZ = uz; a.OCs = u.out.Cs; a.Cout = o;
    a.osx = u.S[0]; a.osy = u.S[1]; a.osz = u.S[2];
    a.KX = Jx; a.KY = Jy; a.KZ = Jz;
    a.sx = a.sy = a.sz = 1;
    a.dx = a.dy = a.dz = 1;
    a.px = Jx - 1; a.py = Jy - 1; a.pz = Jz - 1;
    a.nph = nph; a.phx = u.S[0]; a.phy = u.S[1]; a.phz = u.S[2];
    // columns per phase padded to the 8 (bf16) / 4 (fp32) a packed vector and
    // a lane's store span (zero weights and bias; RDCNet's 5 output channels)
    const int cv = bf ? 8 : 4;
    if (o % cv) a.cph = round_up(o, cv);
    // (fp32: a shape no phase-folding family takes runs the per-phase form below)
    const int e = plan_conv(a, cur.es, kTargetBlocks);
    if (bf && e) return e;
    if (e || !conv_family(a).folds_phases) u.fused = false;
    if (u.fused) {
      u.fwdf = a;
      need.conv(a);
    }
  }
  for (int qx = 0; qx < (bf ? 0 : u.S[0]); ++qx)
    for (int qy = 0; qy < u.S[1]; ++qy)
      for (int qz = 0; qz < u.S[2]; ++qz) {
        const int Jx = cdiv(u.K[0] - qx, u.S[0]), Jy = cdiv(u.K[1] - qy, u.S[1]),
                  Jz = cdiv(u.K[2] - qz, u.S[2]);
        if (Jx < 1 || Jy < 1 || Jz < 1)
          return fail(HCU_ERR_UNSUPPORTED, "ConvTranspose3d with kernel < stride is not supported");
        GConvArgs a{};
        a.B = cur.B;
        a.IX = cur.X; a.IY = cur.Y; a.IZ = cur.Z; a.ICs = cur.Cs;
        a.OX = cdiv(ux - qx, u.S[0]); a.OY = cdiv(uy - qy, u.S[1]); a.OZ = cdiv(uz - qz, u.S[2]);
        a.SX = ux; a.SY = uy; a.SZ = uz; a.OCs = u.out.Cs; a.Cout = o;
        a.osx = u.S[0]; a.osy = u.S[1]; a.osz = u.S[2];
        a.ofx = qx; a.ofy = qy; a.ofz = qz;
        a.KX = Jx; a.KY = Jy; a.KZ = Jz;
        a.sx = a.sy = a.sz = 1;
        a.dx = a.dy = a.dz = 1;
        a.px = Jx - 1; a.py = Jy - 1; a.pz = Jz - 1;
        if (int e = conv_family(KCONV_GCONV, 4).plan(a, std::max(64, kTargetBlocks / nph))) return e;
        u.phases.push_back(a);
        const int pj[6] = {qx, qy, qz, Jx, Jy, Jz};
        u.pJ.insert(u.pJ.end(), pj, pj + 6);
        need.conv(a);
      }
  {  // dgrad: strided correlation of dU with W[ci][co][t]
    GConvArgs a{};
    a.B = cur.B;
    a.IX = cx; a.IY = cy; a.IZ = cz; a.ICs = u.out.Cs;
    a.px = P[0]; a.py = P[1]; a.pz = P[2];
    a.OX = cur.X; a.OY = cur.Y; a.OZ = cur.Z;
    a.SX = cur.X; a.SY = cur.Y; a.SZ = cur.Z; a.OCs = cur.Cs; a.Cout = f;
    a.osx = a.osy = a.osz = 1;
    a.KX = u.K[0]; a.KY = u.K[1]; a.KZ = u.K[2];
    a.sx = u.S[0]; a.sy = u.S[1]; a.sz = u.S[2];
    a.dx = a.dy = a.dz = 1;
    if (int e = plan_conv(a, cur.es, kTargetBlocks)) return e;
    u.dgrad = a;
    need.conv(a, 2);
  }
  // the finalize shape of this layer's weight gradient in mode 1 (per tap) / 3 (phases)
  auto wgf = [&](int mode, const WGradArgs &w) {
    WGradFinalize fz{};
    fz.mode = mode;
    fz.T = u.T;
    fz.Cin = u.Cin;
    fz.CoutT = u.Cout;
    fz.GCs = w.GCs;
    if (mode == 3) {
      fz.ACs = w.ACs;
      for (int d = 0; d < 3; ++d) {
        fz.J[d] = u.K[d] / u.S[d];
        fz.SS[d] = u.S[d];
      }
    }
    return fz;
  };
  {  // wgrad: rows = ci, cols = (t, co)
    WGradArgs w{};
    w.B = cur.B;
    w.AX = cur.X; w.AY = cur.Y; w.AZ = cur.Z; w.ACs = cur.Cs;
    w.GX = cx; w.GY = cy; w.GZ = cz; w.GCs = u.out.Cs;
    w.gpx = P[0]; w.gpy = P[1]; w.gpz = P[2];
    w.PX = cur.X; w.PY = cur.Y; w.PZ = cur.Z;
    w.KX = u.K[0]; w.KY = u.K[1]; w.KZ = u.K[2];
    w.asx = w.asy = w.asz = 1;
    w.gsx = u.S[0]; w.gsy = u.S[1]; w.gsz = u.S[2];
    w.gdx = w.gdy = w.gdz = 1;
    w.taps_rows = 0;
    w.bias_row = 0;
    if (int e = plan_wgrad_any(w, cur.es, kTargetBlocks)) return e;
    u.wg = wgrad_job(w, wgf(1, w));
    need.job(u.wg);
    // the bias gradient's channel-sum rows (layer chains: an arena slab)
    const size_t cs = (size_t)chansum_rows(u.out.vox(), u.out.Cs) * u.out.Cs;
    need.rows(cs);
    need.arena(cs);
  }
  u.wgp = WGradJob{};
  // The weight gradient of the phase-folded forward (stride phases as extra
  // output columns) on wgrad3; the other layers run the per-tap wgrad_kernel.
  // (The U-Net's bias gradient: the column sums of dU, written by the
  // folded conv1's input-gradient kernel; layer chains: chansum.)
  if (!bf && u.fused && o % 4 == 0) {
    // dW'[(j, ci)][(q, co)] = sum_o A[o + j - (J-1)][ci] * dU[o*S + q][co] over the
    // phase grid o (the forward's fused GEMM, hcat/unet.py:294-298)
    const int J[3] = {u.K[0] / u.S[0], u.K[1] / u.S[1], u.K[2] / u.S[2]};
    WGradArgs w{};
    w.B = cur.B;
    w.AX = cur.X; w.AY = cur.Y; w.AZ = cur.Z; w.ACs = cur.Cs;
    w.GX = ux; w.GY = uy; w.GZ = uz; w.GCs = u.out.Cs;
    w.PX = cur.X + J[0] - 1; w.PY = cur.Y + J[1] - 1; w.PZ = cur.Z + J[2] - 1;
    w.KX = J[0]; w.KY = J[1]; w.KZ = J[2];
    w.asx = w.asy = w.asz = 1;
    w.adx = w.ady = w.adz = 1;
    w.apx = J[0] - 1; w.apy = J[1] - 1; w.apz = J[2] - 1;
    w.gsx = u.S[0]; w.gsy = u.S[1]; w.gsz = u.S[2];
    w.gdx = w.gdy = w.gdz = 1;
    w.taps_rows = 1;
    w.bias_row = 0;
    w.nph = nph; w.phx = u.S[0]; w.phy = u.S[1]; w.phz = u.S[2]; w.GCout = o;
    if (plan_wgrad_any(w, cur.es, kTargetBlocks) == 0 && w.kern == KWG_WGRAD3) {
      u.wgp = wgrad_job(w, wgf(3, w));
      need.job(u.wgp);
    } else {
      set_error("");
    }
  }
  u.wgs = WGradJob{};
  if (swap) {
    // dW[ci][co][k] = sum_o x[o][ci] dU[o*S + k - pad][co]
    WGradArgs v{};
    v.B = cur.B;
    v.AX = u.out.X; v.AY = u.out.Y; v.AZ = u.out.Z; v.ACs = u.out.Cs;   // dU (cropped)
    v.GX = u.in.X; v.GY = u.in.Y; v.GZ = u.in.Z; v.GCs = u.in.Cs;        // x
    v.PX = u.in.X; v.PY = u.in.Y; v.PZ = u.in.Z;
    v.KX = u.K[0]; v.KY = u.K[1]; v.KZ = u.K[2];
    v.asx = u.S[0]; v.asy = u.S[1]; v.asz = u.S[2];
    v.adx = v.ady = v.adz = 1;
    v.apx = P[0]; v.apy = P[1]; v.apz = P[2];
    v.gsx = v.gsy = v.gsz = 1;
    v.gdx = v.gdy = v.gdz = 1;
    v.taps_rows = 1;
    v.bias_row = 0;
    v.ACr = u.Cout;
    v.GCr = u.Cin;
    v.flops = 2.0 * cur.B * u.in.X * u.in.Y * u.in.Z * (double)u.T * u.Cin * u.Cout;
    if (plan_wgrad_any(v, cur.es, kTargetBlocks) == 0) {   // (swap: bf16 plans only)
      u.wgs = wgrad_job(v, wgf_conv(u.T, u.Cin, u.Cout, 1, u.Cout, 0, 0, wgrad_slab_acs(v)));
      need.job(u.wgs);
    } else {
      set_error("");
    }
  }
  return 0;
}

void track_conv(PlanCore &p, const ConvLayer &L) {
  p.max_act = std::max(p.max_act, std::max(L.in.floats(), L.out.floats()));
  p.need.conv(L.fwd, 4);  // StatRow
  p.need.conv(L.dgrad, 2);
  p.need.job(L.wg);
  p.need.rows((size_t)bwd_rows(L.out.vox(), L.out.Cs) * L.out.Cs * 2);
}

namespace {

// The re-layout job (prep_all.hip) of the weight image the planned GEMM `a`
// reads, with the kind's parameters (PrepJob::p).  src / dst stay 0: the
// weight and the image themselves (the per-op entry points); add_prep places
// a plan's jobs in the parameter buffer and in `saved`.
PrepJob prep_job(int kind, const GConvArgs &a, std::initializer_list<int> prm) {
  PrepJob j{};
  j.kind = kind;
  j.bf16 = conv_family(a).wbytes == 2;
  j.n = wimage_elems(a);
  j.pk = wpack_of(a);
  std::copy(prm.begin(), prm.end(), j.p);
  return j;
}

// Prepared (GEMM-layout) weights of every layer: written once per forward by
// one batched launch, read by the forward and backward GEMMs.  Places job `j`
// of the weight at parameter offset `src`; off: its image in `saved`.
void add_prep(PlanCore &p, Region &saved, PrepJob j, int64_t src, size_t &off) {
  j.src = src;
  off = saved.take_floats(wimage_floats(j.n, j.bf16 ? 2 : 4));
  j.dst = (int64_t)(off / sizeof(float));
  p.prep_jobs.push_back(j);
}

}  // namespace

// A Conv3d layer's forward image (t, e, co) / input-gradient image (t', co, e).
PrepJob conv_fwd_job(const ConvLayer &cl) {
  return prep_job(PREP_CONV_FWD, cl.fwd,
                  {cl.Cout, cl.Cin_g, cl.groups, cl.fold_mod, cl.T, cl.fwd.ICs, cl.fwd.CoutW,
                   cl.part_c ? cl.fwd.ICs : std::min(cl.fold_mod, cl.groups * cl.Cin_g), cl.part_c, cl.part_cs});
}
PrepJob conv_dgrad_job(const ConvLayer &cl) {
  return prep_job(PREP_CONV_DGRAD, cl.dgrad,
                  {cl.Cout, cl.Cin_g, cl.groups, cl.fold_mod, cl.T, cl.dgrad.ICs, cl.dgrad.CoutW, cl.E,
                   cl.part_c, cl.part_cs});
}
// A ConvTranspose3d layer's images: the phase-folded forward, one forward
// phase (the plain [t][ci][co] layout of gconv) and the input gradient.
PrepJob convt_fused_job(const ConvTLayer &u) {
  return prep_job(PREP_CONVT_FUSED, u.fwdf,
                  {u.Cin, u.Cout, u.K[0], u.K[1], u.K[2], u.S[0], u.S[1], u.S[2], u.fwdf.ICs, u.fwdf.CoutW,
                   u.fwdf.cph});
}
PrepJob convt_phase_job(const ConvTLayer &u, size_t ph) {
  const int *pj = &u.pJ[ph * 6];
  const GConvArgs &a = u.phases[ph];
  return prep_job(PREP_CONVT_PHASE, a,
                  {u.Cin, u.Cout, u.K[0], u.K[1], u.K[2], u.S[0], u.S[1], u.S[2], pj[0], pj[1], pj[2], pj[3],
                   pj[4], pj[5], a.ICs, a.CoutW});
}
PrepJob convt_dgrad_job(const ConvTLayer &u) {
  return prep_job(PREP_CONVT_DGRAD, u.dgrad, {u.Cin, u.Cout, u.T, u.dgrad.ICs, u.dgrad.CoutW});
}

void conv_prep(PlanCore &p, Region &saved, ConvLayer &cl) {
  add_prep(p, saved, conv_fwd_job(cl), cl.w_off, cl.wf_off);
  if (cl.has_dgrad) add_prep(p, saved, conv_dgrad_job(cl), cl.w_off, cl.wd_off);
}

void convt_prep(PlanCore &p, Region &saved, ConvTLayer &u) {
  if (u.fused) {
    add_prep(p, saved, convt_fused_job(u), u.w_off, u.wf_off);
  } else {
    u.wph_off.assign(u.phases.size(), 0);
    for (size_t ph = 0; ph < u.phases.size(); ++ph)
      add_prep(p, saved, convt_phase_job(u, ph), u.w_off, u.wph_off[ph]);
  }
  add_prep(p, saved, convt_dgrad_job(u), u.w_off, u.wd_off);
}

// The forward's images / the input-gradient images only the backward reads.
void split_prep(PlanCore &p) {
  p.prep_fwd.clear();
  p.prep_bwd.clear();
  for (const PrepJob &j : p.prep_jobs)
    (j.kind == PREP_CONV_DGRAD || j.kind == PREP_CONVT_DGRAD ? p.prep_bwd : p.prep_fwd).push_back(j);
}

// The scratch regions both plan kinds have, in their fixed order: `nslots`
// gradient slots of the largest activation (of HCU_NBUF offsets), the
// reduction rows, the weight-gradient slab arena, the weight re-layout scratch
// and the K-split partials.  The arena holds several layers' weight-gradient
// partials until their finalizes run together (at least one layer's, at most
// `arena_floor` floats beyond).  The slots, the arena and the re-layout
// scratch are backward-only: a forward-only plan has none.  The builder
// appends its own regions to the returned Region and sets scratch_bytes.
Region layout_scratch(PlanCore &p, int nslots, size_t arena_floor, bool fwd_only) {
  Region scratch;
  p.nbuf = nslots;
  for (int i = 0; i < HCU_NBUF; ++i)
    p.buf_off[i] = scratch.take_floats(fwd_only || i >= p.nbuf ? 0 : p.max_act);
  p.part_off = scratch.take_floats(p.need.part);
  p.wpart_floats = fwd_only ? 0 : p.need.arena_floats(arena_floor);
  p.wpart_off = scratch.take_floats(p.wpart_floats);
  p.wprep_off = scratch.take_floats(fwd_only ? 0 : p.need.wprep);
  p.kpart_off = scratch.take_floats(std::max<size_t>(p.need.kpart, 1));
  return scratch;
}

// A training forward needs more than one value per channel in every BatchNorm.
int check_bn_counts(const PlanCore &p) {
  for (const ConvLayer *L : p.convs)
    if (L->bn.on && L->bn.count <= 1.0)
      return fail(HCU_ERR_INVALID, "Expected more than 1 value per channel when training");
  return 0;
}

// HCU_PLAN_LOG: the kernel family of every planned convolution with what it
// asks of the workspaces, the weight-gradient kernels with their partial
// slabs, and the slab arena against the largest request it will get
// (measurement).
void plan_log(const hcu_unet_plan &p) {
  if (!getenv("HCU_PLAN_LOG")) return;
  auto clog = [](const std::string &n, const std::string &role, const GConvArgs &a) {
    const dim3 g = conv_family(a).grid(a);
    fprintf(stderr, "conv %-8s %-8s %-10s grid %u x %u x %u lds %d rows %d partial %zu wimage %zu\n", n.c_str(),
            role.c_str(), conv_family(a).name, g.x, g.y, g.z, a.lds_bytes, gconv_rows(a), conv_partial_floats(a),
            wprep_floats(a));
  };
  auto wlog = [](const std::string &n, const WGradArgs &w) {
    fprintf(stderr, "wgrad %-8s %-7s KB %5d M %5d N %4d slabs %7.2f MB grid %d x %d x %d\n", n.c_str(),
            wgrad_family(w).name, w.KB, w.Mtot, w.Ntot, 4e-6 * w.KB * (double)w.Mtot * w.Ntot, w.KB, w.mchunks,
            w.nchunks);
  };
  for (const ConvLayer *cl : p.convs) {
    clog(cl->name, "fwd", cl->fwd);
    if (cl->has_dgrad) clog(cl->name, "dgrad", cl->dgrad);
    wlog(cl->name, cl->wg.w);
  }
  for (const ConvTLayer *up : p.convts) {
    const ConvTLayer &u = *up;
    if (u.fused) clog(u.name, "up.fwd", u.fwdf);
    for (size_t ph = 0; !u.fused && ph < u.phases.size(); ++ph) clog(u.name, "ph" + std::to_string(ph), u.phases[ph]);
    clog(u.name, "up.dgrad", u.dgrad);
    // (the weight-gradient form the executor runs)
    const WGradJob &opt = p.is_chain ? u.wgs : u.wgp;
    wlog(u.name, (opt.on ? opt : u.wg).w);
  }
  // (a forward-only plan has no arena and runs no weight gradient)
  fprintf(stderr, "arena %zu largest slab %zu\n", p.wpart_floats, p.wpart_floats ? p.need.slab : (size_t)0);
}

}  // namespace hcu
