// The executor's plan and layer types, and what its files share of the
// planning side (layers.cpp).  A plan is built once per (spec, input shape):
// it resolves every layer's shapes exactly as hcat.unet.Unet_Constructor would
// see them (hcat/unet.py:16-143), reports the errors torch would raise, picks
// the kernel tiles, and lays out two caller-owned workspaces:
//   saved   - what backward needs from forward: the channels-last input, every
//             conv's pre-BatchNorm output y (post-activation values are
//             recomputed on load as relu(y*scale+shift)), pooled maps, the
//             up-convolution outputs U and the per-BatchNorm coefficients;
//   scratch - per-call temporaries: the gradient slots, reduction partials and
//             the re-laid-out weights of the layer in flight.
// One handle type, hcu_unet_plan, serves both plan kinds: a PlanCore that the
// shared helpers (exec.h) work on, extended by UnetPlan (unet.cpp) or
// ChainPlan (chain.cpp).
#pragma once
#include "common.h"
#include "timing.h"
#include "../../include/hcunet.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#define HCU_NBUF 32   // gradient slots (at most; Ctx::alloc)
#define HCU_NBUF_RING 6   // ring size when one slot per allocation does not fit
#define HCU_FORK_RING 16   // marker events of forks that cannot use the chain record

namespace hcu {

constexpr int kTargetBlocks = 1024;

// Activation tensor dims.  es = element bytes: 4 (fp32 path, channel stride a
// multiple of 4 = 16 bytes) or 2 (bf16 path, channel stride a multiple of 8).
struct Dims {
  int B = 0, X = 0, Y = 0, Z = 0, C = 0, Cs = 0, es = 4;
  // > 0: the channels are parts of part_c real channels, each padded to the
  // vector width on its own (a chain input that is the channel-wise cat of
  // channels-last chain outputs, hcu_chain_spec::in_part_channels)
  int part_c = 0;
  int64_t vox() const { return (int64_t)B * X * Y * Z; }
  // 4-byte slots the tensor occupies (buffers are carved in float units)
  size_t floats() const { return ((size_t)vox() * Cs * es + 3) / 4; }
};

Dims mkdims(int B, int X, int Y, int Z, int C, int es);

struct Region {
  size_t off = 0;
  size_t take_floats(size_t n) {
    const size_t o = off;
    off = align_up(off + n * sizeof(float), 256);
    return o;
  }
};

struct BNLayer {
  bool on = false;      // the layer is followed by BatchNorm3d + ReLU (a chain's conv may not be)
  int C = 0, Cs = 0;
  size_t coef_off = 0;  // saved: 6 arrays of Cs floats
  int64_t gamma = 0, beta = 0;
  int index = 0;
  double count = 0;
};

// One planned weight gradient: the kernel's arguments, the finalize of its
// slabs (the shape fields; run_wgrad adds the pointers) and the floats it takes
// from the slab arena.  The plan sizes the arena from `slab` / `pw_slab`, and
// run_wgrad requests exactly those.
struct WGradJob {
  WGradArgs w{};
  WGradFinalize f{};
  bool on = false;       // planned (ConvTLayer's optional forms)
  // > 0: a bf16 1x1x1 Conv3d whose input carries no BatchNorm+ReLU runs the
  // pointwise VALU form (pw_wgrad_kernel) on this many blocks, one slab each
  int pw_blocks = 0;
  size_t slab = 0, pw_slab = 0;   // slab floats of the planned kernel / of the pointwise form
};

inline long wgrad_gvox(const WGradArgs &w) { return (long)w.B * w.GX * w.GY * w.GZ; }

// What a plan's kernels need from scratch besides the activations: every
// region is sized for the largest request of its kind.
struct ScratchNeed {
  size_t wprep = 0, part = 0, kpart = 0;
  size_t slab = 0;   // the largest single request to the slab arena
  // reduction rows in `part` (BatchNorm statistics, column sums)
  void rows(size_t floats) { part = std::max(part, floats); }
  // a convolution: its weight image, its K-split partials and `stat` floats
  // per (row, column) of epilogue statistics
  void conv(const GConvArgs &a, int stat = 0) {
    wprep = std::max(wprep, wprep_floats(a));
    kpart = std::max(kpart, conv_partial_floats(a));
    rows((size_t)gconv_rows(a) * a.CoutW * stat);
  }
  // an arena request (Ctx::slab)
  void arena(size_t floats) { slab = std::max(slab, floats); }
  // a weight gradient: the arena holds either form's slabs (`part` has always
  // been sized for the planned kernel's too, which the per-op entry points use)
  void job(const WGradJob &j) {
    rows(j.slab);
    arena(std::max(j.slab, j.pw_slab));
  }
  // floats of the arena: every request fits, `floor` floats for batching finalizes
  size_t arena_floats(size_t floor) const { return std::max({part, slab, floor}); }
};

struct ConvLayer {
  std::string name;  // layer tag for per-layer timing ("d0.c1", "u3.c2", ...)
  int Cout = 0, Cin_g = 0, groups = 1, fold_mod = 0, E = 0, T = 0;
  int part_c = 0, part_cs = 0;   // input channel parts (Dims::part_c): packed e <-> torch channel
  int K[3], D[3];
  int S[3] = {1, 1, 1}, P[3] = {0, 0, 0};   // stride, zero padding (chains; the U-Net is valid)
  bool has_dgrad = true;                   // input gradient planned (stride 1)
  // Dilated convolution run on the dilation sub-lattices (space-to-batch):
  // when the dilated halo does not fit the conv kernels' LDS, the input is
  // re-laid as dx*dy*dz dense sub-grids [B*D][X'][Y'][Z'] and fwd / dgrad /
  // wgrad are planned as dilation-1 convolutions on them (padding P/D).
  bool s2b = false;
  int L3[3] = {1, 1, 1};                   // lattice (= D) of the s2b form
  bool pw = false;                         // bf16 1x1x1, no BatchNorm input: pwconv.hip (forward, dgrad)
  Dims sub_in, sub_out;                    // sub-grid tensors (batch B*D)
  int64_t w_off = 0, b_off = 0;
  Dims in, out;
  GConvArgs fwd{}, dgrad{};
  WGradJob wg;
  BNLayer bn;
  size_t y_off = 0;
  size_t wf_off = 0, wd_off = 0;  // prepared fwd / dgrad weight images in `saved`
};

struct ConvTLayer {
  std::string name;
  int Cin = 0, Cout = 0, T = 0;
  int K[3], S[3];
  int64_t w_off = 0, b_off = 0;
  Dims in, out;
  Dims full;            // the output before the crop of a padded layer (== out without padding)
  std::vector<GConvArgs> phases;
  std::vector<int> pJ;  // 6 ints per phase: px,py,pz,Jx,Jy,Jz
  bool fused = false;   // kernel % stride == 0: all phases in one GEMM (N = phase x Cout)
  GConvArgs fwdf{};
  GConvArgs dgrad{};
  WGradJob wg;   // rows ci, columns (tap, co): every layer
  // the weight gradient of the phase-folded forward (WGradArgs::nph: phases
  // as extra columns; the bias from the column-sum rows of dU), fp32 U-Net
  // decoders with kernel % stride == 0 and Cout % 4 == 0
  WGradJob wgp;
  // layer chains, bf16, no BatchNorm+ReLU applied to the input: the weight
  // gradient as the Conv3d weight gradient of the input-gradient convolution
  // (rows (tap, co) over the strided dU halo, columns ci over x; finalize
  // mode 0 with Cout = Cin, Cin_g = Cout -- the [Cin][Cout][K] layout of a
  // ConvTranspose3d weight is a Conv3d weight's [Cout][Cin][K]): every tap in
  // one block, instead of a (tap, co)-column GEMM with one 16-row subtile
  WGradJob wgs;
  size_t u_off = 0;
  size_t wf_off = 0, wd_off = 0;   // prepared weights in `saved` (fused fwd, dgrad)
  std::vector<size_t> wph_off;     // per-phase fwd weights when not fused
};

inline BNCoef coef_at(char *saved, const BNLayer &bn) {
  float *b = reinterpret_cast<float *>(saved + bn.coef_off);
  BNCoef c;
  c.scale = b;
  c.shift = b + bn.Cs;
  c.mean = b + 2 * bn.Cs;
  c.invstd = b + 3 * bn.Cs;
  c.c1 = b + 4 * bn.Cs;
  c.c0 = b + 5 * bn.Cs;
  return c;
}

// What both plan kinds have and every shared helper works on.
struct PlanCore {
  int B = 0, X = 0, Y = 0, Z = 0;
  int es = 4;          // activation element bytes: 4 (fp32 path) or 2 (bf16 path)
  float bn_eps = 0.f, bn_momentum = 0.f;
  Dims xin, outd;
  size_t xcl_off = 0;
  int n_bn = 0;
  // Every Conv3d / ConvTranspose3d layer of the plan in forward order: pointers
  // into the builder's own vectors, set once those have their final size
  // (plans are heap objects and never copied).
  std::vector<ConvLayer *> convs;
  std::vector<ConvTLayer *> convts;
  std::vector<PrepJob> prep_jobs;  // weight re-layouts, one batched launch per forward
  // the same split: images the forward reads / input-gradient images only the
  // backward reads (re-laid on the branch stream while the forward runs)
  std::vector<PrepJob> prep_fwd, prep_bwd;
  size_t saved_bytes = 0, scratch_bytes = 0;
  // scratch layout
  // Backward gradient buffers: a ring of HCU_NBUF activation-sized slots, so
  // a slot read by the weight-gradient branch is rewritten only several
  // layers later (see Ctx::alloc).
  size_t buf_off[HCU_NBUF] = {};
  // slots in use: one per allocation of a U-Net backward when they fit (no
  // slot is rewritten, so no reader events or waits on the gradient ring),
  // else a ring of HCU_NBUF_RING (chains, very large activations)
  int nbuf = HCU_NBUF_RING;
  bool no_reuse = false;
  size_t part_off = 0, wpart_off = 0, wprep_off = 0, kpart_off = 0;
  size_t wpart_floats = 0;   // weight-gradient slab arena (deferred, batched finalizes)
  size_t max_act = 0;
  ScratchNeed need;
  // layer chains: the packed weight images are saved[img_lo, img_lo + img_bytes)
  size_t img_lo = 0, img_bytes = 0;
  PlanCore() = default;
  PlanCore(const PlanCore &) = delete;
  PlanCore &operator=(const PlanCore &) = delete;
};

}  // namespace hcu

// The opaque handle of the C ABI: the core and which kind extends it.
struct hcu_unet_plan : hcu::PlanCore {
  const bool is_chain;
  explicit hcu_unet_plan(bool chain) : is_chain(chain) {}
  virtual ~hcu_unet_plan() = default;
};

namespace hcu {

// ---- layers.cpp: layer planning ----
GConvArgs gconv_conv_fwd(const Dims &in, const Dims &out, const int K[3], const int D[3], int Cout);
GConvArgs gconv_conv_dgrad(const Dims &in, const Dims &out, const int K[3], const int D[3], int E);
WGradArgs wgrad_conv(const Dims &in, const Dims &out, const int K[3], const int D[3]);
void set_pw(ConvLayer &L, const Dims &in, int cin_total);
int setup_conv(ConvLayer &L, const Dims &in, int Cout, int groups, int fold_mod, int cin_total,
               const int K[3], const int D[3], const char *name, bool sublattice = false,
               const int *S = nullptr, const int *P = nullptr);
int setup_convt(ConvTLayer &u, const Dims &cur, int o, const int K[3], const int S[3],
                const int *pad, bool swap, ScratchNeed &need);
void track_conv(PlanCore &p, const ConvLayer &L);
// The weight re-layout jobs (prep_all.hip) of a layer's images.
PrepJob conv_fwd_job(const ConvLayer &cl);
PrepJob conv_dgrad_job(const ConvLayer &cl);
PrepJob convt_fused_job(const ConvTLayer &u);
PrepJob convt_phase_job(const ConvTLayer &u, size_t ph);
PrepJob convt_dgrad_job(const ConvTLayer &u);
void conv_prep(PlanCore &p, Region &saved, ConvLayer &cl);
void convt_prep(PlanCore &p, Region &saved, ConvTLayer &u);
void split_prep(PlanCore &p);
Region layout_scratch(PlanCore &p, int nslots, size_t arena_floor, bool fwd_only);
void plan_log(const hcu_unet_plan &p);
int check_bn_counts(const PlanCore &p);

// Allocates a plan of one kind for the input shape and runs its builder.
template <class Plan, class Build>
int create_plan(int B, int X, int Y, int Z, hcu_unet_plan **out, Build build) {
  auto *p = new Plan();
  p->B = B;
  p->X = X;
  p->Y = Y;
  p->Z = Z;
  const int e = build(*p);
  *out = e ? nullptr : p;
  if (e) delete p;
  return e;
}

}  // namespace hcu
