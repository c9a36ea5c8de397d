// The kernel families of the convolution and weight-gradient GEMMs: one record
// per family (common.h) and the ladders that choose a family for a shape.
// Host code only; the planners and launchers are in the kernels' files.
#include "common.h"

namespace hcu {
namespace {

// clang-format off
const ConvFamily kConv[] = {
    // name, plan, launch, grid, stat_rows, ksplit, wpack, wbytes, bnbwd, folds_phases, ncx_ok
    {"gconv", plan_gconv, launch_gconv, gconv_grid,
     [](const GConvArgs &a) { return a.B * a.ntx * a.nty * a.ntz; }, false, 0, 4, false, false, nullptr},
    {"conv2", plan_conv2, launch_conv2, conv2_grid,
     [](const GConvArgs &a) { return ksplit_stat_rows(a, 4); }, true, 1, 4, true, true, nullptr},
    {"conv8", plan_conv8, launch_conv8, [](const GConvArgs &a) { return dim3(a.gridx); },
     [](const GConvArgs &a) { return a.gridx; }, false, 2, 4, true, false, conv8_ncx_ok},
    {"bconv-f32", [](GConvArgs &a, int tb) { a.bes = 4; return plan_bconv(a, tb); }, launch_bconv, conv2_grid,
     [](const GConvArgs &a) { return ksplit_stat_rows(a, 4); }, true, 1, 4, true, true, bconv_ncx_ok},
    {"bconv-bf16", [](GConvArgs &a, int tb) { a.bes = 2; return plan_bconv(a, tb); }, launch_bconv, conv2_grid,
     [](const GConvArgs &a) { return ksplit_stat_rows(a, 8); }, true, 3, 2, true, true, bconv_ncx_ok},
};
const WGradFamily kWGrad[] = {   // name, launch, real_rows (in WGradKern order)
    {"wgrad", launch_wgrad_generic, false}, {"wgrad2", launch_wgrad2, false}, {"wgrad8", launch_wgrad8, false},
    {"wgrad3", launch_wgrad3, false},       {"bwgrad", launch_bwgrad, true},
};
// clang-format on

// The off-switches of the ladders below (the A/B sides and fallbacks of
// tests/test_gpu_modes.py), read once: NAME=1 takes the family out of its
// ladder, and so does HCU_WGRAD3=0 for wgrad3.
struct Off {
  bool conv8, conv2, bconv_f32, wgrad8, wgrad2, wgrad3;
};
const Off &off() {
  auto is = [](const char *name, char v) {
    const char *e = getenv(name);
    return e && e[0] == v;
  };
  static const Off o = {is("HCU_NO_CONV8", '1'),  is("HCU_NO_CONV2", '1'),  is("HCU_NO_BCONV_F32", '1'),
                        is("HCU_NO_WGRAD8", '1'), is("HCU_NO_WGRAD2", '1'), is("HCU_WGRAD3", '0')};
  return o;
}

// Plans `a` with family f on a copy: a family that refuses leaves `a` as it was.
bool take(const ConvFamily &f, GConvArgs &a, int target_blocks) {
  GConvArgs b = a;
  if (f.plan(b, target_blocks) != 0) return false;
  a = b;
  return true;
}

}  // namespace

const ConvFamily &conv_family(int kern, int bes) { return kConv[kern + (kern == KCONV_BCONV && bes != 4)]; }
const WGradFamily &wgrad_family(const WGradArgs &a) { return kWGrad[a.kern]; }

// fp32: the blocked MFMA kernel (bconv on fp32 elements) for 16 output columns
// or more (with fewer, conv8's 4x4 MFMA blocks waste no MFMA rows), then
// conv8, conv2 and the generic gconv, whose error is the ladder's.  bf16:
// bconv only, its error as it stands.
int plan_conv(GConvArgs &a, int es, int target_blocks) {
  if (es == 2) return conv_family(KCONV_BCONV, 2).plan(a, target_blocks);
  if (!off().bconv_f32 && a.Cout * std::max(1, a.nph) >= 16 && take(conv_family(KCONV_BCONV, 4), a, target_blocks))
    return 0;
  a.cph = 0;   // (bconv only)
  if (!off().conv8 && take(kConv[KCONV_CONV8], a, target_blocks)) return 0;
  if (!off().conv2 && take(kConv[KCONV_CONV2], a, target_blocks)) return 0;
  return kConv[KCONV_GCONV].plan(a, target_blocks);
}

// fp32: wgrad3 (deep layers and the ConvTranspose3d phase form, the
// output-split kernel), then wgrad8, wgrad2 and the generic kernel; the phase
// form (nph > 1) has only wgrad2 behind wgrad3.  bf16: bwgrad only.
int plan_wgrad_any(WGradArgs &a, int es, int target_blocks) {
  if (es == 2) return plan_bwgrad(a);
  if (int e = plan_wgrad_generic(a, target_blocks)) return e;
  if (!off().wgrad3 && plan_wgrad3(a) == 0) return 0;
  if (a.nph > 1) {
    if (off().wgrad2 || plan_wgrad2(a) != 0)
      return fail(4, "wgrad: no wgrad2 tile for the ConvTranspose3d phase form");
    return 0;
  }
  if ((off().wgrad8 || plan_wgrad8(a) != 0) && !off().wgrad2) plan_wgrad2(a);
  return 0;
}

}  // namespace hcu
