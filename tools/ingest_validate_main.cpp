// Stand-alone host program for a sanitizer run of hcu_ingest_jobs' validation
// (tools/ingest_validate_asan.sh): every job here is rejected on the host, so
// nothing is enqueued and no device is needed.  The index maps are heap
// arrays of exactly ox / oy entries -- rot_nx / rot_ny for a rotated job, whose
// maps describe the pre-rotation view -- so a validation that read past a map
// would be reported.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "hcunet.h"

namespace hcu {   // the two error helpers of error.cpp, which this program does not link
static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
}  // namespace hcu

static hcu_ingest_job valid_job() {
  hcu_ingest_job j{};
  j.src = (const void *)0x1000;
  j.dst = (void *)0x2000;
  j.src_dtype = HCU_U16;
  j.Z = 8, j.Y = 20, j.X = 30, j.C = 4;
  j.ox = 10, j.oy = 10, j.oz = 4;
  j.x0 = 20, j.y0 = 10, j.z0 = 4;
  j.n_chan = 4;
  for (int c = 0; c < 4; ++c) j.chan[c] = c;
  j.scale = 1.0 / 65536;
  return j;
}

// The 12x10 window at (18, 10) rotated by 30 degrees; the output is the 10x8
// window at (1, 2) of the rotated view, filled after the first of two steps.
static hcu_ingest_job rotated_job() {
  hcu_ingest_job j = valid_job();
  j.ox = 10, j.oy = 8;
  j.x0 = 18, j.y0 = 10;
  j.n_steps = 2;
  j.steps[0].kind = j.steps[1].kind = HCU_AUG_CLEAN;
  const double c = std::sqrt(3.0) / 2, s = 0.5, cx = 5.5, cy = 4.5;
  j.rot = 1;
  j.rot_m[0] = c, j.rot_m[1] = s, j.rot_m[2] = -s, j.rot_m[3] = c;
  j.rot_off[0] = cx - (c * cx + s * cy);
  j.rot_off[1] = cy - (-s * cx + c * cy);
  j.rot_nx = 12, j.rot_ny = 10;
  j.rot_px = 1, j.rot_py = 2;
  j.fill_after = 1;
  return j;
}

static int bad = 0;
static void expect(const char *what, const hcu_ingest_job &j, int code) {
  const int rc = hcu_ingest_jobs(&j, (const hcu_ingest_job *)0x3000, 1, nullptr);
  if (rc != code) {
    std::printf("FAIL %s: got %d, expected %d (%s)\n", what, rc, code, hcu::g_err.c_str());
    ++bad;
  }
}

int main() {
  hcu_ingest_job j = valid_job();
  j.x0 = 21;
  expect("x window past the source", j, HCU_ERR_SHAPE);
  j = valid_job();
  j.z0 = -1;
  expect("negative z origin", j, HCU_ERR_SHAPE);
  std::vector<int> xmap(10), ymap(10);
  for (int i = 0; i < 10; ++i) xmap[i] = 20 + i, ymap[i] = i;
  j = valid_job();
  j.xmap_dev = (const int *)0x4000;
  j.xmap_host = xmap.data();
  xmap[9] = 30;
  expect("map entry equal to X", j, HCU_ERR_SHAPE);
  xmap[9] = 29;
  j.ymap_dev = (const int *)0x5000;
  j.ymap_host = ymap.data();
  ymap[0] = -1;
  expect("negative map entry", j, HCU_ERR_SHAPE);
  j = valid_job();
  j.C = 17;
  expect("17 channels", j, HCU_ERR_UNSUPPORTED);
  j = valid_job();
  j.n_steps = 9;
  expect("9 steps", j, HCU_ERR_UNSUPPORTED);
  j = valid_job();
  j.oz = 0;
  expect("empty extent", j, HCU_ERR_SHAPE);
  j = valid_job();
  j.chan[3] = 4;
  expect("channel outside the source", j, HCU_ERR_INVALID);

  // rotated jobs
  j = rotated_job();
  j.rot = 2;
  expect("rot = 2", j, HCU_ERR_INVALID);
  j = rotated_job();
  j.rot_m[1] = NAN;
  expect("NaN matrix entry", j, HCU_ERR_INVALID);
  j = rotated_job();
  j.rot_m[3] = 1.5;
  expect("matrix entry beyond 1", j, HCU_ERR_INVALID);
  j = rotated_job();
  j.rot_off[0] = INFINITY;
  expect("infinite offset", j, HCU_ERR_INVALID);
  j = rotated_job();
  j.rot_ny = 0;
  expect("empty pre-rotation view", j, HCU_ERR_SHAPE);
  j = rotated_job();
  j.rot_px = 3;
  expect("output window past the rotated view (x)", j, HCU_ERR_SHAPE);
  j = rotated_job();
  j.rot_py = -1;
  expect("negative origin in the rotated view (y)", j, HCU_ERR_SHAPE);
  j = rotated_job();
  j.x0 = 19;   // 19 + rot_nx > X although 19 + ox <= X
  expect("pre-rotation x window past the source", j, HCU_ERR_SHAPE);
  j = rotated_job();
  j.fill_after = 3;
  expect("fill_after beyond n_steps", j, HCU_ERR_INVALID);
  {
    // maps of exactly rot_nx / rot_ny entries: the bad one is the last, beyond the output's ox / oy
    std::vector<int> rx(12), ry(10);
    for (int i = 0; i < 12; ++i) rx[i] = 18 + i;
    for (int i = 0; i < 10; ++i) ry[i] = 10 + i;
    j = rotated_job();
    j.xmap_dev = (const int *)0x4000;
    j.xmap_host = rx.data();
    j.ymap_dev = (const int *)0x5000;
    j.ymap_host = ry.data();
    rx[11] = 30;
    expect("rotated: last x map entry equal to X", j, HCU_ERR_SHAPE);
    rx[11] = 29;
    ry[9] = -1;
    expect("rotated: last y map entry negative", j, HCU_ERR_SHAPE);
  }
  j = valid_job();
  j.rot_px = 1;
  expect("rot_px without rot", j, HCU_ERR_INVALID);
  j = valid_job();
  j.rot_m[0] = 1.0;
  expect("matrix without rot", j, HCU_ERR_INVALID);
  j = valid_job();
  j.fill_after = 1;
  expect("fill_after without rot", j, HCU_ERR_INVALID);
  std::printf(bad ? "ingest validation: %d failures\n" : "ingest validation: ok\n", bad);
  return bad ? 1 : 0;
}
