// Stand-alone host program for a sanitizer run of hcu_ingest_jobs' validation
// (tools/ingest_validate_asan.sh): every job here is rejected on the host, so
// nothing is enqueued and no device is needed.  The index maps are heap
// arrays of exactly ox / oy entries, so a validation that read past a map
// would be reported.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "hcunet.h"

namespace hcu {   // the two error helpers of unet.cpp, which this program does not link
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
  std::printf(bad ? "ingest validation: %d failures\n" : "ingest validation: ok\n", bad);
  return bad ? 1 : 0;
}
