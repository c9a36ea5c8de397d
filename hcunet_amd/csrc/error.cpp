// The library's error channel: a thread-local message behind hcu_last_error().
#include "common.h"
#include "../../include/hcunet.h"

namespace hcu {
static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
}  // namespace hcu

extern "C" {

const char *hcu_last_error(void) { return hcu::g_err.c_str(); }
int hcu_version(void) { return 100; }

}  // extern "C"
