// C-ABI plumbing: error reporting and version for libsegmentron_hip.so; the host-side entry
// points of the index-division helper (common.h: fast_div) that the CPU test sweeps.
#include "common.h"
#include <stdarg.h>
#include <stdio.h>

namespace seg {
static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return 2;
  }
  return 0;
}
}  // namespace seg

extern "C" const char* seg_last_error(void) { return seg::g_err; }
extern "C" int seg_version(void) { return 1; }

extern "C" int seg_fast_div_host(const int* s, long n, int d, int* q) {
  SEG_REQUIRE(s && q && n >= 0 && d >= 1, "fast_div_host: bad arguments");
  const float inv = 1.f / (float)d;
  for (long i = 0; i < n; ++i) q[i] = seg::fast_div(s[i], d, inv);
  return 0;
}
extern "C" int seg_fast_div_exact(long s, long d) { return seg::fast_div_exact(s, d) ? 1 : 0; }
extern "C" int seg_fast_div_max_quot(long* out) {
  SEG_REQUIRE(out != nullptr, "fast_div_max_quot: null output");
  *out = seg::FAST_DIV_MAX_QUOT;
  return 0;
}
