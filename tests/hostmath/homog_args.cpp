// TEST-ONLY stand-alone program (tests/test_homog_host.py builds it with the host sanitizers): the argument checks of
// thx_homog_eval / thx_homog_error run on the host before any launch.  Linked with csrc/homog_kernels.hip alone, so the library's
// error string lives here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "theseus_hip.h"

namespace thx {
std::string& last_error() {
  static std::string e;
  return e;
}
}  // namespace thx

static int failures = 0;

static void expect(int rc, const char* needle, const char* what) {
  const std::string& e = thx::last_error();
  if (rc != -1 || e.find(needle) == std::string::npos) {
    std::printf("FAIL %s: rc=%d error='%s'\n", what, rc, e.c_str());
    ++failures;
  }
  thx::last_error().clear();
}

int main() {
  static_assert(sizeof(thx_homog_term) == 128, "thx_homog_term is one 128-byte record");
  alignas(16) static char buf[64];
  void* p = buf;
  const thx_homog_term* t = reinterpret_cast<const thx_homog_term*>(buf);
  const thx_homog_term* t_odd = reinterpret_cast<const thx_homog_term*>(buf + 4);
  const int F32 = THX_F32, F64 = THX_F64;
  // (terms, n_terms, n_align, x, ldx, n, scratch, chunks, J, j_total, e, lde, m, B, dtype, stream)
  expect(thx_homog_eval(nullptr, 3, 2, p, 16, 16, p, 5, p, 80, p, 10, 10, 2, F32, nullptr), "null pointer", "eval terms = NULL");
  expect(thx_homog_eval(t, 3, 2, nullptr, 16, 16, p, 5, p, 80, p, 10, 10, 2, F32, nullptr), "null pointer", "eval x = NULL");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, nullptr, 5, p, 80, p, 10, 10, 2, F32, nullptr), "null pointer", "eval scratch = NULL");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, 5, nullptr, 80, p, 10, 10, 2, F32, nullptr), "null pointer", "eval J = NULL");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, 5, p, 80, nullptr, 10, 10, 2, F32, nullptr), "null pointer", "eval e = NULL");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, 5, p, 80, p, 10, 10, 2, 7, nullptr), "dtype", "eval dtype");
  expect(thx_homog_eval(t, 0, 2, p, 16, 16, p, 5, p, 80, p, 10, 10, 2, F32, nullptr), "n_terms", "eval n_terms = 0");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, 5, p, 80, p, 10, 10, 0, F32, nullptr), "batch", "eval B = 0");
  expect(thx_homog_eval(t, 3, 2, p, 15, 16, p, 5, p, 80, p, 10, 10, 2, F32, nullptr), "ldx < n", "eval ldx");
  expect(thx_homog_eval(t, 3, 2, p, 16, 7, p, 5, p, 80, p, 10, 10, 2, F32, nullptr), "n < 8", "eval n");
  expect(thx_homog_eval(t, 3, 0, p, 16, 16, p, 5, p, 80, p, 10, 10, 2, F32, nullptr), "n_align", "eval n_align = 0");
  expect(thx_homog_eval(t, 3, 4, p, 16, 16, p, 5, p, 80, p, 10, 10, 2, F32, nullptr), "n_align", "eval n_align > n_terms");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, 0, p, 80, p, 10, 10, 2, F32, nullptr), "chunks < 1", "eval chunks = 0");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, 5, p, 80, p, 9, 10, 2, F32, nullptr), "lde < m", "eval lde");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, 5, p, 80, p, 10, 0, 2, F32, nullptr), "lde < m", "eval m = 0");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, 5, p, 7, p, 10, 10, 2, F32, nullptr), "j_total", "eval j_total");
  expect(thx_homog_eval(t, INT32_MAX, 1, p, 16, 16, p, 1, p, 80, p, 10, 10, INT32_MAX, F32, nullptr), "grid limit exceeded (n_terms * B)",
         "eval grid limit of the finish stage");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, INT32_MAX, p, 80, p, 10, 10, 2, F32, nullptr),
         "grid limit exceeded (n_align * B * chunks)", "eval grid limit of the partial stage");
  expect(thx_homog_eval(t, 3, 3, p, 16, 16, p, 1, p, 80, p, 10, 10, 1 << 30, F32, nullptr),
         "grid limit exceeded (n_align * B * chunks)", "eval grid limit of the partial stage (n_align * B)");
  expect(thx_homog_eval(t_odd, 3, 2, p, 16, 16, p, 5, p, 80, p, 10, 10, 2, F32, nullptr), "aligned", "eval terms alignment");
  expect(thx_homog_eval(t, 3, 2, buf + 2, 16, 16, p, 5, p, 80, p, 10, 10, 2, F32, nullptr), "aligned", "eval x alignment");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, buf + 4, 5, p, 80, p, 10, 10, 2, F32, nullptr), "aligned", "eval scratch alignment (fp64)");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, 5, buf + 4, 80, p, 10, 10, 2, F64, nullptr), "aligned", "eval J alignment (fp64)");
  expect(thx_homog_eval(t, 3, 2, p, 16, 16, p, 5, p, 80, buf + 2, 10, 10, 2, F32, nullptr), "aligned", "eval e alignment");
  // (terms, n_terms, n_align, x, ldx, n, scratch, chunks, err, B, dtype, stream)
  expect(thx_homog_error(nullptr, 3, 2, p, 16, 16, p, 5, p, 2, F32, nullptr), "null pointer", "error terms = NULL");
  expect(thx_homog_error(t, 3, 2, nullptr, 16, 16, p, 5, p, 2, F32, nullptr), "null pointer", "error x = NULL");
  expect(thx_homog_error(t, 3, 2, p, 16, 16, nullptr, 5, p, 2, F32, nullptr), "null pointer", "error scratch = NULL");
  expect(thx_homog_error(t, 3, 2, p, 16, 16, p, 5, nullptr, 2, F32, nullptr), "null pointer", "error err = NULL");
  expect(thx_homog_error(t, 3, 2, p, 16, 16, p, 5, p, 2, -1, nullptr), "dtype", "error dtype");
  expect(thx_homog_error(t, -2, 2, p, 16, 16, p, 5, p, 2, F64, nullptr), "n_terms", "error n_terms < 0");
  expect(thx_homog_error(t, 3, 2, p, 16, 16, p, 5, p, -1, F64, nullptr), "batch", "error B < 0");
  expect(thx_homog_error(t, 3, 2, p, 3, 16, p, 5, p, 2, F64, nullptr), "ldx < n", "error ldx");
  expect(thx_homog_error(t, 3, -1, p, 16, 16, p, 5, p, 2, F64, nullptr), "n_align", "error n_align < 0");
  expect(thx_homog_error(t, 3, 2, p, 16, 16, p, -4, p, 2, F64, nullptr), "chunks < 1", "error chunks < 0");
  expect(thx_homog_error(t, 3, 2, p, 16, 16, p, 5, buf + 4, 2, F64, nullptr), "aligned", "error err alignment (fp64)");
  expect(thx_homog_error(t, 3, 2, p, 16, 16, buf + 4, 5, p, 2, F32, nullptr), "aligned", "error scratch alignment (fp64)");
  expect(thx_homog_error(t, 3, 2, p, 16, 16, p, INT32_MAX, p, 2, F32, nullptr), "grid limit exceeded (n_align * B * chunks)",
         "error grid limit of the partial stage");
  std::printf(failures ? "%d FAILED\n" : "ALL REFUSED (%d failures)\n", failures);
  return failures != 0;
}
