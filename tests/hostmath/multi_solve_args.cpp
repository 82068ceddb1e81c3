// TEST-ONLY stand-alone program (tests/test_multi_solve_host.py builds it with the host sanitizers): the argument checks of
// thx_chol_solve_multi run on the host before any launch.  Linked with csrc/multi_solve_kernels.hip alone, so the library's
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
  alignas(16) static char buf[64];
  void* p = buf;
  const int64_t ld = 32, ldv = 20, bs = 100;
  expect(thx_chol_solve_multi(nullptr, ld, 20, 2, p, p, p, 5, ldv, bs, 0, THX_F32, nullptr), "null pointer", "L = NULL");
  expect(thx_chol_solve_multi(p, ld, 20, 2, nullptr, p, p, 5, ldv, bs, 0, THX_F32, nullptr), "null pointer", "Winv = NULL");
  expect(thx_chol_solve_multi(p, ld, 20, 2, p, nullptr, p, 5, ldv, bs, 0, THX_F32, nullptr), "null pointer", "rhs = NULL");
  expect(thx_chol_solve_multi(p, ld, 20, 2, p, p, nullptr, 5, ldv, bs, 0, THX_F32, nullptr), "null pointer", "x = NULL");
  expect(thx_chol_solve_multi(p, ld, 20, 2, p, p, p, 5, 19, bs, 0, THX_F32, nullptr), "ldv < n", "ldv");
  expect(thx_chol_solve_multi(p, ld, 20, 2, p, p, p, 5, ldv, 99, 0, THX_F32, nullptr), "bstride", "bstride");
  expect(thx_chol_solve_multi(p, ld, 20, 2, p, p, p, 5, INT64_MAX / 2, INT64_MAX, 0, THX_F32, nullptr), "bstride", "huge ldv");
  expect(thx_chol_solve_multi(p, ld, 20, 2, p, p, p, 5, ldv, bs, 3, THX_F32, nullptr), "which", "which = 3");
  expect(thx_chol_solve_multi(p, ld, 20, 2, p, p, p, 5, ldv, bs, -1, THX_F64, nullptr), "which", "which = -1");
  expect(thx_chol_solve_multi(p, ld, 20, 2, p, p, p, 5, ldv, bs, 0, 7, nullptr), "dtype", "dtype");
  expect(thx_chol_solve_multi(p, ld, 20, 2, p, p, p, 0, ldv, bs, 0, THX_F32, nullptr), "nrhs", "nrhs = 0");
  expect(thx_chol_solve_multi(p, 33, 20, 2, p, p, p, 5, ldv, bs, 0, THX_F32, nullptr), "ld", "ld % 32");
  expect(thx_chol_solve_multi(p, ld, 20, 64, p, p, p, INT32_MAX, ldv, INT64_MAX, 0, THX_F32, nullptr), "grid", "grid limit");
  expect(thx_chol_solve_multi(buf + 4, ld, 20, 2, p, p, p, 5, ldv, bs, 0, THX_F32, nullptr), "aligned", "alignment");
  std::printf(failures ? "%d FAILED\n" : "ALL REFUSED (%d failures)\n", failures);
  return failures != 0;
}
