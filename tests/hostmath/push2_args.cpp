// TEST-ONLY stand-alone program (tests/test_push2_host.py builds it with the host sanitizers): the argument checks of
// thx_push2_eval / thx_push2_error run on the host before any launch.  Linked with csrc/push_kernels.hip alone, so the library's
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
  alignas(32) static char buf[128];
  void* p = buf;
  const thx_push2_term* t = reinterpret_cast<const thx_push2_term*>(buf);
  const thx_push2_term* t_odd = reinterpret_cast<const thx_push2_term*>(buf + 4);
  const thx_se2_eps eps = {1e-6, 1e-3};
  expect(thx_push2_eval(nullptr, 3, p, 12, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "null pointer", "eval terms = NULL");
  expect(thx_push2_eval(t, 3, nullptr, 12, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "null pointer", "eval x = NULL");
  expect(thx_push2_eval(t, 3, p, 12, nullptr, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "null pointer", "eval J = NULL");
  expect(thx_push2_eval(t, 3, p, 12, p, 40, nullptr, 12, 12, 2, THX_F32, &eps, nullptr), "null pointer", "eval e = NULL");
  expect(thx_push2_eval(t, 3, p, 12, p, 40, p, 12, 12, 2, THX_F32, nullptr, nullptr), "null pointer", "eval eps = NULL");
  expect(thx_push2_eval(t, 3, p, 12, p, 40, p, 12, 12, 2, 7, &eps, nullptr), "dtype", "eval dtype");
  expect(thx_push2_eval(t, 0, p, 12, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "n_terms", "eval n_terms = 0");
  expect(thx_push2_eval(t, 3, p, 12, p, 40, p, 12, 12, 0, THX_F32, &eps, nullptr), "batch", "eval B = 0");
  expect(thx_push2_eval(t, 3, p, 0, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "V < 1", "eval V = 0");
  expect(thx_push2_eval(t, 3, p, 12, p, 40, p, 11, 12, 2, THX_F32, &eps, nullptr), "lde < m", "eval lde");
  expect(thx_push2_eval(t, 3, p, 12, p, 40, p, 12, 0, 2, THX_F32, &eps, nullptr), "lde < m", "eval m = 0");
  expect(thx_push2_eval(t, 3, p, 12, p, 2, p, 12, 12, 2, THX_F32, &eps, nullptr), "j_total", "eval j_total");
  expect(thx_push2_eval(t, INT32_MAX, p, 12, p, 40, p, 12, 12, INT32_MAX, THX_F32, &eps, nullptr), "grid limit", "eval grid limit");
  expect(thx_push2_eval(t_odd, 3, p, 12, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "aligned", "eval terms alignment");
  expect(thx_push2_eval(t, 3, buf + 8, 12, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "aligned", "eval x alignment (one fp32 record)");
  expect(thx_push2_eval(t, 3, buf + 16, 12, p, 40, p, 12, 12, 2, THX_F64, &eps, nullptr), "aligned", "eval x alignment (one fp64 record)");
  expect(thx_push2_eval(t, 3, p, 12, buf + 4, 40, p, 12, 12, 2, THX_F64, &eps, nullptr), "aligned", "eval J alignment (fp64)");
  expect(thx_push2_eval(t, 3, p, 12, p, 40, buf + 2, 12, 12, 2, THX_F32, &eps, nullptr), "aligned", "eval e alignment");
  expect(thx_push2_error(nullptr, 3, p, 12, p, 2, THX_F32, &eps, nullptr), "null pointer", "error terms = NULL");
  expect(thx_push2_error(t, 3, nullptr, 12, p, 2, THX_F32, &eps, nullptr), "null pointer", "error x = NULL");
  expect(thx_push2_error(t, 3, p, 12, nullptr, 2, THX_F32, &eps, nullptr), "null pointer", "error err = NULL");
  expect(thx_push2_error(t, 3, p, 12, p, 2, THX_F32, nullptr, nullptr), "null pointer", "error eps = NULL");
  expect(thx_push2_error(t, 3, p, 12, p, 2, -1, &eps, nullptr), "dtype", "error dtype");
  expect(thx_push2_error(t, -2, p, 12, p, 2, THX_F64, &eps, nullptr), "n_terms", "error n_terms < 0");
  expect(thx_push2_error(t, 3, p, 12, p, -1, THX_F64, &eps, nullptr), "batch", "error B < 0");
  expect(thx_push2_error(t, 3, p, -4, p, 2, THX_F64, &eps, nullptr), "V < 1", "error V < 0");
  expect(thx_push2_error(t, 3, buf + 8, 12, p, 2, THX_F32, &eps, nullptr), "aligned", "error x alignment");
  expect(thx_push2_error(t, 3, p, 12, buf + 4, 2, THX_F64, &eps, nullptr), "aligned", "error err alignment (fp64)");
  std::printf(failures ? "%d FAILED\n" : "ALL REFUSED (%d failures)\n", failures);
  return failures != 0;
}
