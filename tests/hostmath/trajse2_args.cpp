// TEST-ONLY stand-alone program (tests/test_trajse2_host.py builds it with the host sanitizers): the argument checks of
// thx_trajse2_eval / thx_trajse2_error / thx_trajse2_retract run on the host before any launch.  Linked with
// csrc/trajse2_kernels.hip alone, so the library's error string lives here.
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
  const uint8_t* k = reinterpret_cast<const uint8_t*>(buf);
  const thx_trajse2_term* t = reinterpret_cast<const thx_trajse2_term*>(buf);
  const thx_trajse2_term* t_odd = reinterpret_cast<const thx_trajse2_term*>(buf + 4);
  const thx_se2_eps eps = {1e-6, 1e-3};
  expect(thx_trajse2_eval(nullptr, 3, p, 12, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "null pointer", "eval terms = NULL");
  expect(thx_trajse2_eval(t, 3, nullptr, 12, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "null pointer", "eval x = NULL");
  expect(thx_trajse2_eval(t, 3, p, 12, nullptr, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "null pointer", "eval J = NULL");
  expect(thx_trajse2_eval(t, 3, p, 12, p, 40, nullptr, 12, 12, 2, THX_F32, &eps, nullptr), "null pointer", "eval e = NULL");
  expect(thx_trajse2_eval(t, 3, p, 12, p, 40, p, 12, 12, 2, THX_F32, nullptr, nullptr), "null pointer", "eval eps = NULL");
  expect(thx_trajse2_eval(t, 3, p, 12, p, 40, p, 12, 12, 2, 7, &eps, nullptr), "dtype", "eval dtype");
  expect(thx_trajse2_eval(t, 0, p, 12, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "n_terms", "eval n_terms = 0");
  expect(thx_trajse2_eval(t, 3, p, 12, p, 40, p, 12, 12, 0, THX_F32, &eps, nullptr), "batch", "eval B = 0");
  expect(thx_trajse2_eval(t, 3, p, 0, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "V < 1", "eval V = 0");
  expect(thx_trajse2_eval(t, 3, p, 12, p, 40, p, 11, 12, 2, THX_F32, &eps, nullptr), "lde < m", "eval lde");
  expect(thx_trajse2_eval(t, 3, p, 12, p, 40, p, 12, 0, 2, THX_F32, &eps, nullptr), "lde < m", "eval m = 0");
  expect(thx_trajse2_eval(t, 3, p, 12, p, 2, p, 12, 12, 2, THX_F32, &eps, nullptr), "j_total", "eval j_total");
  expect(thx_trajse2_eval(t, INT32_MAX, p, 12, p, 40, p, 12, 12, INT32_MAX, THX_F32, &eps, nullptr), "grid limit", "eval grid limit");
  expect(thx_trajse2_eval(t_odd, 3, p, 12, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "aligned", "eval terms alignment");
  expect(thx_trajse2_eval(t, 3, buf + 8, 12, p, 40, p, 12, 12, 2, THX_F32, &eps, nullptr), "aligned", "eval x alignment (one fp32 record)");
  expect(thx_trajse2_eval(t, 3, buf + 16, 12, p, 40, p, 12, 12, 2, THX_F64, &eps, nullptr), "aligned", "eval x alignment (one fp64 record)");
  expect(thx_trajse2_eval(t, 3, p, 12, buf + 4, 40, p, 12, 12, 2, THX_F64, &eps, nullptr), "aligned", "eval J alignment (fp64)");
  expect(thx_trajse2_eval(t, 3, p, 12, p, 40, buf + 2, 12, 12, 2, THX_F32, &eps, nullptr), "aligned", "eval e alignment");
  expect(thx_trajse2_error(nullptr, 3, p, 12, p, 2, THX_F32, &eps, nullptr), "null pointer", "error terms = NULL");
  expect(thx_trajse2_error(t, 3, nullptr, 12, p, 2, THX_F32, &eps, nullptr), "null pointer", "error x = NULL");
  expect(thx_trajse2_error(t, 3, p, 12, nullptr, 2, THX_F32, &eps, nullptr), "null pointer", "error err = NULL");
  expect(thx_trajse2_error(t, 3, p, 12, p, 2, THX_F32, nullptr, nullptr), "null pointer", "error eps = NULL");
  expect(thx_trajse2_error(t, 3, p, 12, p, 2, -1, &eps, nullptr), "dtype", "error dtype");
  expect(thx_trajse2_error(t, -2, p, 12, p, 2, THX_F64, &eps, nullptr), "n_terms", "error n_terms < 0");
  expect(thx_trajse2_error(t, 3, p, 12, p, -1, THX_F64, &eps, nullptr), "batch", "error B < 0");
  expect(thx_trajse2_error(t, 3, p, -4, p, 2, THX_F64, &eps, nullptr), "V < 1", "error V < 0");
  expect(thx_trajse2_error(t, 3, buf + 8, 12, p, 2, THX_F32, &eps, nullptr), "aligned", "error x alignment");
  expect(thx_trajse2_error(t, 3, p, 12, buf + 4, 2, THX_F64, &eps, nullptr), "aligned", "error err alignment (fp64)");
  expect(thx_trajse2_retract(nullptr, k, p, 36, 0.25, nullptr, p, 12, 2, THX_F32, &eps, nullptr), "null pointer", "retract x = NULL");
  expect(thx_trajse2_retract(p, nullptr, p, 36, 0.25, nullptr, p, 12, 2, THX_F32, &eps, nullptr), "null pointer", "retract var_kind = NULL");
  expect(thx_trajse2_retract(p, k, nullptr, 36, 0.25, nullptr, p, 12, 2, THX_F32, &eps, nullptr), "null pointer", "retract delta = NULL");
  expect(thx_trajse2_retract(p, k, p, 36, 0.25, nullptr, nullptr, 12, 2, THX_F32, &eps, nullptr), "null pointer", "retract out = NULL");
  expect(thx_trajse2_retract(p, k, p, 36, 0.25, nullptr, p, 12, 2, THX_F32, nullptr, nullptr), "null pointer", "retract eps = NULL");
  expect(thx_trajse2_retract(p, k, p, 36, 0.25, nullptr, p, 12, 2, 5, &eps, nullptr), "dtype", "retract dtype");
  expect(thx_trajse2_retract(p, k, p, 36, 0.25, nullptr, p, 0, 2, THX_F32, &eps, nullptr), "V < 1", "retract V = 0");
  expect(thx_trajse2_retract(p, k, p, 36, 0.25, nullptr, p, 12, 0, THX_F32, &eps, nullptr), "batch", "retract B = 0");
  expect(thx_trajse2_retract(p, k, p, 35, 0.25, nullptr, p, 12, 2, THX_F32, &eps, nullptr), "ldd < 3 * V", "retract ldd");
  expect(thx_trajse2_retract(buf + 8, k, p, 36, 0.25, nullptr, p, 12, 2, THX_F32, &eps, nullptr), "aligned", "retract x alignment");
  expect(thx_trajse2_retract(p, k, p, 36, 0.25, nullptr, buf + 16, 12, 2, THX_F64, &eps, nullptr), "aligned", "retract out alignment (fp64)");
  expect(thx_trajse2_retract(p, k, buf + 4, 36, 0.25, nullptr, p, 12, 2, THX_F64, &eps, nullptr), "aligned", "retract delta alignment (fp64)");
  expect(thx_trajse2_retract(p, k, p, (int64_t)3 * INT32_MAX, 0.25, nullptr, p, INT32_MAX, INT32_MAX, THX_F32, &eps, nullptr), "grid limit",
         "retract grid limit");
  std::printf(failures ? "%d FAILED\n" : "ALL REFUSED (%d failures)\n", failures);
  return failures != 0;
}
