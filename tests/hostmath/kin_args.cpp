// TEST-ONLY stand-alone program (tests/test_kin_host.py builds it with the host sanitizers): the argument checks of
// thx_kin_eval / thx_kin_error run on the host before any launch.  Linked with csrc/kin_kernels.hip alone, so the library's error
// string lives here.
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
  static_assert(sizeof(thx_kin_term) == 128, "thx_kin_term is one 128-byte record");
  static_assert(sizeof(thx_kin_joint) == 128, "thx_kin_joint is one 128-byte record");
  alignas(16) static char buf[64];
  void* p = buf;
  const thx_kin_term* t = reinterpret_cast<const thx_kin_term*>(buf);
  const thx_kin_term* t_odd = reinterpret_cast<const thx_kin_term*>(buf + 4);
  const thx_kin_joint* q = reinterpret_cast<const thx_kin_joint*>(buf);
  const thx_kin_joint* q_odd = reinterpret_cast<const thx_kin_joint*>(buf + 4);
  const thx_lie_eps eps = {1e-2, 1e-2, 1e-2};
  const int F32 = THX_F32, F64 = THX_F64;
  // (terms, n_terms, paths, n_paths, x, ldx, n, dof, J, j_total, e, lde, m, B, dtype, eps, stream)
  expect(thx_kin_eval(nullptr, 3, q, 8, p, 16, 14, 7, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "null pointer", "eval terms = NULL");
  expect(thx_kin_eval(t, 3, nullptr, 8, p, 16, 14, 7, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "null pointer", "eval paths = NULL");
  expect(thx_kin_eval(t, 3, q, 8, nullptr, 16, 14, 7, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "null pointer", "eval x = NULL");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 7, nullptr, 80, p, 20, 20, 2, F32, &eps, nullptr), "null pointer", "eval J = NULL");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 7, p, 80, nullptr, 20, 20, 2, F32, &eps, nullptr), "null pointer", "eval e = NULL");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 7, p, 80, p, 20, 20, 2, F32, nullptr, nullptr), "null pointer", "eval eps = NULL");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 7, p, 80, p, 20, 20, 2, 7, &eps, nullptr), "dtype", "eval dtype");
  expect(thx_kin_eval(t, 0, q, 8, p, 16, 14, 7, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "n_terms", "eval n_terms = 0");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 7, p, 80, p, 20, 20, 0, F32, &eps, nullptr), "batch", "eval B = 0");
  expect(thx_kin_eval(t, 3, q, -1, p, 16, 14, 7, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "n_paths < 0", "eval n_paths < 0");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 0, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "dof < 1", "eval dof = 0");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 6, 7, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "n < dof", "eval n < dof");
  expect(thx_kin_eval(t, 3, q, 8, p, 13, 14, 7, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "ldx < n", "eval ldx");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 7, p, 80, p, 19, 20, 2, F32, &eps, nullptr), "lde < m", "eval lde");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 7, p, 80, p, 20, 0, 2, F32, &eps, nullptr), "lde < m", "eval m = 0");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 7, p, 6, p, 20, 20, 2, F32, &eps, nullptr), "j_total < dof", "eval j_total");
  expect(thx_kin_eval(t, INT32_MAX, q, 8, p, 16, 14, 7, p, 80, p, 20, 20, INT32_MAX, F32, &eps, nullptr),
         "grid limit exceeded (n_terms * B)", "eval grid limit");
  expect(thx_kin_eval(t_odd, 3, q, 8, p, 16, 14, 7, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "aligned", "eval terms alignment");
  expect(thx_kin_eval(t, 3, q_odd, 8, p, 16, 14, 7, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "aligned", "eval paths alignment");
  expect(thx_kin_eval(t, 3, q, 8, buf + 2, 16, 14, 7, p, 80, p, 20, 20, 2, F32, &eps, nullptr), "aligned", "eval x alignment");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 7, buf + 4, 80, p, 20, 20, 2, F64, &eps, nullptr), "aligned", "eval J alignment (fp64)");
  expect(thx_kin_eval(t, 3, q, 8, p, 16, 14, 7, p, 80, buf + 2, 20, 20, 2, F32, &eps, nullptr), "aligned", "eval e alignment");
  // (terms, n_terms, paths, n_paths, x, ldx, n, dof, err, B, dtype, eps, stream)
  expect(thx_kin_error(nullptr, 3, q, 8, p, 16, 14, 7, p, 2, F32, &eps, nullptr), "null pointer", "error terms = NULL");
  expect(thx_kin_error(t, 3, nullptr, 8, p, 16, 14, 7, p, 2, F32, &eps, nullptr), "null pointer", "error paths = NULL");
  expect(thx_kin_error(t, 3, q, 8, nullptr, 16, 14, 7, p, 2, F32, &eps, nullptr), "null pointer", "error x = NULL");
  expect(thx_kin_error(t, 3, q, 8, p, 16, 14, 7, nullptr, 2, F32, &eps, nullptr), "null pointer", "error err = NULL");
  expect(thx_kin_error(t, 3, q, 8, p, 16, 14, 7, p, 2, F32, nullptr, nullptr), "null pointer", "error eps = NULL");
  expect(thx_kin_error(t, 3, q, 8, p, 16, 14, 7, p, 2, -1, &eps, nullptr), "dtype", "error dtype");
  expect(thx_kin_error(t, -2, q, 8, p, 16, 14, 7, p, 2, F64, &eps, nullptr), "n_terms", "error n_terms < 0");
  expect(thx_kin_error(t, 3, q, 8, p, 16, 14, 7, p, -1, F64, &eps, nullptr), "batch", "error B < 0");
  expect(thx_kin_error(t, 3, q, -3, p, 16, 14, 7, p, 2, F64, &eps, nullptr), "n_paths < 0", "error n_paths < 0");
  expect(thx_kin_error(t, 3, q, 8, p, 16, 14, -7, p, 2, F64, &eps, nullptr), "dof < 1", "error dof < 0");
  expect(thx_kin_error(t, 3, q, 8, p, 16, 5, 7, p, 2, F64, &eps, nullptr), "n < dof", "error n < dof");
  expect(thx_kin_error(t, 3, q, 8, p, 3, 14, 7, p, 2, F64, &eps, nullptr), "ldx < n", "error ldx");
  expect(thx_kin_error(t, 3, q, 8, p, 16, 14, 7, buf + 4, 2, F64, &eps, nullptr), "aligned", "error err alignment (fp64)");
  expect(thx_kin_error(t, 3, q_odd, 8, p, 16, 14, 7, p, 2, F32, &eps, nullptr), "aligned", "error paths alignment");
  std::printf(failures ? "%d FAILED\n" : "ALL REFUSED (%d failures)\n", failures);
  return failures != 0;
}
