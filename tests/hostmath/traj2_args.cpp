// TEST-ONLY stand-alone program (tests/test_traj2_host.py builds it with the host sanitizers): the argument checks of
// thx_traj2_eval / thx_traj2_error run on the host before any launch.  Linked with csrc/traj_kernels.hip alone, so the library's
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
  const thx_traj2_term* t = reinterpret_cast<const thx_traj2_term*>(buf);
  const thx_traj2_term* t_odd = reinterpret_cast<const thx_traj2_term*>(buf + 4);
  expect(thx_traj2_eval(nullptr, 3, p, 28, 28, p, 40, p, 12, 12, 2, THX_F32, nullptr), "null pointer", "eval terms = NULL");
  expect(thx_traj2_eval(t, 3, nullptr, 28, 28, p, 40, p, 12, 12, 2, THX_F32, nullptr), "null pointer", "eval x = NULL");
  expect(thx_traj2_eval(t, 3, p, 28, 28, nullptr, 40, p, 12, 12, 2, THX_F32, nullptr), "null pointer", "eval J = NULL");
  expect(thx_traj2_eval(t, 3, p, 28, 28, p, 40, nullptr, 12, 12, 2, THX_F32, nullptr), "null pointer", "eval e = NULL");
  expect(thx_traj2_eval(t, 3, p, 28, 28, p, 40, p, 12, 12, 2, 7, nullptr), "dtype", "eval dtype");
  expect(thx_traj2_eval(t, 0, p, 28, 28, p, 40, p, 12, 12, 2, THX_F32, nullptr), "n_terms", "eval n_terms = 0");
  expect(thx_traj2_eval(t, 3, p, 28, 28, p, 40, p, 12, 12, 0, THX_F32, nullptr), "batch", "eval B = 0");
  expect(thx_traj2_eval(t, 3, p, 27, 28, p, 40, p, 12, 12, 2, THX_F32, nullptr), "ldx < n", "eval ldx");
  expect(thx_traj2_eval(t, 3, p, 28, 1, p, 40, p, 12, 12, 2, THX_F32, nullptr), "n < 2", "eval n");
  expect(thx_traj2_eval(t, 3, p, 28, 28, p, 40, p, 11, 12, 2, THX_F32, nullptr), "lde < m", "eval lde");
  expect(thx_traj2_eval(t, 3, p, 28, 28, p, 40, p, 12, 0, 2, THX_F32, nullptr), "lde < m", "eval m = 0");
  expect(thx_traj2_eval(t, 3, p, 28, 28, p, 1, p, 12, 12, 2, THX_F32, nullptr), "j_total", "eval j_total");
  expect(thx_traj2_eval(t, INT32_MAX, p, 28, 28, p, 40, p, 12, 12, INT32_MAX, THX_F32, nullptr), "grid limit", "eval grid limit");
  expect(thx_traj2_eval(t_odd, 3, p, 28, 28, p, 40, p, 12, 12, 2, THX_F32, nullptr), "aligned", "eval terms alignment");
  expect(thx_traj2_eval(t, 3, buf + 2, 28, 28, p, 40, p, 12, 12, 2, THX_F32, nullptr), "aligned", "eval x alignment");
  expect(thx_traj2_eval(t, 3, p, 28, 28, buf + 4, 40, p, 12, 12, 2, THX_F64, nullptr), "aligned", "eval J alignment (fp64)");
  expect(thx_traj2_eval(t, 3, p, 28, 28, p, 40, buf + 2, 12, 12, 2, THX_F32, nullptr), "aligned", "eval e alignment");
  expect(thx_traj2_error(nullptr, 3, p, 28, 28, p, 2, THX_F32, nullptr), "null pointer", "error terms = NULL");
  expect(thx_traj2_error(t, 3, nullptr, 28, 28, p, 2, THX_F32, nullptr), "null pointer", "error x = NULL");
  expect(thx_traj2_error(t, 3, p, 28, 28, nullptr, 2, THX_F32, nullptr), "null pointer", "error err = NULL");
  expect(thx_traj2_error(t, 3, p, 28, 28, p, 2, -1, nullptr), "dtype", "error dtype");
  expect(thx_traj2_error(t, -2, p, 28, 28, p, 2, THX_F64, nullptr), "n_terms", "error n_terms < 0");
  expect(thx_traj2_error(t, 3, p, 28, 28, p, -1, THX_F64, nullptr), "batch", "error B < 0");
  expect(thx_traj2_error(t, 3, p, 3, 28, p, 2, THX_F64, nullptr), "ldx < n", "error ldx");
  expect(thx_traj2_error(t, 3, p, 28, 28, buf + 4, 2, THX_F64, nullptr), "aligned", "error err alignment (fp64)");
  std::printf(failures ? "%d FAILED\n" : "ALL REFUSED (%d failures)\n", failures);
  return failures != 0;
}
