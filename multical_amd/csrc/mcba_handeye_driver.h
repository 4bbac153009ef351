// mcba_handeye_driver.h -- host side of mcba_hand_eye that does not touch the device: argument checks, the usable pairs of every
// problem and the outputs of a call that launches nothing.  Shared by the driver (mcba_handeye.hip) and the host build of the
// mathematics (tests/handeye_host), so that both walk the same problems with the same inputs.
#pragma once
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_handeye.h"

namespace mcba {
namespace handeye {

struct Plan {
  std::vector<int32_t> n_pairs;     // [n_problems] frames valid on both sides
  long long usable = 0;             // their sum
  bool same_table = false;          // one upload serves both sides
};

inline bool plan_problems(const mcba_hand_eye_problem& p, Plan& out, std::string& err) {
  if (p.n_problems < 0 || p.F < 0 || p.n_a < 0 || p.n_b < 0) { err = "mcba_hand_eye: negative size"; return false; }
  out.n_pairs.assign((size_t)p.n_problems, 0);
  out.usable = 0;
  out.same_table = p.table_a == p.table_b && p.valid_a == p.valid_b && p.n_a == p.n_b;
  if (p.n_problems == 0) return true;
  if (!p.index_a || !p.index_b) { err = "mcba_hand_eye: null index list"; return false; }
  if (p.F > 0 && (!p.table_a || !p.valid_a || !p.table_b || !p.valid_b)) { err = "mcba_hand_eye: null table"; return false; }
  if ((long long)p.n_a * p.F >= (1ll << 31) / 16 || (long long)p.n_b * p.F >= (1ll << 31) / 16 ||
      (long long)p.n_problems * (p.F > 16 ? p.F : 16) >= (1ll << 31)) {
    err = "mcba_hand_eye: table too large";
    return false;
  }
  for (int k = 0; k < p.n_problems; ++k) {
    const long long ia = p.index_a[k], ib = p.index_b[k];
    if (ia < 0 || ia >= p.n_a || ib < 0 || ib >= p.n_b) {
      char msg[160];
      snprintf(msg, sizeof msg, "mcba_hand_eye: problem %d: rows (%lld, %lld) outside tables of %lld and %lld rows", k, ia, ib,
               (long long)p.n_a, (long long)p.n_b);
      err = msg;
      return false;
    }
    const uint8_t* va = p.valid_a + (size_t)ia * p.F;
    const uint8_t* vb = p.valid_b + (size_t)ib * p.F;
    int n = 0;
    for (int f = 0; f < p.F; ++f) n += (va[f] != 0 && vb[f] != 0);
    out.n_pairs[k] = n;
    out.usable += n;
  }
  return true;
}

// outputs of the problems that get no result (and the default of those that do); any pointer may be null
inline void fill_defaults(const mcba_hand_eye_problem& p, const Plan& plan, double* X, double* Z, int32_t* n_pairs, uint8_t* status,
                          double* err) {
  for (int k = 0; k < p.n_problems; ++k) {
    if (X) identity_pose(X + 16 * (size_t)k);
    if (Z) identity_pose(Z + 16 * (size_t)k);
    if (n_pairs) n_pairs[k] = plan.n_pairs[k];
    if (status) status[k] = (uint8_t)(plan.n_pairs[k] < MIN_PAIRS ? ST_TOO_FEW : ST_DEGENERATE);
    if (err)
      for (int f = 0; f < p.F; ++f) err[(size_t)k * p.F + f] = 0.0;
  }
}

}  // namespace handeye
}  // namespace mcba
