// rzk_keyplan.h — the host part of a key load: the range test of every coefficient, the classification of the
// (n+l)*k entries (KeyClass), their indices into the store of general entries, the general entries themselves and the
// bound of each one's 2-norm.  Host-only and pure: a KeyPlan is a function of the key and q, so it is tested without a
// GPU (tests/test_keyplan_host.py).  rzk_key.cpp goes through plan_key_tables: the context changes only once the key is accepted.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "rzk_plan.h"

namespace rzk {

struct KeyPlan {
  std::vector<uint8_t> key_class;   // (n+l)*k KeyClass values, row-major
  std::vector<int32_t> key_entry;   // index into the store of general entries, -1 if not KC_GENERAL
  uint32_t n_general = 0;
  std::vector<int64_t> general;     // the general entries' coefficients, n_general * N, in the order of their indices
  std::vector<double> kinf;         // per general entry: an upper bound of its 2-norm (prime-count bound), still one after
                                    // rounding to float
};

// a: entries * N coefficients (entries = (n+l)*k).  kPlanArg when a coefficient lies outside [-(q-1)/2, (q-1)/2]; `out`
// is written only on kPlanOk.
inline int plan_key(const int64_t* a, size_t entries, uint32_t N, int64_t q, KeyPlan& out) {
  const int64_t half = (q - 1) / 2;
  KeyPlan kp;
  kp.key_class.assign(entries, KC_GENERAL);
  kp.key_entry.assign(entries, -1);
  for (size_t e = 0; e < entries; ++e) {
    const int64_t* p = a + e * N;
    bool tail_zero = true;
    long double ssq = 0.0L;
    for (uint32_t j = 0; j < N; ++j) {
      const int64_t v = p[j];
      if (v > half || v < -half) return kPlanArg;
      if (j > 0 && v != 0) tail_zero = false;
      ssq += (long double)v * (long double)v;
    }
    if (tail_zero && p[0] == 0)
      kp.key_class[e] = KC_ZERO;
    else if (tail_zero && p[0] == 1)
      kp.key_class[e] = KC_ONE;
    else {
      kp.key_entry[e] = (int32_t)kp.n_general++;
      kp.general.insert(kp.general.end(), p, p + N);
      kp.kinf.push_back((double)(std::sqrt(ssq) * (1.0L + 1e-6L)));
    }
  }
  out = std::move(kp);
  return kPlanOk;
}

// What a load does to the tables a context keeps (rzk_ctx: key_class, key_entry, n_general): plan_key, and only when it
// accepts the key the new tables take their place (kp keeps the general entries and their bounds for the device steps).
// A refused key leaves all three, and kp, as they were.
inline int plan_key_tables(const int64_t* a, size_t entries, uint32_t N, int64_t q, std::vector<uint8_t>& key_class,
                           std::vector<int32_t>& key_entry, uint32_t& n_general, KeyPlan& kp) {
  const int rc = plan_key(a, entries, N, q, kp);
  if (rc != kPlanOk) return rc;
  key_class.swap(kp.key_class);
  key_entry.swap(kp.key_entry);
  n_general = kp.n_general;
  return kPlanOk;
}

}  // namespace rzk
