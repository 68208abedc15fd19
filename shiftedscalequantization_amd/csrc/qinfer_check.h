// Host-side argument checks shared by the integer-inference entry points (qinfer*.hip).
#pragma once
#include <cmath>

#include "ssq_common.h"

namespace ssq {

// A packed weight's code range: n_bits in [1, 8], qmin 0 (asymmetric) or -2^(n_bits-1).
static inline int qrange_ok(const char* what, int n_bits, int qmin) {
  SSQ_REQUIRE(n_bits >= 1 && n_bits <= 8, SSQ_E_ARG, "%s: n_bits %d not in [1, 8]", what, n_bits);
  SSQ_REQUIRE(qmin == 0 || qmin == -(1 << (n_bits - 1)), SSQ_E_ARG,
              "%s: qmin %d is neither 0 nor -2^(n_bits-1)", what, qmin);
  return SSQ_OK;
}

// An act quantizer whose codes are stored as int8 q - (qmin + 128): the code range fits 8 bits,
// delta (where the caller has one; else null) is positive and finite, and the zero point is an
// integer in [qmin, qmin + 255] (a padded tap stores zero_point - (qmin + 128) as an int8).
// `role` names the quantizer in the message: "", "activation ", "output " or "residual ".
static inline int qquant_ok(const char* what, const char* role, const float* delta,
                            float zero_point, int qmin, int qmax) {
  SSQ_REQUIRE(qmin < qmax && qmax - qmin <= 255, SSQ_E_ARG,
              "%s: %scode range [%d, %d] does not fit 8-bit codes", what, role, qmin, qmax);
  SSQ_REQUIRE(!delta || (*delta > 0.0f && *delta <= 3.0e38f), SSQ_E_ARG,
              "%s: %sdelta must be positive and finite", what, role);
  SSQ_REQUIRE(zero_point == rintf(zero_point) && zero_point >= (float)qmin &&
                  zero_point <= (float)(qmin + 255),
              SSQ_E_ARG, "%s: %szero point %g is not an integer in [%d, %d]", what, role,
              (double)zero_point, qmin, qmin + 255);
  return SSQ_OK;
}

}  // namespace ssq
