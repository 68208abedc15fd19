// The element rules of the weight-prepare kernels (K22 in qinfer.hip, K24 in qinfer_grouped.hip).
#pragma once
#include "qinfer_layout.h"
#include "ssq_common.h"

namespace ssq {

// storage bits per code of the packed export: 2, 4 or 8
static inline int packed_bits(int n_bits) { return n_bits <= 2 ? 2 : (n_bits <= 4 ? 4 : 8); }

// code idx of the packed export, u = q - qmin
__device__ __forceinline__ uint32_t packed_code(const uint8_t* packed, size_t idx, int bs) {
  const size_t bit = idx * (size_t)bs;
  return ((uint32_t)packed[bit >> 3] >> (bit & 7)) & ((1u << bs) - 1u);
}

// The zero-point rule: any integer near the code range (|cw - z| <= 384 keeps K * cwz inside
// int32), else counted once per channel and taken as qmin.
__device__ __forceinline__ bool zp_is_code(float z, int qmin) {
  return z == rintf(z) && z >= (float)(qmin - 256) && z <= (float)(qmin + 511);
}

// A scaled weight W_hat = ((q - z_w[co]) * d[co]) * (k / L): the operand is the centred integer
// m = (q - z_w[co]) * k.  Where k lies is stated once: element (co, ci, tap) reads
// k[co * s_co + ci * s_ci + tap * s_tap] -- a column scale (ChannelQuantMSE) is (0, RS, 1), a
// per-(co, ci) scale (ChannelQuant's shifted scale) (Ci, 1, 0), Cig for a grouped conv.  `lim`: the
// largest k and |m| the operand holds, 127 (int8) or kQWideMax (two int8 digits).
struct QFactor {
  const int32_t* k;
  uint32_t s_co, s_ci, s_tap;
  int lim;
};

static inline QFactor qfactor(const int32_t* k, bool per_ci, uint32_t Ci, uint32_t RS, int lim) {
  return per_ci ? QFactor{k, Ci, 1u, 0u, lim} : QFactor{k, 0u, RS, 1u, lim};
}

__device__ __forceinline__ int qfactor_at(const QFactor& f, uint32_t co, uint32_t ci, uint32_t tap) {
  return f.k[(size_t)co * f.s_co + (size_t)ci * f.s_ci + (size_t)tap * f.s_tap];
}

// nbad counts a k outside [1, lim] (taken as 0) and an m outside [-lim, lim] (stored saturated).
__device__ __forceinline__ int qscaled(int centred, int kj, int lim, uint32_t& nbad) {
  if (kj < 1 || kj > lim) {
    ++nbad;
    kj = 0;
  }
  int v = centred * kj;   // |q - z| <= 767, kj <= 16319: no overflow
  if (v > lim || v < -lim) {
    ++nbad;
    v = v > 0 ? lim : -lim;
  }
  return v;
}

// The wide operand's digits: m = 128 h + l, l = ((m + 64) mod 128) - 64 in [-64, 63] (floor mod),
// h = (m - l) / 128 in [-127, 127] for |m| <= kQWideMax.
__device__ __forceinline__ int qdigit_lo(int m) { return ((m + 64) & 127) - 64; }
__device__ __forceinline__ int qdigit_hi(int m) { return (m - qdigit_lo(m)) >> 7; }

}  // namespace ssq
