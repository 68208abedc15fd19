// The element rules of the weight-prepare kernels (K22 in qinfer.hip, K24 in qinfer_grouped.hip).
#pragma once
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

// A column-scaled weight W_hat = ((q - z_w[co]) * d1[co]) * (kcol[j] / L): the operand is the
// centred integer m = (q - z_w[co]) * kcol[j].  nbad counts a kcol[j] outside [1, 127] (taken
// as 0) and an m outside [-127, 127] (stored saturated).
__device__ __forceinline__ int colscaled(int centred, int kj, uint32_t& nbad) {
  if (kj < 1 || kj > 127) {
    ++nbad;
    kj = 0;
  }
  int v = centred * kj;   // |q - z| <= 767, kj <= 127: no overflow
  if (v > 127 || v < -127) {
    ++nbad;
    v = v > 0 ? 127 : -127;
  }
  return v;
}

}  // namespace ssq
