// K22's prepared-weight layout, shared by its readers (K23 in qinfer.hip, K30 in
// qinfer_head.hip): [Cop = 64*ceil(Co/64)][Kp = 64*ceil(R*S*Cp/64)] int8 rows,
// k = (r*S + s)*Cp + ci with Cp = 16*ceil(Ci/16), then the 0/1 row [Kp], then cwz[Cop] and
// T[Cop] (int32).
#pragma once
#include <cstddef>
#include <cstdint>

namespace ssq {

constexpr int kQT = 64;     // pixels, channels and k per tile step
constexpr int kQRow = 80;   // LDS row stride in bytes (64 + 16)
constexpr int64_t kQMaxK = 65536;

static inline int64_t rup(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

struct QLayout {
  int64_t Cp, Kp, Cop;
  size_t off_mask, off_cwz, off_t, bytes;
};

static inline QLayout qlayout(int64_t Co, int64_t Ci, int64_t R, int64_t S) {
  QLayout L;
  L.Cp = rup(Ci, 16);
  L.Kp = rup(R * S * L.Cp, kQT);
  L.Cop = rup(Co, kQT);
  L.off_mask = (size_t)L.Cop * (size_t)L.Kp;
  L.off_cwz = L.off_mask + (size_t)L.Kp;
  L.off_t = L.off_cwz + (size_t)L.Cop * 4;
  L.bytes = L.off_t + (size_t)L.Cop * 4;
  return L;
}

}  // namespace ssq
