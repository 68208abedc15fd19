// The prepared-weight layouts of the integer route.
//
// QLayout, K22's blob, shared by its readers (K23 in qinfer.hip, K30 in qinfer_head.hip):
// [Cop = 64*ceil(Co/64)][Kp = 64*ceil(R*S*Cp/64)] int8 rows, k = (r*S + s)*Cp + ci with
// Cp = 16*ceil(Ci/16), then the 0/1 row [Kp], then cwz[Cop] and T[Cop] (int32).
//
// The wide blob (qlayout(..., 2), ssq_qweight_prepare_wide; read by K23's WIDE instantiations
// only): a centred operand m = 128 h + l in two int8 digit planes of the rows above, first h
// in [-127, 127], then l in [-64, 63], at a distance of Cop * Kp bytes; then the 0/1 row [Kp] (written,
// not read), cwz[Cop] = 0 and T[Cop] = sum m (int32).
//
// GLayout, K24's blob (qinfer_grouped.hip), by kind.  Depthwise (K25): int32 [R*S][Cp].
// Grouped (K26): int8 [G*Cogp][Kp], Kp = 64*ceil(R*S*Wc/64), k = tap * Wc + (c - w0_g) inside
// group g's 16-aligned channel window; then the 0/1 rows [G][Kp]; then cwz[Co], T[Co] (int32).
//
// The wide grouped blob (glayout(..., 2), ssq_qweight_prepare_grouped_wide; read by K26's WIDE
// instantiations only): the grouped rows above as two int8 digit planes of m = 128 h + l, first h,
// then l at a distance of G * Cogp * Kp bytes; then the 0/1 rows [G][Kp] (written, not read),
// cwz[Co] = 0 and T[Co] = sum m (int32).  The depthwise blob has one form: int32 holds m as it is.
//
// SLayout, K31's blob (qinfer_stemconv.hip): the fp32 weight in the order the 16x16x4 fp32 MFMA
// takes its A operand, float [Kp / 4][Cop / 16][4][16] with Kp = 4*ceil(K/4), K = Ci*R*S,
// k = (ci*R + r)*S + s (the weight's own memory order) and Cop = 16*ceil(Co/16): entry
// [t][c][kk][j] is W[co = 16 c + j][k = 4 t + kk], so lane l of a wave reads word l of the 64
// of (step t, chunk c).  A padded channel is +0; a padded k is -0 in every channel (the pixel
// operand there is +0, the product -0, and acc + (-0) is acc for every acc, a signed zero too).
#pragma once
#include <cstddef>
#include <cstdint>

namespace ssq {

constexpr int64_t kStemMaxCi = 4, kStemMaxRS = 7;

struct SLayout {
  int64_t K, Kp, Cop;
  size_t bytes;   // 0: outside K31's geometry
};

static inline SLayout slayout(int64_t Co, int64_t Ci, int64_t R, int64_t S) {
  SLayout L = {};
  if (Co < 1 || Co >= (1ll << 24) || Ci < 1 || Ci > kStemMaxCi || R < 1 || R > kStemMaxRS ||
      S < 1 || S > kStemMaxRS)
    return L;
  L.K = Ci * R * S;
  L.Kp = (L.K + 3) / 4 * 4;
  L.Cop = (Co + 15) / 16 * 16;
  L.bytes = (size_t)L.Kp * (size_t)L.Cop * 4;
  return L;
}

// ULayout, K32's blob (qinfer_stemu8.hip): per input channel c the int8 rows w_s = q - (qmin + 128)
// as [Ci][Cop][64], k = r*S + s (R*S <= 49 taps, zero from R*S on, a padded channel all zero), the
// order the 16x16x64 int8 MFMA takes its A operand (row = channel, 16 k per lane); then
// cwz[Cop] = qmin + 128 - z_w[co] and T[Ci][Cop] = sum over every tap of (q - z_w[co]) (int32).
struct ULayout {
  int64_t RS, Cop;
  size_t off_cwz, off_t, bytes;   // bytes 0: outside K32's geometry (K31's)
};

static inline ULayout ulayout(int64_t Co, int64_t Ci, int64_t R, int64_t S) {
  ULayout L = {};
  if (!slayout(Co, Ci, R, S).bytes) return L;
  L.RS = R * S;
  L.Cop = (Co + 15) / 16 * 16;
  L.off_cwz = (size_t)(Ci * L.Cop) * 64;
  L.off_t = L.off_cwz + (size_t)L.Cop * 4;
  L.bytes = L.off_t + (size_t)(Ci * L.Cop) * 4;
  return L;
}

constexpr int kQT = 64;     // pixels, channels and k per tile step
constexpr int kQRow = 80;   // LDS row stride in bytes (64 + 16)
constexpr int64_t kQMaxK = 65536;

static inline int64_t rup(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

struct QLayout {
  int64_t Cp, Kp, Cop;
  size_t off_mask, off_cwz, off_t, bytes;
};

constexpr int kQWideMax = 16319;   // |m| of the wide operand: 128 * 127 + 63

// planes: 1, K22's blob; 2, the wide blob
static inline QLayout qlayout(int64_t Co, int64_t Ci, int64_t R, int64_t S, int planes = 1) {
  QLayout L;
  L.Cp = rup(Ci, 16);
  L.Kp = rup(R * S * L.Cp, kQT);
  L.Cop = rup(Co, kQT);
  L.off_mask = (size_t)planes * (size_t)L.Cop * (size_t)L.Kp;
  L.off_cwz = L.off_mask + (size_t)L.Kp;
  L.off_t = L.off_cwz + (size_t)L.Cop * 4;
  L.bytes = L.off_t + (size_t)L.Cop * 4;
  return L;
}

constexpr int kGT = 64;      // K26: pixels, channel rows (at most) and k per tile step
constexpr int64_t kGMaxK = 65536;

// 0 invalid, 1 depthwise direct, 2 grouped MFMA
static inline int qg_kind(int64_t Co, int64_t Cig, int64_t groups) {
  if (groups < 2 || Co < 1 || Cig < 1 || Co % groups != 0) return 0;
  return (Cig == 1 && Co == groups) ? 1 : 2;
}

struct GLayout {
  int kind;
  int64_t C, Cp, Cog, Cogp, Wc, Kp, tiles;   // tiles: channel tiles per group
  size_t off_mask, off_cwz, off_t, bytes;
};

// planes: 1, K24's blob; 2, the wide grouped blob (the depthwise blob is the same for both)
static inline GLayout glayout(int64_t Co, int64_t Cig, int64_t R, int64_t S, int64_t groups,
                              int planes = 1) {
  GLayout L = {};
  L.kind = qg_kind(Co, Cig, groups);
  if (!L.kind || R < 1 || S < 1) {
    L.kind = 0;
    return L;
  }
  L.C = Cig * groups;
  L.Cp = rup(L.C, 16);
  L.Cog = Co / groups;
  if (L.kind == 1) {
    L.bytes = (size_t)(R * S) * (size_t)L.Cp * 4;
    return L;
  }
  L.Cogp = rup(L.Cog, 16);
  L.tiles = (L.Cogp + kGT - 1) / kGT;
  // the window width repeats with period 16 / gcd(Cig, 16) <= 16 groups
  for (int64_t g = 0; g < groups && g < 16; ++g) {
    const int64_t w = rup((g + 1) * Cig, 16) - g * Cig / 16 * 16;
    if (w > L.Wc) L.Wc = w;
  }
  L.Kp = rup(R * S * L.Wc, kGT);
  L.off_mask = (size_t)planes * (size_t)(groups * L.Cogp) * (size_t)L.Kp;
  L.off_cwz = L.off_mask + (size_t)groups * (size_t)L.Kp;
  L.off_t = L.off_cwz + (size_t)Co * 4;
  L.bytes = L.off_t + (size_t)Co * 4;
  return L;
}

}  // namespace ssq
