// K33's device functions and host checks (actshift.hip says what they compute), shared with the
// kernels that run the shifted-scale act quantizer inside another pass (actshift_epi.hip, K34).
// The K33 kernels themselves, and the finish kernels behind act_finish_launch, live in
// actshift.hip.
#pragma once

#include "ssq_common.h"
#include "qinfer_epi.h"   // SSQ_NO_PK_F32

namespace ssq {

constexpr int kActMaxS = 4;
constexpr int kActU = 4;                 // loads in flight per thread and step

enum ActOp { kFwdSoft = 0, kFwdHard = 1, kBwdSoft = 2, kBwdHard = 3, kInit = 4,
             kBwdSoftD = 5, kBwdHardD = 6 };   // the backwards with ddelta

struct ActShifts {
  float s[kActMaxS];
};

template <int S>
struct ActGrid {
  float d[S], r[S], p[S];
  float z, hi;
  int k;
  bool fast;
  double ps[S];   // ddelta forms only: p[c,i] * s_i (exact in double); hard: s_i
};

// the per-tensor part of the grid: d_i = fp32(delta * s_i), its reciprocal, z and qmax
template <int S>
__device__ __forceinline__ void act_grid_scales(ActGrid<S>& G, const float* __restrict__ delta,
                                                const float* __restrict__ zp, const ActShifts& sh,
                                                float hi) {
  G.z = zp[0];
  G.hi = hi;
  G.fast = true;
  const float d0 = delta[0];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    G.d[i] = __fmul_rn(d0, sh.s[i]);
    G.r[i] = recip_for_div(G.d[i]);
    G.fast = G.fast && G.r[i] != 0.0f;
  }
}

// channel c's part: its p row and k, the first index of the row's maximum (torch.argmax's tie
// rule) as an unrolled compare chain -- no runtime index into G.p, so the grid stays in
// registers.  DELTA: ps too (HARD: s_i alone).
template <int S, bool DELTA, bool HARD>
__device__ __forceinline__ void act_grid_channel(ActGrid<S>& G, const float* __restrict__ p,
                                                 uint32_t c, const ActShifts& sh) {
#pragma unroll
  for (int i = 0; i < S; ++i) {
    G.p[i] = p[(size_t)c * S + i];
    if (DELTA)
      G.ps[i] = HARD ? (double)sh.s[i] : (double)G.p[i] * (double)sh.s[i];   // 48 bits: exact
  }
  float best = G.p[0];
  G.k = 0;
#pragma unroll
  for (int i = 1; i < S; ++i) {
    const bool gt = G.p[i] > best;
    best = gt ? G.p[i] : best;
    G.k = gt ? i : G.k;
  }
}

// t_i of the ddelta rule, in double from the forward's fp32 c_i and in_i
__device__ __forceinline__ double act_dterm(double xd, float c, float in, float z, float d) {
  return ((double)c - (double)z) - (double)in * (xd / (double)d);
}

template <int S, int OP, bool FAST>
__device__ __forceinline__ float act_elem(float x, float gv, const ActGrid<S>& G, double* acc) {
  float Q[S], in[S], cl[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const float t = FAST ? div_fast(x, G.d[i], G.r[i]) : x / G.d[i];
    const float v = __fadd_rn(rintf(t), G.z);
    in[i] = (v >= 0.0f && v <= G.hi) ? 1.0f : 0.0f;
    cl[i] = clampf(v, 0.0f, G.hi);
    Q[i] = __fmul_rn(__fsub_rn(cl[i], G.z), G.d[i]);
  }
  if (OP == kFwdSoft) {
    float y = __fmul_rn(Q[0], G.p[0]);
#pragma unroll
    for (int i = 1; i < S; ++i) y = __fadd_rn(y, __fmul_rn(Q[i], G.p[i]));
    return y;
  } else if (OP == kFwdHard) {
    float y = Q[0];
#pragma unroll
    for (int i = 1; i < S; ++i) y = i == G.k ? Q[i] : y;
    return y;
  } else if (OP == kBwdSoft) {
    float m = 0.0f;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      m = __fadd_rn(m, __fmul_rn(G.p[i], in[i]));
      acc[i] = fma((double)gv, (double)Q[i], acc[i]);   // the product is exact in double
    }
    return __fmul_rn(gv, m);
  } else if (OP == kBwdHard) {
    float mk = in[0];
#pragma unroll
    for (int i = 1; i < S; ++i) mk = i == G.k ? in[i] : mk;
    return __fmul_rn(gv, mk);
  } else if (OP == kBwdSoftD) {
    // kBwdSoft's dx and dp, operation for operation; acc[S] is the ddelta sum
    const double xd = (double)x, gd = (double)gv;
    float m = 0.0f;
    double e = 0.0;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      m = __fadd_rn(m, __fmul_rn(G.p[i], in[i]));
      acc[i] = fma(gd, (double)Q[i], acc[i]);
      e = fma(G.ps[i], act_dterm(xd, cl[i], in[i], G.z, G.d[i]), e);
    }
    acc[S] = fma(gd, e, acc[S]);
    return __fmul_rn(gv, m);
  } else if (OP == kBwdHardD) {
    // kBwdHard's dx; acc[0] is the ddelta sum over the chosen candidate
    float mk = in[0], ck = cl[0], dk = G.d[0];
    double sk = G.ps[0];
#pragma unroll
    for (int i = 1; i < S; ++i) {
      const bool sel = i == G.k;
      mk = sel ? in[i] : mk;
      ck = sel ? cl[i] : ck;
      dk = sel ? G.d[i] : dk;
      sk = sel ? G.ps[i] : sk;
    }
    acc[0] = fma((double)gv, sk * act_dterm((double)x, ck, mk, G.z, dk), acc[0]);
    return __fmul_rn(gv, mk);
  } else {
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const double r = (double)x - (double)Q[i];
      acc[i] = fma(r, r, acc[i]);
    }
    return 0.0f;
  }
}

// ---------------------------------------------------------------- host side
// The launch geometry of a plane walk: a wave per plane while a plane is at most kBlock work
// items (float4s or elements), the workgroup otherwise; at most 8 workgroups per CU.  Every
// kernel whose dp / ddelta partials K33's finish kernels sum takes this geometry.
struct ActGeometry {
  bool wave;
  uint32_t blocks;
};
inline ActGeometry act_geometry(bool vec, uint32_t planes, uint32_t hw) {
  const uint32_t items = vec ? hw / 4 : hw;
  constexpr uint32_t kMaxBlocks = 256 * 8;
  constexpr uint32_t GPB = kBlock / kWave;
  const bool wave = items <= (uint32_t)kBlock;
  const uint32_t blocks = wave ? (planes + GPB - 1) / GPB : planes;
  return ActGeometry{wave, blocks > kMaxBlocks ? kMaxBlocks : blocks};
}

inline bool act_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Shared argument checks; fills sh.  planes = N * C.
inline int act_check(const char* what, const float* shifts, int S, int64_t N, int64_t C,
                     int64_t HW, int qmax, ActShifts& sh) {
  SSQ_REQUIRE(S >= 1 && S <= kActMaxS, SSQ_E_ARG, "%s: S = %d shift targets (1..%d supported)",
              what, S, kActMaxS);
  SSQ_REQUIRE(N >= 0 && C >= 1 && C < (1ll << 28) && HW >= 1, SSQ_E_ARG, "%s: bad sizes", what);
  SSQ_REQUIRE(N < (1ll << 31) && C < (1ll << 31) && HW < (1ll << 31) &&
                  (N == 0 || (C * HW) < (1ll << 31) / N),
              SSQ_E_ARG, "%s: N*C*H*W must stay below 2^31", what);
  SSQ_REQUIRE(qmax >= 1, SSQ_E_ARG, "%s: qmax < 1", what);
  SSQ_REQUIRE(shifts != nullptr, SSQ_E_ARG, "%s: null pointer (shifts)", what);
  for (int i = 0; i < kActMaxS; ++i) sh.s[i] = i < S ? shifts[i] : 1.0f;
  return SSQ_OK;
}

inline size_t act_part_bytes(int64_t N, int64_t C, int S) {
  if (N <= 0 || C <= 0 || S <= 0 || S > kActMaxS || N >= (1ll << 31) || C >= (1ll << 31) ||
      C >= (1ll << 31) / N)
    return 0;
  return (size_t)N * (size_t)C * (size_t)S * sizeof(double);
}

// The backward's finish (actshift.hip): dp[c, i] from the N*C plane partials at part (zeros when
// hard; dp may be NULL then), and, when ddelta is given, ddelta from the N*C partials behind
// them -- one launch either way, none when there is nothing to write.
void act_finish_launch(hipStream_t s, const double* part, int64_t N, int64_t C, int S, bool hard,
                       float* dp, float* ddelta);

}  // namespace ssq
