// K33: shifted-scale activations -- ChannelQuantAct 'shiftFeature' (DESIGN.md section 6).
//
// x is (N, C, H*W) in NCHW order.  Every candidate is the 'none'-mode q/dq of the replaced
// per-tensor quantizer at the scale s_i (fq1<false, false> with d_i = fp32(delta * s_i)):
//   v_i = rint(x / d_i) + z;  Q_i = (clamp(v_i, 0, qmax) - z) * d_i;  in_i = [0 <= v_i <= qmax]
// forward   soft: y = Q_0*p[c,0]; y += Q_i*p[c,i]  (each product and sum rounded, no fma)
//           hard: y = Q_k, k = first argmax of p[c,:]
// backward  soft: dx = g * m, m = (+0 + p[c,0]*in_0) + ... ; dp[c,i] = sum_{n,hw} g*Q_i
//           hard: dx = g * in_k; dp = 0
// init      mse[c,i] = sum_{n,hw} (x - Q_i)^2
//
// Bandwidth kernels: 8 B/elem forward, 12 B/elem backward, 4 B/elem init.  A group of
// TPP threads (a wave for short planes, the workgroup otherwise) owns whole (n, c) planes,
// so the channel's p row and its S grids sit in scalar registers; each thread issues U
// loads (float4 when H*W % 4 == 0 and the bases are 16-B aligned, else scalar) before any
// math.  x / d_i takes the reciprocal form (div_fast, bit-identical) when the whole wave's
// step is in its range, one wave-uniform branch per step.  The channel sums are exact
// products accumulated in double, reduced in a fixed order inside the group, stored per
// plane in the workspace and summed over n in ascending order by a finish kernel: no
// atomics, the same bits on every run.
#include "ssq_common.h"

namespace ssq {

constexpr int kActMaxS = 4;
constexpr int kActU = 4;                 // loads in flight per thread and step

enum ActOp { kFwdSoft = 0, kFwdHard = 1, kBwdSoft = 2, kBwdHard = 3, kInit = 4 };

struct ActShifts {
  float s[kActMaxS];
};

template <int S>
struct ActGrid {
  float d[S], r[S], p[S];
  float z, hi;
  int k;
  bool fast;
};

template <int S, int OP, bool FAST>
__device__ __forceinline__ float act_elem(float x, float gv, const ActGrid<S>& G, double* acc) {
  float Q[S], in[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const float t = FAST ? div_fast(x, G.d[i], G.r[i]) : x / G.d[i];
    const float v = __fadd_rn(rintf(t), G.z);
    in[i] = (v >= 0.0f && v <= G.hi) ? 1.0f : 0.0f;
    Q[i] = __fmul_rn(__fsub_rn(clampf(v, 0.0f, G.hi), G.z), G.d[i]);
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
  } else {
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const double r = (double)x - (double)Q[i];
      acc[i] = fma(r, r, acc[i]);
    }
    return 0.0f;
  }
}

template <int OP>
constexpr bool act_has_g() { return OP == kBwdSoft || OP == kBwdHard; }
template <int OP>
constexpr bool act_has_out() { return OP != kInit; }
template <int OP>
constexpr bool act_has_acc() { return OP == kBwdSoft || OP == kInit; }

// One plane of `hw` elements at x/g/out, walked by the TPP threads of the group.
template <int S, int OP, bool VEC, int TPP>
__device__ __forceinline__ void act_plane(const float* __restrict__ x, const float* __restrict__ g,
                                          float* __restrict__ out, uint32_t hw,
                                          const ActGrid<S>& G, uint32_t lane, double* acc) {
  if (VEC) {
    const uint32_t n4 = hw >> 2;
    const f32x4* xv = (const f32x4*)x;
    const f32x4* gv = (const f32x4*)g;
    f32x4* ov = (f32x4*)out;
    for (uint32_t base = 0; base < n4; base += kActU * TPP) {
      f32x4 vx[kActU], vg[kActU];
      unsigned ok = G.fast;
#pragma unroll
      for (int u = 0; u < kActU; ++u) {
        const uint32_t j = base + u * TPP + lane;
        const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
        vx[u] = j < n4 ? xv[j] : zero;
        if (act_has_g<OP>()) vg[u] = j < n4 ? gv[j] : zero;
        ok &= (unsigned)div_fast_ok(vx[u].x) & (unsigned)div_fast_ok(vx[u].y) &
              (unsigned)div_fast_ok(vx[u].z) & (unsigned)div_fast_ok(vx[u].w);
      }
      const bool fast = __all(ok);
#pragma unroll
      for (int u = 0; u < kActU; ++u) {
        const uint32_t j = base + u * TPP + lane;
        if (j < n4) {
          const float xe[4] = {vx[u].x, vx[u].y, vx[u].z, vx[u].w};
          float ge[4] = {0.0f, 0.0f, 0.0f, 0.0f}, oe[4];
          if (act_has_g<OP>()) {
            ge[0] = vg[u].x;
            ge[1] = vg[u].y;
            ge[2] = vg[u].z;
            ge[3] = vg[u].w;
          }
          if (fast) {
#pragma unroll
            for (int e = 0; e < 4; ++e) oe[e] = act_elem<S, OP, true>(xe[e], ge[e], G, acc);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) oe[e] = act_elem<S, OP, false>(xe[e], ge[e], G, acc);
          }
          if (act_has_out<OP>()) {
            f32x4 o;
            o.x = oe[0];
            o.y = oe[1];
            o.z = oe[2];
            o.w = oe[3];
            ov[j] = o;
          }
        }
      }
    }
  } else {
    for (uint32_t base = 0; base < hw; base += kActU * TPP) {
      float vx[kActU], vg[kActU];
      unsigned ok = G.fast;
#pragma unroll
      for (int u = 0; u < kActU; ++u) {
        const uint32_t j = base + u * TPP + lane;
        vx[u] = j < hw ? x[j] : 0.0f;
        vg[u] = (act_has_g<OP>() && j < hw) ? g[j] : 0.0f;
        ok &= (unsigned)div_fast_ok(vx[u]);
      }
      const bool fast = __all(ok);
#pragma unroll
      for (int u = 0; u < kActU; ++u) {
        const uint32_t j = base + u * TPP + lane;
        if (j < hw) {
          const float o = fast ? act_elem<S, OP, true>(vx[u], vg[u], G, acc)
                               : act_elem<S, OP, false>(vx[u], vg[u], G, acc);
          if (act_has_out<OP>()) out[j] = o;
        }
      }
    }
  }
}

// Groups of TPP threads walk the planes group, group + ngroups, ...; plane pl is channel
// pl % C.  part: (planes, S) doubles, the per-plane channel sums (kBwdSoft / kInit).
template <int S, int OP, bool VEC, int TPP>
__global__ __launch_bounds__(kBlock) void act_kernel(const float* __restrict__ x,
                                                     const float* __restrict__ g,
                                                     float* __restrict__ out,
                                                     const float* __restrict__ p,
                                                     const float* __restrict__ delta,
                                                     const float* __restrict__ zp, ActShifts sh,
                                                     float hi, uint32_t planes, uint32_t C,
                                                     uint32_t hw, double* __restrict__ part) {
  __shared__ double red[16];
  constexpr uint32_t GPB = kBlock / TPP;
  const uint32_t lane = threadIdx.x % TPP;
  const uint32_t ngroups = gridDim.x * GPB;
  ActGrid<S> G;
  G.z = zp[0];
  G.hi = hi;
  G.fast = true;
  const float d0 = delta[0];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    G.d[i] = __fmul_rn(d0, sh.s[i]);
    G.r[i] = recip_for_div(G.d[i]);
    G.fast = G.fast && G.r[i] != 0.0f;
    G.p[i] = 0.0f;
  }
  G.k = 0;
  // (TPP == kBlock: one group per workgroup, so the trip count -- and every barrier of
  // block_sum below -- is uniform over the workgroup)
  for (uint32_t pl = blockIdx.x * GPB + threadIdx.x / TPP; pl < planes; pl += ngroups) {
    const uint32_t c = pl % C;
    if (OP != kInit) {
#pragma unroll
      for (int i = 0; i < S; ++i) G.p[i] = p[(size_t)c * S + i];
      // first index of the maximum (torch.argmax's tie rule), as an unrolled compare chain:
      // no runtime index into G.p, so the grid stays in registers
      float best = G.p[0];
      G.k = 0;
#pragma unroll
      for (int i = 1; i < S; ++i) {
        const bool gt = G.p[i] > best;
        best = gt ? G.p[i] : best;
        G.k = gt ? i : G.k;
      }
    }
    double acc[S];
#pragma unroll
    for (int i = 0; i < S; ++i) acc[i] = 0.0;
    const size_t off = (size_t)pl * hw;
    act_plane<S, OP, VEC, TPP>(x + off, act_has_g<OP>() ? g + off : nullptr,
                               act_has_out<OP>() ? out + off : nullptr, hw, G, lane, acc);
    if (act_has_acc<OP>()) {
#pragma unroll
      for (int i = 0; i < S; ++i) {
        double t;
        if constexpr (TPP == kWave) t = wave_sum(acc[i]);
        else t = block_sum(acc[i], red);
        if (lane == 0) part[(size_t)pl * S + i] = t;
      }
    }
  }
}

// out[c, i] = sum over n (ascending) of part[(n*C + c), i]; zero == 1 writes zeros (the
// hard backward's dp).
__global__ __launch_bounds__(kBlock) void act_finish(const double* __restrict__ part, uint32_t N,
                                                     uint32_t C, int S, int zero,
                                                     float* __restrict__ out) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= C * (uint32_t)S) return;
  double t = 0.0;
  if (!zero)
    for (uint32_t n = 0; n < N; ++n) t += part[(size_t)n * C * S + e];
  out[e] = (float)t;
}

static bool act_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <int S, int OP, bool VEC>
static void act_launch_tpp(hipStream_t s, const float* x, const float* g, float* out,
                           const float* p, const float* delta, const float* zp,
                           const ActShifts& sh, float hi, uint32_t planes, uint32_t C, uint32_t hw,
                           double* part) {
  const uint32_t items = VEC ? hw / 4 : hw;
  constexpr uint32_t kMaxBlocks = 256 * 8;   // 8 workgroups per CU
  if (items <= (uint32_t)kBlock) {
    constexpr uint32_t GPB = kBlock / kWave;
    uint32_t blocks = (planes + GPB - 1) / GPB;
    blocks = blocks > kMaxBlocks ? kMaxBlocks : blocks;
    hipLaunchKernelGGL((act_kernel<S, OP, VEC, kWave>), dim3(blocks), dim3(kBlock), 0, s, x, g, out,
                       p, delta, zp, sh, hi, planes, C, hw, part);
  } else {
    const uint32_t blocks = planes > kMaxBlocks ? kMaxBlocks : planes;
    hipLaunchKernelGGL((act_kernel<S, OP, VEC, kBlock>), dim3(blocks), dim3(kBlock), 0, s, x, g,
                       out, p, delta, zp, sh, hi, planes, C, hw, part);
  }
}

template <int OP>
static void act_launch(hipStream_t s, int S, bool vec, const float* x, const float* g, float* out,
                       const float* p, const float* delta, const float* zp, const ActShifts& sh,
                       float hi, uint32_t planes, uint32_t C, uint32_t hw, double* part) {
#define SSQ_ACT_CASE(SV)                                                                        \
  case SV:                                                                                      \
    if (vec)                                                                                    \
      act_launch_tpp<SV, OP, true>(s, x, g, out, p, delta, zp, sh, hi, planes, C, hw, part);    \
    else                                                                                        \
      act_launch_tpp<SV, OP, false>(s, x, g, out, p, delta, zp, sh, hi, planes, C, hw, part);   \
    break;
  switch (S) {
    SSQ_ACT_CASE(1)
    SSQ_ACT_CASE(2)
    SSQ_ACT_CASE(3)
    SSQ_ACT_CASE(4)
  }
#undef SSQ_ACT_CASE
}

// Shared argument checks; fills sh.  planes = N * C.
static int act_check(const char* what, const float* shifts, int S, int64_t N, int64_t C,
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

static size_t act_part_bytes(int64_t N, int64_t C, int S) {
  if (N <= 0 || C <= 0 || S <= 0 || S > kActMaxS || N >= (1ll << 31) || C >= (1ll << 31) ||
      C >= (1ll << 31) / N)
    return 0;
  return (size_t)N * (size_t)C * (size_t)S * sizeof(double);
}

}  // namespace ssq

using namespace ssq;

extern "C" size_t ssq_actshift_fwd_workspace_size(int64_t N, int64_t C, int64_t HW, int S) {
  (void)N;
  (void)C;
  (void)HW;
  (void)S;
  return 0;
}

extern "C" int ssq_actshift_fwd(const float* x, const float* p, const float* delta,
                                const float* zp, const float* shifts, int S, int64_t N, int64_t C,
                                int64_t HW, int qmax, int hard, float* y, void* ws,
                                size_t ws_bytes, ssq_stream_t stream) {
  (void)ws;
  (void)ws_bytes;
  const char* what = "ssq_actshift_fwd";
  ActShifts sh;
  if (int rc = act_check(what, shifts, S, N, C, HW, qmax, sh)) return rc;
  if (N == 0) return SSQ_OK;
  SSQ_REQUIRE(x && p && delta && zp && y, SSQ_E_ARG, "%s: null pointer", what);
  const bool vec = HW % 4 == 0 && act_aligned16(x) && act_aligned16(y);
  hipStream_t s = (hipStream_t)stream;
  if (hard)
    act_launch<kFwdHard>(s, S, vec, x, nullptr, y, p, delta, zp, sh, (float)qmax,
                         (uint32_t)(N * C), (uint32_t)C, (uint32_t)HW, nullptr);
  else
    act_launch<kFwdSoft>(s, S, vec, x, nullptr, y, p, delta, zp, sh, (float)qmax,
                         (uint32_t)(N * C), (uint32_t)C, (uint32_t)HW, nullptr);
  return check_launch(what);
}

extern "C" size_t ssq_actshift_bwd_workspace_size(int64_t N, int64_t C, int64_t HW, int S) {
  (void)HW;
  return act_part_bytes(N, C, S);
}

extern "C" int ssq_actshift_bwd(const float* x, const float* g, const float* p,
                                const float* delta, const float* zp, const float* shifts, int S,
                                int64_t N, int64_t C, int64_t HW, int qmax, int hard, float* dx,
                                float* dp, void* ws, size_t ws_bytes, ssq_stream_t stream) {
  const char* what = "ssq_actshift_bwd";
  ActShifts sh;
  if (int rc = act_check(what, shifts, S, N, C, HW, qmax, sh)) return rc;
  // (the hard backward's dp is zero: a caller that does not read it passes NULL and saves
  // the launch that writes the zeros)
  SSQ_REQUIRE(dp != nullptr || hard, SSQ_E_ARG, "%s: null pointer (dp)", what);
  hipStream_t s = (hipStream_t)stream;
  const int fin_grid = grid_for(C * S, kBlock, 1 << 30);
  if (N == 0) {
    if (dp)
      hipLaunchKernelGGL(act_finish, dim3(fin_grid), dim3(kBlock), 0, s, nullptr, 0u, (uint32_t)C,
                         S, 1, dp);
    return check_launch(what);
  }
  SSQ_REQUIRE(x && g && p && delta && zp && dx, SSQ_E_ARG, "%s: null pointer", what);
  const bool vec = HW % 4 == 0 && act_aligned16(x) && act_aligned16(g) && act_aligned16(dx);
  if (hard) {
    act_launch<kBwdHard>(s, S, vec, x, g, dx, p, delta, zp, sh, (float)qmax, (uint32_t)(N * C),
                         (uint32_t)C, (uint32_t)HW, nullptr);
    if (dp)
      hipLaunchKernelGGL(act_finish, dim3(fin_grid), dim3(kBlock), 0, s, nullptr, 0u, (uint32_t)C,
                         S, 1, dp);
    return check_launch(what);
  }
  const size_t need = act_part_bytes(N, C, S);
  SSQ_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 7u) == 0, SSQ_E_WS,
              "%s: workspace of %zu bytes (8-B aligned) needed, %zu given", what, need, ws_bytes);
  act_launch<kBwdSoft>(s, S, vec, x, g, dx, p, delta, zp, sh, (float)qmax, (uint32_t)(N * C),
                       (uint32_t)C, (uint32_t)HW, (double*)ws);
  hipLaunchKernelGGL(act_finish, dim3(fin_grid), dim3(kBlock), 0, s, (const double*)ws,
                     (uint32_t)N, (uint32_t)C, S, 0, dp);
  return check_launch(what);
}

extern "C" size_t ssq_actshift_init_workspace_size(int64_t N, int64_t C, int64_t HW, int S) {
  (void)HW;
  return act_part_bytes(N, C, S);
}

extern "C" int ssq_actshift_init(const float* x, const float* delta, const float* zp,
                                 const float* shifts, int S, int64_t N, int64_t C, int64_t HW,
                                 int qmax, float* mse, void* ws, size_t ws_bytes,
                                 ssq_stream_t stream) {
  const char* what = "ssq_actshift_init";
  ActShifts sh;
  if (int rc = act_check(what, shifts, S, N, C, HW, qmax, sh)) return rc;
  SSQ_REQUIRE(mse != nullptr, SSQ_E_ARG, "%s: null pointer (mse)", what);
  hipStream_t s = (hipStream_t)stream;
  const int fin_grid = grid_for(C * S, kBlock, 1 << 30);
  if (N == 0) {
    hipLaunchKernelGGL(act_finish, dim3(fin_grid), dim3(kBlock), 0, s, nullptr, 0u, (uint32_t)C,
                       S, 1, mse);
    return check_launch(what);
  }
  SSQ_REQUIRE(x && delta && zp, SSQ_E_ARG, "%s: null pointer", what);
  const size_t need = act_part_bytes(N, C, S);
  SSQ_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 7u) == 0, SSQ_E_WS,
              "%s: workspace of %zu bytes (8-B aligned) needed, %zu given", what, need, ws_bytes);
  const bool vec = HW % 4 == 0 && act_aligned16(x);
  act_launch<kInit>(s, S, vec, x, nullptr, nullptr, nullptr, delta, zp, sh, (float)qmax,
                    (uint32_t)(N * C), (uint32_t)C, (uint32_t)HW, (double*)ws);
  hipLaunchKernelGGL(act_finish, dim3(fin_grid), dim3(kBlock), 0, s, (const double*)ws,
                     (uint32_t)N, (uint32_t)C, S, 0, mse);
  return check_launch(what);
}
