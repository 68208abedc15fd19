// K34: the shifted-scale act quantizer (K33, actshift.hip) inside the K13 epilogue pass
// ("K34").
//
// conv is a conv's raw output, (N, C, H*W) in NCHW order.  With K13's epilogue
//   x = act(((conv + bias[c]) * gamma[c] + phi[c]) + res)             (k13_elem, epilogue_elem.h)
// and K33's quantizer Q_shift (act_elem, actshift_kernels.h):
// forward   y = Q_shift(x).  Reads conv (+ res), writes y: 8 B/elem (+4); x is never stored.
// backward  x recomputed from conv (+ res); dx_q = K33's dx for the upstream g,
//           g_t = act_pass(x) ? dx_q : 0 (ssq_epilogue_bwd's mask rule: ReLU out <= 0, ReLU6 also
//           out >= 6, a NaN passes), dconv = g_t * gamma[c], dres = g_t, and K33's dp / ddelta
//           sums of (g, x).  Reads conv, g (+ res), writes dconv (+ dres): 12 B/elem (+8).
// The epilogue's own parameters get no gradient here: the act loop freezes them, and a caller
// that learns them takes K13's backward.
//
// The geometry is K33's: a group of TPP threads (a wave while a plane is at most 256 work items,
// the workgroup otherwise) owns whole (n, c) planes, so bias[c] / gamma[c] / phi[c] sit in
// scalar registers beside the channel's p row and the S grids.  Each thread issues kActU loads
// of every stream before any math: float4 items when H*W % 4 == 0, moved as one 16-B access
// when every base is 16-B aligned and as four dwords otherwise (the lane keeps the elements
// K33 gives it after K13, whose output is always aligned), single elements for other planes.
// A lane meets the elements K33's lane meets, in the same order, with the same
// element function on the same x bits; the plane sums are reduced by the same trees into the
// same workspace layout (dp partials, then one ddelta partial per plane) and summed over the
// planes by K33's finish kernels: y, dconv, dres, dp and ddelta are bit for bit those of
// ssq_epilogue_fwd -> ssq_actshift_fwd and ssq_actshift_bwd[_delta] -> ssq_epilogue_bwd.
// Which epilogue operands exist and the activation code are uniform kernel arguments (a
// scalar branch around k13_elem's instantiations), so the kernel count stays K33's.
#include "actshift_kernels.h"
#include "epilogue_elem.h"

namespace ssq {

// the epilogue's operands of one launch; b / ga / ph are the current plane's channel values
struct EpiAct {
  const float* bias;
  const float* gamma;   // with phi, or neither
  const float* phi;
  int relu;             // K13's activation code
  bool res;
  bool wide;            // every base 16-B aligned: the float4 form moves 16 B per access
  float b, ga, ph;
};

__device__ __forceinline__ void epi_act_channel(EpiAct& E, uint32_t c) {
  E.b = E.bias ? E.bias[c] : 0.0f;
  E.ga = E.gamma ? E.gamma[c] : 1.0f;
  E.ph = E.gamma ? E.phi[c] : 0.0f;
}

template <int ACT>
__device__ __forceinline__ float epi_act_x(const EpiAct& E, float v, float rv) {
  const bool bias = E.bias != nullptr;
  if (E.gamma)
    return E.res ? k13_elem<true, ACT, true>(bias, v, rv, E.b, E.ga, E.ph)
                 : k13_elem<false, ACT, true>(bias, v, rv, E.b, E.ga, E.ph);
  return E.res ? k13_elem<true, ACT, false>(bias, v, rv, E.b, E.ga, E.ph)
               : k13_elem<false, ACT, false>(bias, v, rv, E.b, E.ga, E.ph);
}
// x, the quantizer's input
__device__ __forceinline__ float epi_act_x(const EpiAct& E, float v, float rv) {
  return E.relu == 2 ? epi_act_x<2>(E, v, rv)
                     : (E.relu == 1 ? epi_act_x<1>(E, v, rv) : epi_act_x<0>(E, v, rv));
}
__device__ __forceinline__ bool epi_act_pass(const EpiAct& E, float x) {
  return E.relu == 2 ? act_pass<2>(x) : (E.relu == 1 ? act_pass<1>(x) : true);
}

template <int OP>
constexpr bool epi_act_bwd() { return OP != kFwdSoft && OP != kFwdHard; }
// double sums per plane: dp's S (soft), then ddelta's one
template <int S, int OP>
constexpr int epi_act_nd() { return (OP == kBwdSoft || OP == kBwdSoftD) ? S : 0; }
template <int S, int OP>
constexpr int epi_act_nacc() {
  return epi_act_nd<S, OP>() + ((OP == kBwdSoftD || OP == kBwdHardD) ? 1 : 0);
}

// One element: forward -> o0 = y; backward -> o0 = dconv, o1 = dres.
template <int S, int OP, bool FAST>
__device__ __forceinline__ void epi_act_elem(const EpiAct& E, const ActGrid<S>& G, float x,
                                             float gv, double* acc, float& o0, float& o1) {
  const float q = act_elem<S, OP, FAST>(x, gv, G, acc);
  if (!epi_act_bwd<OP>()) {
    o0 = q;
    o1 = 0.0f;
    return;
  }
  const float gt = epi_act_pass(E, x) ? q : 0.0f;
  o0 = E.gamma ? __fmul_rn(gt, E.ga) : gt;
  o1 = gt;
}

// Elements 4j .. 4j + 3 of a plane: one 16-B access (WIDE), or four dwords where a base is not
// 16-B aligned.
template <bool WIDE>
__device__ __forceinline__ f32x4 epi_act_load4(const float* __restrict__ q, uint32_t j) {
  if (WIDE) return ((const f32x4*)q)[j];
  return f32x4{q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3]};
}
__device__ __forceinline__ void epi_act_store4(float* __restrict__ q, uint32_t j, const float* a,
                                               bool wide) {
  if (wide) {
    ((f32x4*)q)[j] = f32x4{a[0], a[1], a[2], a[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) q[4 * j + e] = a[e];
  }
}
// a step's kActU loads of every stream, all issued before any math (j0: the lane's first item)
template <bool WIDE, bool BWD, int TPP>
__device__ __forceinline__ void epi_act_loads(const float* __restrict__ v,
                                              const float* __restrict__ r,
                                              const float* __restrict__ g, bool res, uint32_t j0,
                                              uint32_t n4, f32x4* vv, f32x4* vr, f32x4* vg) {
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int u = 0; u < kActU; ++u) {
    const uint32_t j = j0 + u * TPP;
    const bool on = j < n4;
    vv[u] = on ? epi_act_load4<WIDE>(v, j) : zero;
    vr[u] = (on && res) ? epi_act_load4<WIDE>(r, j) : zero;
    vg[u] = (BWD && on) ? epi_act_load4<WIDE>(g, j) : zero;
  }
}

// One plane of hw elements, walked by the TPP threads of the group as K33's act_plane walks it.
// v: the conv output; r: the residual (E.res); g: the upstream gradient (backward); o0 / o1:
// see epi_act_elem (either may be null: not stored).
template <int S, int OP, bool VEC, int TPP>
__device__ __forceinline__ void epi_act_plane(const float* __restrict__ v,
                                              const float* __restrict__ r,
                                              const float* __restrict__ g, float* __restrict__ o0,
                                              float* __restrict__ o1, uint32_t hw, const EpiAct& E,
                                              const ActGrid<S>& G, uint32_t lane, double* acc) {
  constexpr bool BWD = epi_act_bwd<OP>();
  if (VEC) {
    const uint32_t n4 = hw >> 2;
    for (uint32_t base = 0; base < n4; base += kActU * TPP) {
      f32x4 vv[kActU], vr[kActU], vg[kActU];
      if (E.wide) epi_act_loads<true, BWD, TPP>(v, r, g, E.res, base + lane, n4, vv, vr, vg);
      else epi_act_loads<false, BWD, TPP>(v, r, g, E.res, base + lane, n4, vv, vr, vg);
      float xe[kActU][4];
      unsigned ok = G.fast;
#pragma unroll
      for (int u = 0; u < kActU; ++u) {
        const uint32_t j = base + u * TPP + lane;
        const float ve[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
        const float re[4] = {vr[u].x, vr[u].y, vr[u].z, vr[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // (a lane past the plane's end tests x = 0, as K33's does)
          xe[u][e] = j < n4 ? epi_act_x(E, ve[e], re[e]) : 0.0f;
          ok &= (unsigned)div_fast_ok(xe[u][e]);
        }
      }
      const bool fast = __all(ok);
#pragma unroll
      for (int u = 0; u < kActU; ++u) {
        const uint32_t j = base + u * TPP + lane;
        if (j < n4) {
          const float ge[4] = {vg[u].x, vg[u].y, vg[u].z, vg[u].w};
          float a[4], b[4];
          if (fast) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              epi_act_elem<S, OP, true>(E, G, xe[u][e], ge[e], acc, a[e], b[e]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              epi_act_elem<S, OP, false>(E, G, xe[u][e], ge[e], acc, a[e], b[e]);
          }
          if (o0) epi_act_store4(o0, j, a, E.wide);
          if (BWD && o1) epi_act_store4(o1, j, b, E.wide);
        }
      }
    }
  } else {
    for (uint32_t base = 0; base < hw; base += kActU * TPP) {
      float vv[kActU], vr[kActU], vg[kActU], xe[kActU];
#pragma unroll
      for (int u = 0; u < kActU; ++u) {
        const uint32_t j = base + u * TPP + lane;
        const bool on = j < hw;
        vv[u] = on ? v[j] : 0.0f;
        vr[u] = (on && E.res) ? r[j] : 0.0f;
        vg[u] = (BWD && on) ? g[j] : 0.0f;
      }
      unsigned ok = G.fast;
#pragma unroll
      for (int u = 0; u < kActU; ++u) {
        const uint32_t j = base + u * TPP + lane;
        xe[u] = j < hw ? epi_act_x(E, vv[u], vr[u]) : 0.0f;
        ok &= (unsigned)div_fast_ok(xe[u]);
      }
      const bool fast = __all(ok);
#pragma unroll
      for (int u = 0; u < kActU; ++u) {
        const uint32_t j = base + u * TPP + lane;
        if (j < hw) {
          float a, b;
          if (fast) epi_act_elem<S, OP, true>(E, G, xe[u], vg[u], acc, a, b);
          else epi_act_elem<S, OP, false>(E, G, xe[u], vg[u], acc, a, b);
          if (o0) o0[j] = a;
          if (BWD && o1) o1[j] = b;
        }
      }
    }
  }
}

// Groups of TPP threads walk the planes group, group + ngroups, ...; plane pl is channel pl % C.
// part (backward): planes * ND doubles laid out as K33's dp partials (ND = S soft, 0 hard), then,
// for the ddelta forms, one partial per plane.
template <int S, int OP, bool VEC, int TPP>
__global__ __launch_bounds__(kBlock) SSQ_NO_PK_F32 void epi_act_kernel(
    const float* __restrict__ v, const float* __restrict__ r, const float* __restrict__ g,
    float* __restrict__ o0, float* __restrict__ o1, EpiAct E, const float* __restrict__ p,
    const float* __restrict__ delta, const float* __restrict__ zp, ActShifts sh, float hi,
    uint32_t planes, uint32_t C, uint32_t hw, double* __restrict__ part) {
  __shared__ double red[16];
  constexpr int ND = epi_act_nd<S, OP>();
  constexpr int NACC = epi_act_nacc<S, OP>();
  constexpr bool DELTA = OP == kBwdSoftD || OP == kBwdHardD;
  constexpr uint32_t GPB = kBlock / TPP;
  const uint32_t lane = threadIdx.x % TPP;
  const uint32_t ngroups = gridDim.x * GPB;
  ActGrid<S> G;
  act_grid_scales<S>(G, delta, zp, sh, hi);
  // (TPP == kBlock: one group per workgroup, so the trip count -- and every barrier of
  // block_sum below -- is uniform over the workgroup)
  for (uint32_t pl = blockIdx.x * GPB + threadIdx.x / TPP; pl < planes; pl += ngroups) {
    const uint32_t c = pl % C;
    act_grid_channel<S, DELTA, OP == kBwdHardD>(G, p, c, sh);
    epi_act_channel(E, c);
    double acc[NACC + 1];   // (+1: no zero-length array for the forms without sums)
#pragma unroll
    for (int i = 0; i <= NACC; ++i) acc[i] = 0.0;
    const size_t off = (size_t)pl * hw;
    epi_act_plane<S, OP, VEC, TPP>(v + off, E.res ? r + off : nullptr,
                                   epi_act_bwd<OP>() ? g + off : nullptr, o0 ? o0 + off : nullptr,
                                   o1 ? o1 + off : nullptr, hw, E, G, lane, acc);
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
      double t;
      if constexpr (TPP == kWave) t = wave_sum(acc[i]);
      else t = block_sum(acc[i], red);
      if (lane == 0) part[i < ND ? (size_t)pl * ND + i : (size_t)planes * ND + pl] = t;
    }
  }
}

struct EpiActArgs {
  const float *v, *r, *g;
  float *o0, *o1;
  EpiAct E;
  const float *p, *delta, *zp;
  ActShifts sh;
  float hi;
  uint32_t planes, C, hw;
  double* part;
};

template <int S, int OP>
static void epi_act_launch_s(hipStream_t s, bool vec, const EpiActArgs& a) {
  const ActGeometry geo = act_geometry(vec, a.planes, a.hw);
#define SSQ_EPI_ACT(VEC, TPP)                                                                   \
  hipLaunchKernelGGL((epi_act_kernel<S, OP, VEC, TPP>), dim3(geo.blocks), dim3(kBlock), 0, s,   \
                     a.v, a.r, a.g, a.o0, a.o1, a.E, a.p, a.delta, a.zp, a.sh, a.hi, a.planes,  \
                     a.C, a.hw, a.part)
  if (vec && geo.wave) SSQ_EPI_ACT(true, kWave);
  else if (vec) SSQ_EPI_ACT(true, kBlock);
  else if (geo.wave) SSQ_EPI_ACT(false, kWave);
  else SSQ_EPI_ACT(false, kBlock);
#undef SSQ_EPI_ACT
}

template <int OP>
static void epi_act_launch(hipStream_t s, int S, bool vec, const EpiActArgs& a) {
  switch (S) {
    case 1: epi_act_launch_s<1, OP>(s, vec, a); break;
    case 2: epi_act_launch_s<2, OP>(s, vec, a); break;
    case 3: epi_act_launch_s<3, OP>(s, vec, a); break;
    case 4: epi_act_launch_s<4, OP>(s, vec, a); break;
  }
}

// K33's and K13's refusals, before any launch
static int epi_act_check(const char* what, const float* gamma, const float* phi, int relu,
                         const float* shifts, int S, int64_t N, int64_t C, int64_t HW, int qmax,
                         ActShifts& sh) {
  if (int rc = act_check(what, shifts, S, N, C, HW, qmax, sh)) return rc;
  SSQ_REQUIRE(!gamma == !phi, SSQ_E_ARG, "%s: gamma and phi go together", what);
  SSQ_REQUIRE(relu >= 0 && relu <= 2, SSQ_E_ARG, "%s: activation code %d (0/1/2)", what, relu);
  return SSQ_OK;
}

}  // namespace ssq

using namespace ssq;

extern "C" int ssq_epilogue_actshift_fwd(const float* conv, const float* bias, const float* gamma,
                                         const float* phi, const float* res, int relu,
                                         const float* p, const float* delta, const float* zp,
                                         const float* shifts, int S, int64_t N, int64_t C,
                                         int64_t HW, int qmax, int hard, float* y,
                                         ssq_stream_t stream) {
  const char* what = "ssq_epilogue_actshift_fwd";
  EpiActArgs a{};
  if (int rc = epi_act_check(what, gamma, phi, relu, shifts, S, N, C, HW, qmax, a.sh)) return rc;
  if (N == 0) return SSQ_OK;
  SSQ_REQUIRE(conv && p && delta && zp && y, SSQ_E_ARG, "%s: null pointer", what);
  const bool vec = HW % 4 == 0;
  const bool wide = act_aligned16(conv) && act_aligned16(y) && (!res || act_aligned16(res));
  a.v = conv, a.r = res, a.o0 = y;
  a.E = EpiAct{bias, gamma, phi, relu, res != nullptr, wide, 0.0f, 1.0f, 0.0f};
  a.p = p, a.delta = delta, a.zp = zp, a.hi = (float)qmax;
  a.planes = (uint32_t)(N * C), a.C = (uint32_t)C, a.hw = (uint32_t)HW;
  hipStream_t s = (hipStream_t)stream;
  if (hard) epi_act_launch<kFwdHard>(s, S, vec, a);
  else epi_act_launch<kFwdSoft>(s, S, vec, a);
  return check_launch(what);
}

// the soft form with ddelta (dp's partials, then one double per plane); the other forms use less
extern "C" size_t ssq_epilogue_actshift_bwd_workspace_size(int64_t N, int64_t C, int64_t HW,
                                                           int S) {
  (void)HW;
  const size_t dp_bytes = act_part_bytes(N, C, S);
  return dp_bytes ? dp_bytes + (size_t)N * (size_t)C * sizeof(double) : 0;
}

extern "C" int ssq_epilogue_actshift_bwd(const float* conv, const float* g, const float* bias,
                                         const float* gamma, const float* phi, const float* res,
                                         int relu, const float* p, const float* delta,
                                         const float* zp, const float* shifts, int S, int64_t N,
                                         int64_t C, int64_t HW, int qmax, int hard, float* dconv,
                                         float* dres, float* dp, float* ddelta, void* ws,
                                         size_t ws_bytes, ssq_stream_t stream) {
  const char* what = "ssq_epilogue_actshift_bwd";
  EpiActArgs a{};
  if (int rc = epi_act_check(what, gamma, phi, relu, shifts, S, N, C, HW, qmax, a.sh)) return rc;
  SSQ_REQUIRE(dp != nullptr || hard, SSQ_E_ARG, "%s: null pointer (dp)", what);
  SSQ_REQUIRE(!dres || res, SSQ_E_ARG, "%s: dres without res", what);
  hipStream_t s = (hipStream_t)stream;
  if (N > 0) {
    SSQ_REQUIRE(conv && g && p && delta && zp, SSQ_E_ARG, "%s: null pointer", what);
    const size_t need = (size_t)N * (size_t)C * (size_t)((hard ? 0 : S) + (ddelta ? 1 : 0)) *
                        sizeof(double);
    SSQ_REQUIRE(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 7u) == 0), SSQ_E_WS,
                "%s: workspace of %zu bytes (8-B aligned) needed, %zu given", what, need, ws_bytes);
    // which elements a lane sums is K33's choice for an aligned x and this g (the dp / ddelta
    // bits depend on it); how they are loaded is the bases' alignment
    const bool vec = HW % 4 == 0 && act_aligned16(g);
    const bool wide = act_aligned16(conv) && (!res || act_aligned16(res)) &&
                      (!dconv || act_aligned16(dconv)) && (!dres || act_aligned16(dres));
    a.v = conv, a.r = res, a.g = g, a.o0 = dconv, a.o1 = dres;
    a.E = EpiAct{bias, gamma, phi, relu, res != nullptr, wide, 0.0f, 1.0f, 0.0f};
    a.p = p, a.delta = delta, a.zp = zp, a.hi = (float)qmax;
    a.planes = (uint32_t)(N * C), a.C = (uint32_t)C, a.hw = (uint32_t)HW;
    a.part = (double*)ws;
    if (hard && ddelta) epi_act_launch<kBwdHardD>(s, S, vec, a);
    else if (hard) epi_act_launch<kBwdHard>(s, S, vec, a);
    else if (ddelta) epi_act_launch<kBwdSoftD>(s, S, vec, a);
    else epi_act_launch<kBwdSoft>(s, S, vec, a);
  }
  // (N == 0: no plane, the finish stores dp = 0 and ddelta = 0)
  act_finish_launch(s, (const double*)ws, N, C, S, hard != 0, dp, ddelta);
  return check_launch(what);
}
