// The code-emitting epilogue of the integer conv kernels (K23 / K25 / K26 with CODES = true):
// an output element leaves as the int8 code its consumer's K21 would re-derive, not as fp32.
//
// For the exact integer sum I of channel co, qepi_code runs the fp32 operations the uncarried
// route runs between the conv and the next conv's operand, in their order:
//     y    = fp32(I) * s[co]                       the conv kernel's own output
//     pre  = y + bias[co]                          K13 (recon.hip epi / epi_elem), if bias
//     t    = pre * gamma[co] + phi[co]             two roundings, if gamma / phi
//     t    = t + rv                                K13's residual add, if a residual (RES)
//     t    = act(t)                                act_fwd: 0 identity, 1 ReLU, 2 ReLU6
//     v    = round_ste(t / d) + z                  IEEE divide; NaN at an infinite t / d
//     q    = clamp(v, lo, hi)                      NaN stays NaN
//     code = (int)(q - lo) - 128                   K21's stored form, q - (qmin + 128)
// K13 would write (q - z) * d and K21 map it back to q; where K21 counts nothing off-grid that
// round trip is the identity, and where q is NaN K21 stores qmin and counts the element: so
// does this (the caller sums `nbad` over the wave into one atomic, as K21 does).
//
// The output is K21's layout: NHWC int8, channels padded to Cpo = 16*ceil(Co/16), padded
// channels 0.
#pragma once
#include "ssq_common.h"
#include "qinfer_check.h"

namespace ssq {

struct QEpi {
  const float* bias;    // [Co] or null
  const float* gamma;   // [Co] or null (with phi)
  const float* phi;
  float d, z, lo, hi;   // the output act quantizer
  int act;              // 0 identity, 1 ReLU, 2 ReLU6
  uint32_t Cpo;         // padded output channels
  int8_t* out;          // [Nb*OH*OW][Cpo]
  uint32_t* bad;
};

// A block tail's residual operand (K23 only): the fp32 NCHW tensor K13 would add, or the int8
// codes (K21's stored form, the output's pixel and channel layout) of a carried block input
// with that tensor's own act quantizer.  Exactly one pointer is set.
struct QRes {
  const float* f32;     // [Nb, Co, OH, OW] or null
  const int8_t* codes;  // [Nb*OH*OW][Cpo] or null
  float d, z, lo;       // the residual codes' quantizer
};

struct QEpiRes {
  QEpi e;
  QRes r;
};

__device__ __forceinline__ const QEpi& qepi_of(const QEpi& e) { return e; }
__device__ __forceinline__ const QEpi& qepi_of(const QEpiRes& er) { return er.e; }

// the fp32 value act_decode_kernel writes for a stored code: (q - z) * d, q = code + 128 + lo
__device__ __forceinline__ float qres_decode(int code, const QRes& r) {
  const float q = __fadd_rn((float)(code + 128), r.lo);   // exact: |q| <= 255
  return __fmul_rn(__fsub_rn(q, r.z), r.d);
}

// The epilogue from the conv's fp32 output y on (the list above from `pre`): what K27
// (qinfer_stem.hip) runs on an fp32 conv's output and the integer kernels after their own product.
// RES: `rv` is the residual K13 adds between the affine and the activation
template <bool RES = false>
__device__ __forceinline__ int qepi_code_y(float y, uint32_t co, const QEpi& e, uint32_t& nbad,
                                           float rv = 0.0f) {
  const float pre = e.bias ? __fadd_rn(y, e.bias[co]) : y;
  float t = e.gamma ? __fadd_rn(__fmul_rn(pre, e.gamma[co]), e.phi[co]) : pre;
  if constexpr (RES) t = __fadd_rn(t, rv);
  t = e.act == 1 ? act_fwd<1>(t) : (e.act == 2 ? act_fwd<2>(t) : t);
  const float v = round_ste_zp(t / e.d, e.z);
  float q = clampf(v, e.lo, e.hi);
  if (q != q) {   // NaN: stored as qmin and counted, as K21 does with K13's NaN
    q = e.lo;
    nbad += 1u;
  }
  return (int)__fsub_rn(q, e.lo) - 128;
}

template <bool RES = false>
__device__ __forceinline__ int qepi_code(float fI, uint32_t co, const float* __restrict__ scale,
                                         const QEpi& e, uint32_t& nbad, float rv = 0.0f) {
  return qepi_code_y<RES>(__fmul_rn(fI, scale[co]), co, e, nbad, rv);
}

// four codes (each in [-128, 127]) as the bytes of one word, c0 lowest
__device__ __forceinline__ int qepi_pack4(int c0, int c1, int c2, int c3) {
  return (c0 & 0xff) | ((c1 & 0xff) << 8) | ((c2 & 0xff) << 16) | ((int)((uint32_t)c3 << 24));
}

// every lane of the wave must be here
__device__ __forceinline__ void qepi_count(uint32_t nbad, uint32_t* bad) {
  nbad = wave_sum(nbad);
  if ((threadIdx.x & (kWave - 1)) == 0 && nbad) atomicAdd(bad, nbad);
}

// The epilogue's arguments checked (the output quantizer as ssq_act_encode checks its own) and
// gathered; the caller sets Cpo.
static inline int qepi_init(const char* what, const float* bias, const float* gamma,
                            const float* phi, int act, float delta, float zero_point, int qmin,
                            int qmax, int8_t* out, uint32_t* bad, QEpi* e) {
  SSQ_REQUIRE(out && bad, SSQ_E_ARG, "%s: null pointer", what);
  SSQ_REQUIRE((gamma == nullptr) == (phi == nullptr), SSQ_E_ARG,
              "%s: gamma and phi go together", what);
  SSQ_REQUIRE(act >= 0 && act <= 2, SSQ_E_ARG, "%s: activation code %d not in [0, 2]", what, act);
  const int rc = qquant_ok(what, "output ", &delta, zero_point, qmin, qmax);
  if (rc) return rc;
  *e = {bias, gamma, phi, delta, zero_point, (float)qmin, (float)qmax, act, 0u, out, bad};
  return SSQ_OK;
}

// A tail's residual likewise: exactly one operand, the codes' quantizer held to the same rules
static inline int qres_init(const char* what, const float* res_f32, const int8_t* res_codes,
                            float delta, float zero_point, int qmin, int qmax, QRes* r) {
  SSQ_REQUIRE((res_f32 != nullptr) != (res_codes != nullptr), SSQ_E_ARG,
              "%s: exactly one of res_f32 and res_codes must be set", what);
  const int rc = res_codes ? qquant_ok(what, "residual ", &delta, zero_point, qmin, qmax) : SSQ_OK;
  if (rc) return rc;
  *r = {res_f32, res_codes, delta, zero_point, (float)qmin};
  return SSQ_OK;
}

}  // namespace ssq
