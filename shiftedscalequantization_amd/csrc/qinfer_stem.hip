// K27-K28: int8 codes from the stem through the max-pool (quant/integer.py, carry_stem).
//
// K27 ssq_epilogue_codes_fwd: the K13 epilogue of an fp32 conv output (the stem conv stays on
// the fp32 route: its input is an unquantized image), leaving as K21's stored codes instead of
// the act quantizer's fp32 output.  Per element it runs qepi_code_y (qinfer_epi.h), the tail the
// integer kernels' code epilogue runs after their own product, so the bytes are the ones K21
// derives from K13's output wherever K21 counts nothing off-grid; a NaN is stored as qmin and
// counted, as K21 does.
//
// K28 ssq_maxpool_i8_fwd: the max-pool on stored codes.  (q - z) * d rounded to fp32 is
// non-decreasing in q for d > 0, so the max of the decoded values is the decoded max code; the
// stored form q - (qmin + 128) is shifted by one constant per tensor, so the signed byte order
// is the code order.  An out-of-bounds tap is skipped (it stands for -inf; 2 * pad <= K leaves
// every window a real tap); padded channels stay 0, the maximum of zeros.
//
// Layouts: fp32 NCHW in (K27), NHWC int8 with C padded to Cp = 16*ceil(C/16) otherwise.
#include "ssq_common.h"
#include "qinfer_epi.h"
#include "qinfer_layout.h"

namespace ssq {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------- K27 epilogue to codes
// One wave per (64 consecutive pixels, 16-channel chunk): lane = pixel, so each of the 16 channel
// loads is 256 contiguous bytes and the chunk index is wave-uniform (bias / gamma / phi are
// scalar loads).  Consecutive waves take the chunks of the same 64 pixels, so the 16-B stores of
// a workgroup fill one contiguous 64 * Cp-byte span of the output.
__global__ __launch_bounds__(kBlock) void epilogue_codes_kernel(const float* __restrict__ y,
                                                                uint32_t npix, uint32_t HW,
                                                                uint32_t C, uint32_t nch,
                                                                uint32_t nwork, FastDiv div_nch,
                                                                FastDiv div_hw, QEpi e) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t wstride = gridDim.x * (kBlock / kWave);
  uint32_t nbad = 0;
  for (uint32_t w0 = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave; w0 < nwork;
       w0 += wstride) {
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)w0);
    const uint32_t pb = fdiv(w, div_nch);
    const uint32_t c0 = (w - pb * nch) * 16;
    const uint32_t pix = pb * kWave + lane;
    if (pix < npix) {
      const uint32_t n = fdiv(pix, div_hw);
      const float* src = y + ((size_t)n * C + c0) * HW + (pix - n * HW);
      float v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = c0 + j < C ? src[(size_t)j * HW] : 0.0f;
      int c[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) c[j] = c0 + j < C ? qepi_code_y(v[j], c0 + j, e, nbad) : 0;
      i32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = qepi_pack4(c[4 * k], c[4 * k + 1], c[4 * k + 2], c[4 * k + 3]);
      *(i32x4*)(e.out + (size_t)pix * e.Cpo + c0) = o;
    }
  }
  qepi_count(nbad, e.bad);
}

// ---------------------------------------------------------------- K28 max-pool on codes
// gfx950 has no packed int8 max: each dword goes through two v_pk_max_i16.  As signed 16-bit
// halves, x orders by its odd bytes first and x << 8 by its even bytes first, whatever the low
// byte of a half holds; so the high byte of each half of the running maxima is the byte maximum.
struct PoolAcc {
  i32x4 odd, even;
};

__device__ __forceinline__ i32x4 pk_max_i16(i32x4 a, i32x4 b) {
  return __builtin_bit_cast(i32x4, __builtin_elementwise_max(__builtin_bit_cast(i16x8, a),
                                                             __builtin_bit_cast(i16x8, b)));
}

__device__ __forceinline__ void pool_tap(PoolAcc& m, i32x4 x) {
  m.odd = pk_max_i16(m.odd, x);
  m.even = pk_max_i16(m.even, __builtin_bit_cast(i32x4, __builtin_bit_cast(u32x4, x) << 8));
}

__device__ __forceinline__ i32x4 pool_result(const PoolAcc& m) {
  const u32x4 hi = __builtin_bit_cast(u32x4, m.odd) & 0xff00ff00u;
  const u32x4 lo = (__builtin_bit_cast(u32x4, m.even) >> 8) & 0x00ff00ffu;
  return __builtin_bit_cast(i32x4, hi | lo);
}

// One thread per (output pixel, 16-B chunk), the chunks of a pixel on consecutive lanes.
// KT > 0: the window size at compile time, all KT * KT loads issued before the compares (an
// out-of-bounds tap reads a clamped in-plane address and enters as -128, the identity).
template <int KT>
__global__ __launch_bounds__(kBlock) void maxpool_i8_kernel(const int8_t* __restrict__ codes,
                                                            int8_t* __restrict__ out, uint32_t total,
                                                            uint32_t nch, uint32_t H, uint32_t W,
                                                            uint32_t OH, uint32_t OW, uint32_t Kr,
                                                            uint32_t st, int pad, FastDiv div_nch,
                                                            FastDiv div_ow, FastDiv div_oh) {
  const int kMin = (int)0x80808080u;
  const i32x4 none = {kMin, kMin, kMin, kMin};
  const uint32_t Cp = nch * 16;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const uint32_t opix = fdiv(i, div_nch), ch = i - opix * nch;
    const uint32_t q1 = fdiv(opix, div_ow), ow = opix - q1 * OW;
    const uint32_t n = fdiv(q1, div_oh), oh = q1 - n * OH;
    const int8_t* __restrict__ xp = codes + (size_t)n * H * W * Cp + (size_t)ch * 16;
    const int h0 = (int)(oh * st) - pad, w0 = (int)(ow * st) - pad;
    PoolAcc m = {none, none};
    if constexpr (KT > 0) {
      i32x4 v[KT * KT];
      bool ok[KT * KT];
#pragma unroll
      for (int r = 0; r < KT; ++r)
#pragma unroll
        for (int s = 0; s < KT; ++s) {
          const int h = h0 + r, w = w0 + s;
          ok[r * KT + s] = h >= 0 && h < (int)H && w >= 0 && w < (int)W;
          const int hc = min(max(h, 0), (int)H - 1), wc = min(max(w, 0), (int)W - 1);
          v[r * KT + s] = *(const i32x4*)(xp + ((size_t)hc * W + wc) * Cp);
        }
#pragma unroll
      for (int t = 0; t < KT * KT; ++t) pool_tap(m, ok[t] ? v[t] : none);
    } else {
      for (uint32_t r = 0; r < Kr; ++r) {
        const int h = h0 + (int)r;
        if (h < 0 || h >= (int)H) continue;
        for (uint32_t s = 0; s < Kr; ++s) {
          const int w = w0 + (int)s;
          if (w < 0 || w >= (int)W) continue;
          pool_tap(m, *(const i32x4*)(xp + ((size_t)h * W + w) * Cp));
        }
      }
    }
    *(i32x4*)(out + (size_t)i * 16) = pool_result(m);
  }
}

}  // namespace ssq

using namespace ssq;

extern "C" int ssq_epilogue_codes_fwd(const float* y, const float* bias, const float* gamma,
                                      const float* phi, int64_t Nb, int64_t C, int64_t H,
                                      int64_t W, int act, float out_delta, float out_zero_point,
                                      int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad,
                                      ssq_stream_t stream) {
  const char* me = "ssq_epilogue_codes_fwd";
  SSQ_REQUIRE(y, SSQ_E_ARG, "%s: null pointer", me);
  QEpi e;
  const int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin,
                           out_qmax, out_codes, bad, &e);
  if (rc) return rc;
  SSQ_REQUIRE(Nb >= 1 && C >= 1 && H >= 1 && W >= 1, SSQ_E_ARG, "%s: bad geometry", me);
  const int64_t Cp = rup(C, 16);
  SSQ_REQUIRE(Nb * H * W * Cp < (1ll << 31), SSQ_E_ARG, "%s: tensor exceeds 2^31 elements", me);
  const uint32_t npix = (uint32_t)(Nb * H * W), nch = (uint32_t)(Cp / 16);
  const uint32_t nwork = (npix + kWave - 1) / kWave * nch;
  e.Cpo = (uint32_t)Cp;
  const dim3 grid(grid_for((int64_t)nwork * kWave, kBlock, 8192));
  hipLaunchKernelGGL(epilogue_codes_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, y, npix,
                     (uint32_t)(H * W), (uint32_t)C, nch, nwork, make_fastdiv(nch),
                     make_fastdiv((uint32_t)(H * W)), e);
  return check_launch(me);
}

extern "C" int ssq_maxpool_i8_fwd(const int8_t* codes, int64_t Nb, int64_t C, int64_t H, int64_t W,
                                  int64_t K, int64_t stride, int64_t pad, int8_t* out,
                                  ssq_stream_t stream) {
  const char* me = "ssq_maxpool_i8_fwd";
  SSQ_REQUIRE(codes && out, SSQ_E_ARG, "%s: null pointer", me);
  SSQ_REQUIRE(Nb >= 1 && C >= 1 && H >= 1 && W >= 1 && K >= 1 && K <= 7 && stride >= 1 &&
                  pad >= 0 && 2 * pad <= K,
              SSQ_E_ARG, "%s: bad geometry (K <= 7, pad <= K / 2, stride >= 1)", me);
  const int64_t OH = (H + 2 * pad - K) / stride + 1, OW = (W + 2 * pad - K) / stride + 1;
  SSQ_REQUIRE(H + 2 * pad >= K && W + 2 * pad >= K && OH >= 1 && OW >= 1, SSQ_E_ARG,
              "%s: empty output", me);
  const int64_t Cp = rup(C, 16);
  SSQ_REQUIRE(Nb * H * W * Cp < (1ll << 31) && Nb * OH * OW * Cp < (1ll << 31), SSQ_E_ARG,
              "%s: tensor exceeds 2^31 elements", me);
  const uint32_t nch = (uint32_t)(Cp / 16);
  const uint32_t total = (uint32_t)(Nb * OH * OW) * nch;
  const dim3 grid(grid_for(total, kBlock, 8192));
#define SSQ_MPI8(KT)                                                                          \
  hipLaunchKernelGGL(maxpool_i8_kernel<KT>, grid, dim3(kBlock), 0, (hipStream_t)stream, codes,  \
                     out, total, nch, (uint32_t)H, (uint32_t)W, (uint32_t)OH, (uint32_t)OW,    \
                     (uint32_t)K, (uint32_t)stride, (int)pad, make_fastdiv(nch),               \
                     make_fastdiv((uint32_t)OW), make_fastdiv((uint32_t)OH))
  if (K == 3) SSQ_MPI8(3);
  else if (K == 2) SSQ_MPI8(2);
  else SSQ_MPI8(0);
#undef SSQ_MPI8
  return check_launch(me);
}
