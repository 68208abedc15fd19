// K29-K30: the pooling head on int8 codes (quant/integer.py, carry_head).
//
// The head's input is an act quantizer's output x_hat = (q_a - z_a) * delta_a on an H x W
// plane, the fc's weight W_hat = (q_w - z_w[co]) * d1[co]; the fc has no input quantizer of its
// own, so the pooled value is never re-quantized:
//     P[n,c]  = sum_hw (q_a - z_a)                      exact integer, |P| <= 255 * HW
//     I[n,co] = sum_c P[n,c] (q_w[co,c] - z_w[co])      exact integer (int64)
//     y[n,co] = fp32(I) * sh[co]     sh[co] = fp32(fp32(delta_a * d1[co]) / fp32(HW)), the caller's
// one conversion (round to nearest even) and one multiply, no bias, no FMA: K23's contract with
// the 1 / HW of the mean folded into the scale.  On K21's stored form a_s = q_a - ca
// (ca = qmin_a + 128, az = ca - z_a) and K22's w_s, cwz, T for K = C:
//     P_s[n,c] = sum_hw a_s        P = P_s + HW * az
//     I = D + cwz[co] * SP[n] + HW * az * T[co]      D = sum_c P_s w_s     SP[n] = sum_c P_s[n,c]
// P_s does not fit int8 (|P_s| <= 128 * HW), so it is stored as two int8 digits
//     hi = (P_s + 64) >> 7 (arithmetic)      lo = P_s - 128 * hi  in [-64, 63]
// and D = 128 * D_hi + D_lo, two int8-MFMA products against the same weight fragment.
// HW <= 126 keeps |hi| <= 126; C <= 65536 keeps both int32 accumulators below 2^30.  The
// correction runs in int64: |I| passes 2^31 at C = 2048, HW = 49 with 8-bit operands.
//
// K29 ssq_avgpool_i8_digits_fwd: codes NHWC int8 [N][H*W][Cp] -> hi, lo [N][Cp] int8 and
// sp [N] int32; padded channels 0 in both planes, every output byte written by one thread.
// K30 ssq_qlinear_pooled_fwd: hi, lo, sp and the fc's K22 blob -> y [N][Co] fp32.
//
// A scaled fc (W_hat = (q_w - z_w[co]) d1[co] k / L, qinfer_prepare.h) whose centred operand
// m = (q_w - z_w[co]) k fits int8 is K22's centred blob in the kernel above as it stands: cwz = 0
// makes the cwz * SP term vanish, and the caller's sh[co] = fp32(fp32(delta_a * base[co]) /
// fp32(L * HW)) carries the grid (L * HW <= 1024 * 126 is exact in fp32: one division).  Beyond
// int8, ssq_qlinear_pooled_wide_fwd reads the dense wide blob (ssq_qweight_prepare_wide:
// m = 128 h + l, |m| <= 16319) with the WIDE instantiations: four products per fragment,
//     I = 128^2 D_hh + 128 (D_hl + D_lh) + D_ll + HW * az * T[co]     (D_xy = sum_c x_a y_w)
// in int64; C <= 65536 keeps every D below 2^30 (|hi| <= 126, |h| <= 127), and at HW = 126,
// C = 65536, |m| = 16319 |I| < 2^47.  SP is not read.
#include "ssq_common.h"
#include "qinfer_check.h"
#include "qinfer_layout.h"

namespace ssq {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int kHeadMaxHW = 126;
constexpr int kPoolMaxSlices = 16;   // pixel slices per chunk: bounds the LDS reduction's length
constexpr int kPoolBatch = 8;        // loads in flight per thread

// ---------------------------------------------------------------- K29 average pool to digits
// gfx950 has no packed int8 add: the even bytes of a dword ((x << 8) >> 8 per 16-bit half) and
// the odd ones (x >> 8 per half) are sign-extended into halves and summed with v_pk_add_u16;
// |P_s| <= 128 * 126 fits int16.  Half h of dword d holds channels 4d + 2h (even) and
// 4d + 2h + 1 (odd) of the 16-channel chunk.
struct DigAcc {
  i16x8 even, odd;
};

__device__ __forceinline__ void dig_add(DigAcc& a, i32x4 x) {
  a.even += __builtin_bit_cast(i16x8, __builtin_bit_cast(u16x8, x) << 8) >> 8;
  a.odd += __builtin_bit_cast(i16x8, x) >> 8;
}

// One workgroup per image.  A pass covers cpw = min(Cp / 16, 256) chunks; thread (slice, chunk)
// sums the pixels slice, slice + S, ... of its 16-B chunk (S = min(256 / cpw, 16) slices),
// kPoolBatch loads issued before their adds; the slices meet in LDS, the slice-0 thread of a
// chunk splits the 16 sums into digits and stores 16 B of each plane.  SP is a wave reduction
// of what those threads summed, then one LDS word per wave.
__global__ __launch_bounds__(kBlock) void avgpool_i8_digits_kernel(
    const int8_t* __restrict__ codes, uint32_t HW, uint32_t C, uint32_t nch, uint32_t cpw,
    uint32_t S, FastDiv div_cpw, int8_t* __restrict__ hi, int8_t* __restrict__ lo,
    int32_t* __restrict__ sp) {
  __shared__ __attribute__((aligned(16))) i32x4 red[kBlock * 2];
  __shared__ int wred[kBlock / kWave];
  const uint32_t tid = threadIdx.x, n = blockIdx.x;
  const uint32_t slice = fdiv(tid, div_cpw), cidx = tid - slice * cpw;
  const size_t Cp = (size_t)nch * 16;
  const int8_t* __restrict__ img = codes + (size_t)n * HW * Cp;
  int spacc = 0;
  for (uint32_t c0 = 0; c0 < nch; c0 += cpw) {
    const uint32_t chunk = c0 + cidx;
    const i16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    DigAcc a = {zero, zero};
    if (slice < S && chunk < nch) {
      const int8_t* __restrict__ p = img + (size_t)chunk * 16;
      uint32_t px = slice;
      for (; px + (kPoolBatch - 1) * S < HW; px += kPoolBatch * S) {
        i32x4 v[kPoolBatch];
#pragma unroll
        for (int t = 0; t < kPoolBatch; ++t) v[t] = *(const i32x4*)(p + (size_t)(px + t * S) * Cp);
#pragma unroll
        for (int t = 0; t < kPoolBatch; ++t) dig_add(a, v[t]);
      }
      for (; px < HW; px += S) dig_add(a, *(const i32x4*)(p + (size_t)px * Cp));
    }
    __syncthreads();   // the previous pass's reduction reads are done
    if (slice < S) {   // slot tid = slice * cpw + cidx < S * cpw <= kBlock
      red[tid * 2] = __builtin_bit_cast(i32x4, a.even);
      red[tid * 2 + 1] = __builtin_bit_cast(i32x4, a.odd);
    }
    __syncthreads();
    if (slice == 0 && chunk < nch) {
      for (uint32_t s = 1; s < S; ++s) {
        a.even += __builtin_bit_cast(i16x8, red[(s * cpw + cidx) * 2]);
        a.odd += __builtin_bit_cast(i16x8, red[(s * cpw + cidx) * 2 + 1]);
      }
      union {
        i32x4 v;
        int8_t b[16];
      } oh, ol;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int e = (j >> 2) * 2 + ((j >> 1) & 1);
        int P = (j & 1) ? (int)a.odd[e] : (int)a.even[e];
        P = chunk * 16 + j < C ? P : 0;
        const int h = (P + 64) >> 7;
        oh.b[j] = (int8_t)h;
        ol.b[j] = (int8_t)(P - 128 * h);
        spacc += P;
      }
      *(i32x4*)(hi + (size_t)n * Cp + (size_t)chunk * 16) = oh.v;
      *(i32x4*)(lo + (size_t)n * Cp + (size_t)chunk * 16) = ol.v;
    }
  }
  // not wave_sum(uint32_t): through the helper one instruction of this kernel's stream moves
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) spacc += __shfl_xor(spacc, o, kWave);
  if ((tid & (kWave - 1)) == 0) wred[tid / kWave] = spacc;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int i = 0; i < kBlock / kWave; ++i) total += wred[i];
    sp[n] = total;
  }
}

// ---------------------------------------------------------------- K30 int8 linear on digits
struct QHeadGeo {
  uint32_t N, Cp, Co, Kp;
  long long hwaz;   // HW * az
};

// K23's tile and lane map with images where pixels stood: 64 output channels x IT images x 64 k
// per workgroup of 4 waves, operands register-staged into LDS rows of 64 B at an 80 B stride,
// the next k step's global loads in flight during the MFMAs, weights as the A operand (C rows
// are channels, C columns images).  Two activation fragments per step (hi, lo) against one
// weight fragment; no SA product, SP arrives from K29.
// IT = 64: wave w owns images 16w..16w+15 against all 64 channels (8 MFMAs per step).
// IT = 16: wave w owns channels 16w..16w+15 against the tile's 16 images (2 MFMAs per step).
// WIDE: lW rows [0, 64) hold the h plane's tile, [64, 128) the l plane's (`plane` bytes behind);
// acch / accl are then D_hh / D_lh and acchl / accll D_hl / D_ll (activation digit first), twice
// the MFMAs; `sp` and `cwz` are not read.
template <int IT, bool WIDE = false>
__global__ __launch_bounds__(kBlock) void qlinear_pooled_kernel(
    const int8_t* __restrict__ hi, const int8_t* __restrict__ lo, const int32_t* __restrict__ sp,
    const int8_t* __restrict__ wp, const int32_t* __restrict__ cwz,
    const int32_t* __restrict__ tt, const float* __restrict__ sh, QHeadGeo g,
    float* __restrict__ y) {
  static_assert(IT == 64 || IT == 16, "image tile");
  constexpr int NJ = IT == 64 ? 4 : 1;
  __shared__ __attribute__((aligned(16))) int8_t lW[(WIDE ? 2 : 1) * kQT * kQRow];
  __shared__ __attribute__((aligned(16))) int8_t lH[IT * kQRow];
  __shared__ __attribute__((aligned(16))) int8_t lL[IT * kQRow];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & (kWave - 1), wave = tid / kWave;
  const uint32_t fr = lane & 15, fq = lane >> 4;
  const uint32_t ib = IT == 64 ? wave : 0u;   // the wave's image fragment

  // staging role: one 16-byte chunk of each operand tile per thread
  const uint32_t srow = tid >> 2, sc = tid & 3;
  const uint32_t gi = blockIdx.x * IT + srow;
  const bool stage = srow < (uint32_t)IT;
  const bool ival = stage && gi < g.N;
  const size_t aoff = (size_t)(ival ? gi : 0u) * g.Cp + sc * 16;
  const int8_t* wrow = wp + (size_t)(blockIdx.y * kQT + srow) * g.Kp + sc * 16;
  const size_t plane = WIDE ? (size_t)gridDim.y * kQT * g.Kp : 0;   // Cop * Kp
  const i32x4 zero = {0, 0, 0, 0};

  // Cp is a multiple of 16: a chunk that starts below Cp lies inside the row
  auto load_a = [&](const int8_t* __restrict__ base, uint32_t kt) -> i32x4 {
    if (ival && kt * kQT + sc * 16 < g.Cp) return *(const i32x4*)(base + aoff + (size_t)kt * kQT);
    return zero;
  };

  i32x4 rh = load_a(hi, 0), rl = load_a(lo, 0);
  i32x4 rb = *(const i32x4*)wrow;
  i32x4 rb2 = zero;   // WIDE: the l plane's chunk
  if constexpr (WIDE) rb2 = *(const i32x4*)(wrow + plane);

  i32x4 acch[NJ], accl[NJ];
  i32x4 acchl[WIDE ? NJ : 1], accll[WIDE ? NJ : 1];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acch[j] = accl[j] = zero;
#pragma unroll
  for (int j = 0; j < (WIDE ? NJ : 1); ++j) acchl[j] = accll[j] = zero;

  const uint32_t nk = g.Kp / kQT;
  for (uint32_t kt = 0; kt < nk; ++kt) {
    __syncthreads();   // the previous step's fragment reads are done
    *(i32x4*)(lW + srow * kQRow + sc * 16) = rb;
    if constexpr (WIDE) *(i32x4*)(lW + (kQT + srow) * kQRow + sc * 16) = rb2;
    if (stage) {
      *(i32x4*)(lH + srow * kQRow + sc * 16) = rh;
      *(i32x4*)(lL + srow * kQRow + sc * 16) = rl;
    }
    __syncthreads();
    if (kt + 1 < nk) {
      rh = load_a(hi, kt + 1);
      rl = load_a(lo, kt + 1);
      rb = *(const i32x4*)(wrow + (size_t)(kt + 1) * kQT);
      if constexpr (WIDE) rb2 = *(const i32x4*)(wrow + plane + (size_t)(kt + 1) * kQT);
    }
    const i32x4 hf = *(const i32x4*)(lH + (ib * 16 + fr) * kQRow + fq * 16);
    const i32x4 lf = *(const i32x4*)(lL + (ib * 16 + fr) * kQRow + fq * 16);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const uint32_t crow = (IT == 64 ? (uint32_t)j : wave) * 16;
      const i32x4 wf = *(const i32x4*)(lW + (crow + fr) * kQRow + fq * 16);
      acch[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, hf, acch[j], 0, 0, 0);
      accl[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, lf, accl[j], 0, 0, 0);
      if constexpr (WIDE) {
        const i32x4 wl = *(const i32x4*)(lW + (kQT + crow + fr) * kQRow + fq * 16);
        acchl[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wl, hf, acchl[j], 0, 0, 0);
        accll[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wl, lf, accll[j], 0, 0, 0);
      }
    }
  }

  // C/D map: column (image) = lane & 15, row (channel) = 4 * (lane >> 4) + reg
  const uint32_t image = blockIdx.x * IT + ib * 16 + fr;
  if (image >= g.N) return;
  const long long spn = WIDE ? 0ll : (long long)sp[image];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const uint32_t crow = (IT == 64 ? (uint32_t)j : wave) * 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t co = blockIdx.y * kQT + crow + fq * 4 + r;
      if (co < g.Co) {
        long long I;
        if constexpr (WIDE)
          I = 16384ll * (long long)acch[j][r] +
              128ll * ((long long)acchl[j][r] + (long long)accl[j][r]) +
              (long long)accll[WIDE ? j : 0][r] + g.hwaz * (long long)tt[co];
        else
          I = 128ll * (long long)acch[j][r] + (long long)accl[j][r] + (long long)cwz[co] * spn +
              g.hwaz * (long long)tt[co];
        y[(size_t)image * g.Co + co] = __fmul_rn((float)I, sh[co]);
      }
    }
  }
}

}  // namespace ssq

using namespace ssq;

// K30's image tile (16 or 64): A/B plumbing for tools/int_infer_head_rate.py
static int g_head_tile = 16;
static int head_tile() { return g_head_tile; }

extern "C" int ssq_qlinear_pooled_set_tile(int tile) {
  const int old = g_head_tile;
  if (tile == 16 || tile == 64) g_head_tile = tile;
  return old;
}

extern "C" int ssq_avgpool_i8_digits_fwd(const int8_t* codes, int64_t Nb, int64_t C, int64_t H,
                                         int64_t W, int8_t* hi, int8_t* lo, int32_t* sp,
                                         ssq_stream_t stream) {
  const char* me = "ssq_avgpool_i8_digits_fwd";
  SSQ_REQUIRE(codes && hi && lo && sp, SSQ_E_ARG, "%s: null pointer", me);
  SSQ_REQUIRE(Nb >= 1 && C >= 1 && H >= 1 && W >= 1, SSQ_E_ARG, "%s: bad geometry", me);
  SSQ_REQUIRE(H <= kHeadMaxHW && W <= kHeadMaxHW && H * W <= kHeadMaxHW, SSQ_E_ARG,
              "%s: H*W = %lld exceeds %d (the int8 digit range)", me, (long long)(H * W),
              kHeadMaxHW);
  SSQ_REQUIRE(C <= kQMaxK, SSQ_E_ARG, "%s: C = %lld exceeds 65536", me, (long long)C);
  const int64_t Cp = rup(C, 16);
  // (H * W * Cp <= 126 * 65536: the product cannot wrap once Nb is below 2^31)
  SSQ_REQUIRE(Nb < (1ll << 31) && Nb * H * W * Cp < (1ll << 31), SSQ_E_ARG,
              "%s: tensor exceeds 2^31 elements", me);
  const uint32_t nch = (uint32_t)(Cp / 16);
  const uint32_t cpw = nch < (uint32_t)kBlock ? nch : (uint32_t)kBlock;
  uint32_t S = (uint32_t)kBlock / cpw;
  if (S > (uint32_t)kPoolMaxSlices) S = kPoolMaxSlices;
  hipLaunchKernelGGL(avgpool_i8_digits_kernel, dim3((uint32_t)Nb), dim3(kBlock), 0,
                     (hipStream_t)stream, codes, (uint32_t)(H * W), (uint32_t)C, nch, cpw, S,
                     make_fastdiv(cpw), hi, lo, sp);
  return check_launch(me);
}

// wide: ssq_qlinear_pooled_wide_fwd, on a blob of ssq_qweight_prepare_wide
static int qlinear_pooled_launch(const char* me, bool wide, const int8_t* hi, const int8_t* lo,
                                 const int32_t* sp, const void* prepared, const float* scale_h,
                                 int64_t Nb, int64_t Ci, int64_t Co, int64_t HW,
                                 float act_zero_point, int act_qmin, int act_qmax, float* y,
                                 ssq_stream_t stream) {
  SSQ_REQUIRE(hi && lo && sp && prepared && scale_h && y, SSQ_E_ARG, "%s: null pointer", me);
  SSQ_REQUIRE(Nb >= 1 && Ci >= 1 && Co >= 1, SSQ_E_ARG, "%s: bad geometry", me);
  SSQ_REQUIRE(Nb < (1ll << 31) && Co < (1ll << 31), SSQ_E_ARG,
              "%s: tensor exceeds 2^31 elements", me);
  SSQ_REQUIRE(HW >= 1 && HW <= kHeadMaxHW, SSQ_E_ARG,
              "%s: HW = %lld not in [1, %d] (the int8 digit range)", me, (long long)HW, kHeadMaxHW);
  SSQ_REQUIRE(Ci <= kQMaxK, SSQ_E_ARG, "%s: C = %lld exceeds 65536 (int32 accumulator range)", me,
              (long long)Ci);
  const int rc = qquant_ok(me, "activation ", nullptr, act_zero_point, act_qmin, act_qmax);
  if (rc) return rc;
  const QLayout L = qlayout(Co, Ci, 1, 1, wide ? 2 : 1);
  SSQ_REQUIRE(L.off_mask < (1ull << 31), SSQ_E_ARG, "%s: prepared weights exceed 2^31 bytes", me);
  SSQ_REQUIRE(Nb * L.Cp < (1ll << 31) && Nb * Co < (1ll << 31), SSQ_E_ARG,
              "%s: tensor exceeds 2^31 elements", me);
  QHeadGeo g;
  g.N = (uint32_t)Nb;
  g.Cp = (uint32_t)L.Cp;
  g.Co = (uint32_t)Co;
  g.Kp = (uint32_t)L.Kp;
  g.hwaz = (long long)HW * (long long)(act_qmin + 128 - (int)act_zero_point);
  const int8_t* base = (const int8_t*)prepared;
  const int32_t* cwz = (const int32_t*)(base + L.off_cwz);
  const int32_t* tt = (const int32_t*)(base + L.off_t);
  const uint32_t ctiles = (uint32_t)(L.Cop / kQT);
  const int it = head_tile();
  auto* kernel = it == 64 ? (wide ? qlinear_pooled_kernel<64, true> : qlinear_pooled_kernel<64>)
                          : (wide ? qlinear_pooled_kernel<16, true> : qlinear_pooled_kernel<16>);
  hipLaunchKernelGGL(kernel, dim3((g.N + (uint32_t)it - 1) / (uint32_t)it, ctiles), dim3(kBlock), 0,
                     (hipStream_t)stream, hi, lo, sp, base, cwz, tt, scale_h, g, y);
  return check_launch(me);
}

extern "C" int ssq_qlinear_pooled_fwd(const int8_t* hi, const int8_t* lo, const int32_t* sp,
                                      const void* prepared, const float* scale_h, int64_t Nb,
                                      int64_t Ci, int64_t Co, int64_t HW, float act_zero_point,
                                      int act_qmin, int act_qmax, float* y, ssq_stream_t stream) {
  return qlinear_pooled_launch("ssq_qlinear_pooled_fwd", false, hi, lo, sp, prepared, scale_h, Nb,
                               Ci, Co, HW, act_zero_point, act_qmin, act_qmax, y, stream);
}

extern "C" int ssq_qlinear_pooled_wide_fwd(const int8_t* hi, const int8_t* lo, const int32_t* sp,
                                           const void* prepared, const float* scale_h, int64_t Nb,
                                           int64_t Ci, int64_t Co, int64_t HW,
                                           float act_zero_point, int act_qmin, int act_qmax,
                                           float* y, ssq_stream_t stream) {
  return qlinear_pooled_launch("ssq_qlinear_pooled_wide_fwd", true, hi, lo, sp, prepared, scale_h,
                               Nb, Ci, Co, HW, act_zero_point, act_qmin, act_qmax, y, stream);
}
