// K21-K23: integer inference from the packed export (int8 MFMA conv / linear).
//
// An interior layer of a calibrated model reads an input on an integer grid,
// x_hat = (q_a - z_a) * delta_a (scalar delta_a, z_a), and a weight on one,
// W_hat = (q_w - z_w[co]) * d1[co], so its raw output is
//     y[co] = fp32(I) * s[co],   I = sum_k (q_a - z_a)(q_w - z_w[co]),   s[co] = fp32(delta_a * d1[co])
// with I an exact integer.  q - z spans +-255 at 8 bits and does not fit int8, so both
// operands are stored shifted by a per-tensor constant,
//     a_s = q_a - ca,  ca = qmin_a + 128        w_s = q_w - cw,  cw = qmin_w + 128
// (both in [-128, 127] for every bit width), and the cross terms come back in the epilogue:
//     I = D + cwz[co] * SA + az * T[co]
//     D  = sum_k a_s w_s   (the int8 MFMA)       SA = sum_k a_s  (window sum, one more MFMA
//     cwz[co] = cw - z_w[co]                          against a 0/1 row: 1 on real k)
//     az = ca - z_a                              T[co] = sum_k w_s + K * cwz[co]
// The sums run over the K = Ci*R*S real taps.  A spatially padded tap holds a_s = z_a - ca,
// i.e. (q_a - z_a) = 0; padded channels and the K tail hold zero weights and a zero in the
// 0/1 row, so whatever the activation operand holds there contributes nothing.  The epilogue
// is evaluated in int64 (|I| can pass 2^31 at K = 65536), converted once (round to nearest
// even) and multiplied once: bit-reproducible from a host integer reference.
//
// Layouts.  Activation codes: NHWC int8 with C padded to Cp = 16*ceil(C/16) (padded channels
// 0), so every 16-byte K chunk of the implicit GEMM lies inside one (r, s) tap and is one
// aligned vector load.  Prepared weights: [Cop = 64*ceil(Co/64)][Kp = 64*ceil(R*S*Cp/64)]
// int8, k = (r*S + s)*Cp + ci, then the 0/1 row [Kp], then cwz[Cop] and T[Cop] (int32).
//
// K23 tile: 64 output pixels x 64 output channels x 64 k per workgroup of 4 waves.  Both
// operands are register-staged into one LDS buffer (rows of 64 B at an 80 B stride: the 16
// lanes of a ds_read_b128 group land on 16 distinct 16-B slots), the next k step's global
// loads fly during the MFMAs.  Wave w owns pixels 16w..16w+15 against all 64 channels:
// 4 x v_mfma_i32_16x16x64_i8 (weights as the A operand, so C rows are channels and C columns
// pixels: a store instruction writes 16 consecutive pixels per channel of the NCHW output)
// plus one for SA.  Both operand fragments use the same lane map (row / column l & 15,
// k chunk l >> 4), so the product does not depend on the k order inside a step.
//
// Column-scaled weights, W_hat = ((q_w - z_w[co]) * d1[co]) * (kcol[j] / L), j = (ci, r, s): the
// prepared operand is the centred integer m = (q_w - z_w[co]) * kcol[j] itself (|m| <= 127), so
// cwz = 0, I = D + az * T[co] with T[co] = sum m, and the CENTRED instantiation of K23 drops the
// 0/1 row and the SA MFMA; the caller's s[co] = fp32(fp32(delta_a * d1[co]) / fp32(L)).
//
// Per-(co, ci) scaled weights, W_hat = (q_w - z_w[co]) * fp32(base[co] * fp32(k[co, ci] / L)), are the
// same centred operand with the factor read per (co, ci) (QFactor, qinfer_prepare.h).  Where
// |m| leaves int8 the wide blob holds m = 128 h + l as two int8 planes (|m| <= 16319) and the WIDE
// instantiation of K23 sums D_h and D_l separately: I = 128 D_h + D_l + az * T[co].
#include <type_traits>

#include "ssq_common.h"
#include "qinfer_epi.h"
#include "qinfer_layout.h"
#include "qinfer_prepare.h"

namespace ssq {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- K21 activation encode
__global__ __launch_bounds__(kBlock) void act_encode_kernel(const float* __restrict__ x,
                                                            uint32_t npix, uint32_t HW, uint32_t C,
                                                            uint32_t Cp, FastDiv div_npix,
                                                            FastDiv div_hw, float d, float z,
                                                            float lo, float hi,
                                                            int8_t* __restrict__ out,
                                                            uint32_t* __restrict__ bad) {
  const uint32_t total = npix * (Cp / 16);
  const uint32_t stride = gridDim.x * blockDim.x;
  uint32_t nbad = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const uint32_t ch = fdiv(i, div_npix);
    const uint32_t pix = i - ch * npix;
    const uint32_t n = fdiv(pix, div_hw);
    const uint32_t p = pix - n * HW;
    const float* src = x + ((size_t)n * C + (size_t)ch * 16) * HW + p;
    union {
      i32x4 v;
      int8_t b[16];
    } o;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      int8_t code = 0;
      if (ch * 16 + j < C) {
        const float xv = src[(size_t)j * HW];
        float q = lo;   // NaN / +-inf: counted below, stored as qmin
        if (isfinite(xv)) {
          const float v = __fadd_rn(rintf(xv / d), z);
          q = v >= lo ? (v <= hi ? v : hi) : lo;
        }
        const bool ok = __float_as_uint(__fmul_rn(__fsub_rn(q, z), d)) == __float_as_uint(xv);
        nbad += ok ? 0u : 1u;
        code = (int8_t)((int)__fsub_rn(q, lo) - 128);
      }
      o.b[j] = code;
    }
    *(i32x4*)(out + (size_t)pix * Cp + (size_t)ch * 16) = o.v;
  }
  nbad = wave_sum(nbad);
  if ((threadIdx.x & (kWave - 1)) == 0 && nbad) atomicAdd(bad, nbad);
}

// ---------------------------------------------------------------- K22 weight prepare
// One workgroup per padded output channel, one more (blockIdx.x == Cop) for the 0/1 row.
// Plain: the operand is q - cw, cwz[co] = cw - z_w[co], T[co] = sum + K * cwz[co].
// SCALED, a weight W_hat = ((q - z_w[co]) * d[co]) * (k / L) with k the QFactor's entry of the
// element (a column scale or a per-(co, ci) scale, qinfer_prepare.h): the operand is the centred
// integer m = (q - z_w[co]) * k itself, so cwz = 0 and T[co] = sum m; the 0/1 row is written all
// the same, so every reader of the layout runs the blob as it stands.  WIDE (with SCALED): m leaves
// as its two digits, h into the first plane and l into the second (qinfer_layout.h).  *bad counts
// the real channels whose zero point breaks zp_is_code and, SCALED, the real elements qscaled()
// counts.
template <bool SCALED, bool WIDE = false>
__global__ __launch_bounds__(kBlock) void qweight_prepare_kernel(
    const uint8_t* __restrict__ packed, const float* __restrict__ zp, QFactor f, int bs, int qmin,
    uint32_t Co, uint32_t Ci, uint32_t RS, uint32_t Cp, uint32_t Kp, uint32_t Cop, FastDiv div_cp,
    int8_t* __restrict__ wp, int8_t* __restrict__ mask, int32_t* __restrict__ cwz,
    int32_t* __restrict__ tt, uint32_t* __restrict__ bad) {
  static_assert(SCALED || !WIDE, "the wide blob holds a centred operand");
  __shared__ int red[kBlock / kWave];
  const uint32_t co = blockIdx.x;
  if (co == Cop) {
    for (uint32_t k = threadIdx.x; k < Kp; k += blockDim.x) {
      const uint32_t tap = fdiv(k, div_cp);
      mask[k] = (tap < RS && k - tap * Cp < Ci) ? 1 : 0;
    }
    return;
  }
  const bool real = co < Co;
  const bool zok = !real || zp_is_code(zp[co], qmin);
  const int z = real && zok ? (int)zp[co] : qmin;
  int sum = 0;
  uint32_t nbad = 0;
  for (uint32_t k = threadIdx.x; k < Kp; k += blockDim.x) {
    const uint32_t tap = fdiv(k, div_cp);
    const uint32_t ci = k - tap * Cp;
    int v = 0;
    if (real && tap < RS && ci < Ci) {
      const size_t j = (size_t)ci * RS + tap;
      const int u = (int)packed_code(packed, (size_t)co * Ci * RS + j, bs);   // q - qmin
      if constexpr (SCALED) v = qscaled(u + qmin - z, qfactor_at(f, co, ci, tap), f.lim, nbad);
      else v = u - 128;   // q - cw, cw = qmin + 128
      sum += v;   // WIDE: |sum| <= 65536 * 16319 < 2^31
    }
    if constexpr (WIDE) {
      wp[(size_t)co * Kp + k] = (int8_t)qdigit_hi(v);
      wp[((size_t)Cop + co) * Kp + k] = (int8_t)qdigit_lo(v);
    } else {
      wp[(size_t)co * Kp + k] = (int8_t)v;
    }
  }
  sum = (int)wave_sum((uint32_t)sum);
  nbad = wave_sum(nbad);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red[threadIdx.x / kWave] = sum;
    if (nbad) atomicAdd(bad, nbad);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int i = 0; i < kBlock / kWave; ++i) total += red[i];
    if (!zok) atomicAdd(bad, 1u);
    const int c = (SCALED || !real) ? 0 : qmin + 128 - z;
    cwz[co] = c;
    tt[co] = total + (int)(Ci * RS) * c;   // a padded channel: 0
  }
}

// ---------------------------------------------------------------- K23 int8 implicit-GEMM conv
struct QConvGeo {
  uint32_t M, P, OW, H, W, Cp, Co, Kp, RS, S;
  int stride, pad, az, padv;
  FastDiv div_p, div_ow, div_cp, div_s;
};

// the epilogue's integer sum of channel co: I = D + cwz[co] * SA + az * T[co]; centred, cwz = 0
template <bool CENTRED>
__device__ __forceinline__ long long qconv_sum(int d, const int32_t* __restrict__ cwz,
                                               long long sa, int az,
                                               const int32_t* __restrict__ tt, uint32_t co) {
  if constexpr (CENTRED) return (long long)d + (long long)az * (long long)tt[co];
  else return (long long)d + (long long)cwz[co] * sa + (long long)az * (long long)tt[co];
}

// the wide operand's sum: I = 128 D_h + D_l + az * T[co], each D an exact int32 digit sum
__device__ __forceinline__ long long qconv_sum_wide(int dh, int dl, int az,
                                                    const int32_t* __restrict__ tt, uint32_t co) {
  return 128ll * (long long)dh + (long long)dl + (long long)az * (long long)tt[co];
}

// K23's choice between the two: `d` is D, or, WIDE, D_h with `dl` = D_l
template <bool CENTRED, bool WIDE>
__device__ __forceinline__ long long qconv_sum_of(int d, int dl, const int32_t* __restrict__ cwz,
                                                  long long sa, int az,
                                                  const int32_t* __restrict__ tt, uint32_t co) {
  if constexpr (WIDE) return qconv_sum_wide(d, dl, az, tt, co);
  else return qconv_sum<CENTRED>(d, cwz, sa, az, tt, co);
}

// CODES: the code-emitting epilogue (qinfer_epi.h) instead of the fp32 NCHW store; `y` is then
// the QEpi.  The 64 px x 64 ch code tile is transposed through the (then free) activation
// tile and leaves as one 16-B chunk of a pixel's channels per thread.
// RES (with CODES): a block tail's residual, added where K13 adds it (qepi_code<true>).  1: fp32
// NCHW, four loads per fragment, each 16 consecutive pixels of one channel plane (the fp32
// form's store pattern); 2: int8 codes in the output's own layout, one aligned dword (the
// lane's 4 channels of its pixel) per fragment.  `y` is then the QEpiRes.  The loads are issued
// right after the K loop, so the cwz / T correction arithmetic covers their latency.
// CENTRED: the blob holds a centred operand (ssq_qweight_prepare_colscale: cwz = 0), so SA is
// not needed: no 0/1 row load, LDS store or fragment read, no SA MFMA (four per k step, not
// five) and I = D + az * T[co].  `mask` and `cwz` are not read.
// PARTIAL (qconv_i8_partial_kernel<CENTRED>, the split-K form's first kernel): a third grid
// dimension of Z slices; slice z walks the k steps [z nk / Z, (z + 1) nk / Z) with the staging,
// LDS layout, fragment map and MFMAs of the whole walk, and instead of an epilogue stores its raw
// int32 accumulators to the QPartial `y`.  Every element of D[Z][Co][M] and (not CENTRED)
// SA[Z][M] is written exactly once, by one thread, and nothing else: no memset, no counter.
// WIDE (implies CENTRED; not with PARTIAL): the blob holds a centred operand m = 128 h + l in two
// int8 digit planes (qinfer_layout.h).  The tile and lane maps stay; per k step a thread stages
// one activation chunk and one chunk of each plane (lB holds two 64-row tiles, h then l), a wave
// reads one activation fragment and eight weight fragments and issues eight MFMAs into two sets
// of accumulators, D_h = sum a_s h and D_l = sum a_s l (|D| <= 65536 * 128 * 127 < 2^30 each), and
// the epilogue takes I = 128 D_h + D_l + az * T[co] in int64 (qconv_sum_wide) and is otherwise
// the one above.
struct QPartial {
  int32_t* D;    // [Z][Co][M]: slice z's sum of a_s w_s, the fp32 form's store pattern
  int32_t* SA;   // [Z][M]: slice z's window sum (not CENTRED)
};

template <bool CODES, int RES = 0, bool CENTRED = false, bool PARTIAL = false, bool WIDE = false>
__global__ __launch_bounds__(kBlock) void qconv_i8_kernel(
    const int8_t* __restrict__ act, const int8_t* __restrict__ wp, const int8_t* __restrict__ mask,
    const int32_t* __restrict__ cwz, const int32_t* __restrict__ tt,
    const float* __restrict__ scale, QConvGeo g,
    typename std::conditional<
        PARTIAL, QPartial,
        typename std::conditional<CODES, typename std::conditional<RES != 0, QEpiRes, QEpi>::type,
                                  float* __restrict__>::type>::type y) {
  static_assert(CODES || RES == 0, "a residual goes with the code-emitting epilogue");
  static_assert(!PARTIAL || (!CODES && RES == 0), "a partial walk has no epilogue");
  static_assert(!WIDE || (CENTRED && !PARTIAL), "the wide operand is centred and has no split form");
  __shared__ __attribute__((aligned(16))) int8_t lA[kQT * kQRow];
  __shared__ __attribute__((aligned(16))) int8_t lB[(WIDE ? 2 * kQT : kQT + 1) * kQRow];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & (kWave - 1), wave = tid / kWave;
  const uint32_t fr = lane & 15, fq = lane >> 4;

  // staging role: one 16-byte chunk of each operand tile per thread
  const uint32_t srow = tid >> 2, sc = tid & 3;
  const uint32_t gm = blockIdx.x * kQT + srow;
  const bool mval = gm < g.M;
  const uint32_t gmc = mval ? gm : 0u;
  const uint32_t sn = fdiv(gmc, g.div_p);
  const uint32_t sp = gmc - sn * g.P;
  const uint32_t soh = fdiv(sp, g.div_ow);
  const uint32_t sow = sp - soh * g.OW;
  const int ih0 = (int)soh * g.stride - g.pad, iw0 = (int)sow * g.stride - g.pad;
  const int8_t* abase = act + (size_t)sn * g.H * g.W * g.Cp;
  const int8_t* wrow = wp + (size_t)(blockIdx.y * kQT + srow) * g.Kp + sc * 16;
  const int pv = (g.padv & 0xff) * 0x01010101;
  const i32x4 padfill = {pv, pv, pv, pv};

  auto load_a = [&](uint32_t kt) -> i32x4 {
    const uint32_t k = kt * kQT + sc * 16;
    const uint32_t tap = fdiv(k, g.div_cp);
    const uint32_t ci0 = k - tap * g.Cp;
    const uint32_t r = fdiv(tap, g.div_s);
    const uint32_t s = tap - r * g.S;
    const int ih = ih0 + (int)r, iw = iw0 + (int)s;
    if (mval && tap < g.RS && (uint32_t)ih < g.H && (uint32_t)iw < g.W)
      return *(const i32x4*)(abase + ((size_t)ih * g.W + (size_t)iw) * g.Cp + ci0);
    return padfill;
  };

  const uint32_t nk = g.Kp / kQT;
  uint32_t kt0 = 0, kt1 = nk;   // this workgroup's k steps: all of them, or slice blockIdx.z's
  if constexpr (PARTIAL) {
    kt0 = blockIdx.z * nk / gridDim.z;
    kt1 = (blockIdx.z + 1) * nk / gridDim.z;
  }

  i32x4 ra = load_a(kt0);
  i32x4 rb = *(const i32x4*)(wrow + (size_t)kt0 * kQT);
  // WIDE: the l plane lies Cop * Kp bytes behind the h plane, Cop = 64 gridDim.y
  const size_t plane = WIDE ? (size_t)gridDim.y * kQT * g.Kp : 0;
  i32x4 rl = {0, 0, 0, 0};
  if constexpr (WIDE) rl = *(const i32x4*)(wrow + plane + (size_t)kt0 * kQT);
  i32x4 rm = {0, 0, 0, 0};
  if constexpr (!CENTRED) {
    if (tid < 4) rm = *(const i32x4*)(mask + (size_t)kt0 * kQT + tid * 16);
  }

  i32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = i32x4{0, 0, 0, 0};
  i32x4 accs = {0, 0, 0, 0};
  i32x4 accl[WIDE ? 4 : 1];   // WIDE: acc is D_h, accl D_l
#pragma unroll
  for (int j = 0; j < (WIDE ? 4 : 1); ++j) accl[j] = i32x4{0, 0, 0, 0};

  for (uint32_t kt = kt0; kt < kt1; ++kt) {
    __syncthreads();   // the previous step's fragment reads are done
    *(i32x4*)(lA + srow * kQRow + sc * 16) = ra;
    *(i32x4*)(lB + srow * kQRow + sc * 16) = rb;
    if constexpr (WIDE) *(i32x4*)(lB + (kQT + srow) * kQRow + sc * 16) = rl;
    if constexpr (!CENTRED) {
      if (tid < 4) *(i32x4*)(lB + kQT * kQRow + tid * 16) = rm;
    }
    __syncthreads();
    if (kt + 1 < kt1) {
      ra = load_a(kt + 1);
      rb = *(const i32x4*)(wrow + (size_t)(kt + 1) * kQT);
      if constexpr (WIDE) rl = *(const i32x4*)(wrow + plane + (size_t)(kt + 1) * kQT);
      if constexpr (!CENTRED) {
        if (tid < 4) rm = *(const i32x4*)(mask + (size_t)(kt + 1) * kQT + tid * 16);
      }
    }
    const i32x4 af = *(const i32x4*)(lA + (wave * 16 + fr) * kQRow + fq * 16);
    if constexpr (!CENTRED) {
      const i32x4 mf = *(const i32x4*)(lB + kQT * kQRow + fq * 16);
      accs = __builtin_amdgcn_mfma_i32_16x16x64_i8(mf, af, accs, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const i32x4 wf = *(const i32x4*)(lB + (j * 16 + fr) * kQRow + fq * 16);
      acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, af, acc[j], 0, 0, 0);
    }
    if constexpr (WIDE) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const i32x4 wf = *(const i32x4*)(lB + (kQT + j * 16 + fr) * kQRow + fq * 16);
        accl[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, af, accl[j], 0, 0, 0);
      }
    }
  }

  // C/D map: column (pixel) = lane & 15, row (channel) = 4 * (lane >> 4) + reg
  const uint32_t pixel = blockIdx.x * kQT + wave * 16 + fr;
  const long long sa = (long long)accs[0];
  if constexpr (PARTIAL) {
    if (pixel >= g.M) return;
    int32_t* dz = y.D + (size_t)blockIdx.z * g.Co * g.M + pixel;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t co = blockIdx.y * kQT + j * 16 + fq * 4 + r;
        if (co < g.Co) dz[(size_t)co * g.M] = acc[j][r];
      }
    }
    if constexpr (!CENTRED) {
      // every C row of the 0/1-row product holds the window sum: row 0 (register 0 of the
      // fq == 0 lanes) of the first channel tile's workgroup writes it
      if (blockIdx.y == 0 && fq == 0) y.SA[(size_t)blockIdx.z * g.M + pixel] = accs[0];
    }
  } else if constexpr (CODES) {
    const QEpi& e = qepi_of(y);
    const bool pval = pixel < g.M;
    uint32_t nbad = 0;
    float rf[RES == 1 ? 16 : 1];
    int rw[RES == 2 ? 4 : 1];
    if constexpr (RES == 1) {
      const uint32_t pc = pval ? pixel : 0u;
      const uint32_t n = fdiv(pc, g.div_p);
      const float* rp = y.r.f32 + (size_t)n * g.Co * g.P + (pc - n * g.P);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t co = blockIdx.y * kQT + j * 16 + fq * 4 + r;
          rf[j * 4 + r] = (pval && co < g.Co) ? rp[(size_t)co * g.P] : 0.0f;
        }
      }
    } else if constexpr (RES == 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // co0 is a multiple of 4 below Co <= Cpo (a multiple of 16): the dword lies in the row
        const uint32_t co0 = blockIdx.y * kQT + j * 16 + fq * 4;
        rw[j] = (pval && co0 < g.Co) ? *(const int*)(y.r.codes + (size_t)pixel * e.Cpo + co0) : 0;
      }
    }
    __syncthreads();   // the last step's fragment reads are done: lA is free
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int c[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t co = blockIdx.y * kQT + j * 16 + fq * 4 + r;
        c[r] = 0;
        if (pval && co < g.Co) {
          const long long I = qconv_sum_of<CENTRED, WIDE>(acc[j][r], accl[WIDE ? j : 0][r], cwz, sa,
                                                          g.az, tt, co);
          if constexpr (RES == 1) {
            c[r] = qepi_code<true>((float)I, co, scale, e, nbad, rf[j * 4 + r]);
          } else if constexpr (RES == 2) {
            const int code = (int)(int8_t)((uint32_t)rw[j] >> (8 * r));
            c[r] = qepi_code<true>((float)I, co, scale, e, nbad, qres_decode(code, y.r));
          } else {
            c[r] = qepi_code((float)I, co, scale, e, nbad);
          }
        }
      }
      *(int*)(lA + (wave * 16 + fr) * kQRow + j * 16 + fq * 4) = qepi_pack4(c[0], c[1], c[2], c[3]);
    }
    __syncthreads();
    // the staging role's map again: thread (row, chunk) stores channels [16 chunk, 16 chunk + 16)
    // of pixel row.  Recomputed from a thread id the compiler cannot tie to the one above, or
    // srow / sc / gm / mval stay live across the K loop: 62 VGPRs and 5 waves per SIMD, not 56 and 6
    uint32_t t2 = tid;
    asm volatile("" : "+v"(t2));
    const uint32_t row = t2 >> 2, chunk = t2 & 3;
    const uint32_t gpix = blockIdx.x * kQT + row, ch0 = blockIdx.y * kQT + chunk * 16;
    if (gpix < g.M && ch0 < e.Cpo)
      *(i32x4*)(e.out + (size_t)gpix * e.Cpo + ch0) = *(const i32x4*)(lA + row * kQRow + chunk * 16);
    qepi_count(nbad, e.bad);
  } else {
    if (pixel >= g.M) return;
    const uint32_t n = fdiv(pixel, g.div_p);
    const uint32_t p = pixel - n * g.P;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t co = blockIdx.y * kQT + j * 16 + fq * 4 + r;
        if (co < g.Co) {
          const long long I = qconv_sum_of<CENTRED, WIDE>(acc[j][r], accl[WIDE ? j : 0][r], cwz, sa,
                                                          g.az, tt, co);
          y[((size_t)n * g.Co + co) * g.P + p] = __fmul_rn((float)I, scale[co]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- K23 split along K
// The integer sum is exact and associative, so Z workgroups may each walk a slice of the k steps
// and a second kernel add the slices: bit-identical to the whole walk, and with each element of
// the workspace written once by one thread, identical from run to run.  No atomics.
template <bool CENTRED>
constexpr auto qconv_i8_partial_kernel = qconv_i8_kernel<false, 0, CENTRED, true>;

// slices summed: D in int32 (|whole-K sum| <= 65536 * 128 * 128 = 2^30, as in one walk), SA in int64
template <bool CENTRED>
__device__ __forceinline__ long long qsplit_sa(const int32_t* __restrict__ SA, uint32_t Z,
                                               uint32_t M, uint32_t pixel) {
  long long sa = 0;
  if constexpr (!CENTRED) {
    for (uint32_t z = 0; z < Z; ++z) sa += (long long)SA[(size_t)z * M + pixel];
  }
  return sa;
}
__device__ __forceinline__ int qsplit_d(const int32_t* __restrict__ D, uint32_t Z, size_t slice,
                                        size_t at) {
  int d = 0;
  for (uint32_t z = 0; z < Z; ++z) d += D[(size_t)z * slice + at];
  return d;
}

// The finish: K23's own epilogue functions on the summed slices, so the bits are K23's.
// fp32 form: one thread per (co, pixel), coalesced along pixels, NCHW store.  Code forms: one
// thread per (pixel, 16-channel chunk), K25's pattern: a wave reads 64 consecutive pixels of a
// channel row per load and each thread stores its pixel's chunk as one 16-B word; channels at or
// past Co inside a chunk are 0.  RES as in K23: 1 loads fp32 NCHW along pixels, 2 one 16-B word
// at the output's own address.  Threads past the end are predicated, not returned: qepi_count is
// a wave reduction.
template <bool CODES, int RES = 0, bool CENTRED = false>
__global__ __launch_bounds__(kBlock) void qconv_i8_finish_kernel(
    const int32_t* __restrict__ D, const int32_t* __restrict__ SA, uint32_t Z,
    const int32_t* __restrict__ cwz, const int32_t* __restrict__ tt,
    const float* __restrict__ scale, QConvGeo g, FastDiv div_m,
    typename std::conditional<CODES, typename std::conditional<RES != 0, QEpiRes, QEpi>::type,
                              float* __restrict__>::type y) {
  static_assert(CODES || RES == 0, "a residual goes with the code-emitting epilogue");
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const size_t slice = (size_t)g.Co * g.M;
  if constexpr (CODES) {
    const QEpi& e = qepi_of(y);
    const bool live = i < g.M * (e.Cpo / 16);
    const uint32_t ic = live ? i : 0u;
    const uint32_t chunk = fdiv(ic, div_m);
    const uint32_t pixel = ic - chunk * g.M;
    uint32_t nbad = 0;
    union {
      i32x4 v;
      int8_t b[16];
    } o, rc;
    const float* rp = nullptr;
    if constexpr (RES == 1) {
      const uint32_t n = fdiv(pixel, g.div_p);
      rp = y.r.f32 + (size_t)n * g.Co * g.P + (pixel - n * g.P);
    } else if constexpr (RES == 2) {
      rc.v = *(const i32x4*)(y.r.codes + (size_t)pixel * e.Cpo + chunk * 16);
    }
    const long long sa = qsplit_sa<CENTRED>(SA, Z, g.M, pixel);
    // Straight-line code: a channel at or past Co (and every channel of a thread past the end)
    // computes on its chunk's first channel, which is a real one, and is discarded by a select,
    // so the 16 rows of a slice are 16 independent loads in flight and so are the per-channel
    // vectors; with the work under a branch per channel every load is waited for on its own.
    const uint32_t co0 = chunk * 16;
    const uint32_t real = !live ? 0u : (g.Co - co0 < 16u ? g.Co - co0 : 16u);
    const int32_t* dp = D + (size_t)co0 * g.M + pixel;
    int d[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) d[j] = 0;
    for (uint32_t z = 0; z < Z; ++z) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        d[j] += dp[(size_t)z * slice + (size_t)((uint32_t)j < real ? j : 0) * g.M];
    }
    // `el`: the epilogue with its optional vectors known present or absent (the launch-wide
    // tests of qepi_code_y hoisted out of the 16 channels), so their loads are issued together
    auto emit = [&](const QEpi& el) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool on = (uint32_t)j < real;
        const uint32_t co = on ? co0 + j : co0;
        const long long I = qconv_sum<CENTRED>(d[j], cwz, sa, g.az, tt, co);
        uint32_t nb = 0;
        int c;
        if constexpr (RES == 1) {
          c = qepi_code<true>((float)I, co, scale, el, nb, rp[(size_t)co * g.P]);
        } else if constexpr (RES == 2) {
          c = qepi_code<true>((float)I, co, scale, el, nb, qres_decode((int)rc.b[j], y.r));
        } else {
          c = qepi_code((float)I, co, scale, el, nb);
        }
        nbad += on ? nb : 0u;
        o.b[j] = (int8_t)(on ? c : 0);
      }
    };
    QEpi el = e;
    if (e.bias && e.gamma) {
      __builtin_assume(el.bias != nullptr && el.gamma != nullptr);
      emit(el);
    } else if (e.bias) {
      __builtin_assume(el.bias != nullptr);
      el.gamma = el.phi = nullptr;
      emit(el);
    } else if (e.gamma) {
      __builtin_assume(el.gamma != nullptr);
      el.bias = nullptr;
      emit(el);
    } else {
      el.bias = el.gamma = el.phi = nullptr;
      emit(el);
    }
    if (live) *(i32x4*)(e.out + (size_t)pixel * e.Cpo + chunk * 16) = o.v;
    qepi_count(nbad, e.bad);
  } else {
    if (i >= g.Co * g.M) return;
    const uint32_t co = fdiv(i, div_m);
    const uint32_t pixel = i - co * g.M;
    const uint32_t n = fdiv(pixel, g.div_p);
    const uint32_t p = pixel - n * g.P;
    const long long sa = qsplit_sa<CENTRED>(SA, Z, g.M, pixel);
    const long long I = qconv_sum<CENTRED>(qsplit_d(D, Z, slice, i), cwz, sa, g.az, tt, co);
    y[((size_t)n * g.Co + co) * g.P + p] = __fmul_rn((float)I, scale[co]);
  }
}

// ---------------------------------------------------------------- K21's inverse
// NHWC codes -> fp32 NCHW (q - z) * d: a carried tensor handed to an fp32 consumer.  K21's
// thread map: one 16-B chunk of a pixel per thread, 16 stores each coalesced across pixels.
__global__ __launch_bounds__(kBlock) void act_decode_kernel(const int8_t* __restrict__ codes,
                                                            uint32_t npix, uint32_t HW, uint32_t C,
                                                            uint32_t Cp, FastDiv div_npix,
                                                            FastDiv div_hw, float d, float z,
                                                            float lo, float* __restrict__ x) {
  const uint32_t total = npix * (Cp / 16);
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const uint32_t ch = fdiv(i, div_npix);
    const uint32_t pix = i - ch * npix;
    const uint32_t n = fdiv(pix, div_hw);
    const uint32_t p = pix - n * HW;
    union {
      i32x4 v;
      int8_t b[16];
    } in;
    in.v = *(const i32x4*)(codes + (size_t)pix * Cp + (size_t)ch * 16);
    float* dst = x + ((size_t)n * C + (size_t)ch * 16) * HW + p;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (ch * 16 + j < C) {
        const float q = __fadd_rn((float)((int)in.b[j] + 128), lo);   // exact: |q| <= 255
        dst[(size_t)j * HW] = __fmul_rn(__fsub_rn(q, z), d);
      }
    }
  }
}

static int qgeo_ok(const char* what, int64_t Co, int64_t Ci, int64_t R, int64_t S,
                   int planes = 1) {
  SSQ_REQUIRE(Co >= 1 && Ci >= 1 && R >= 1 && S >= 1 && R <= 7 && S <= 7, SSQ_E_ARG,
              "%s: bad geometry (Co, Ci >= 1; R, S in [1, 7])", what);
  SSQ_REQUIRE(Ci * R * S <= kQMaxK, SSQ_E_ARG,
              "%s: K = Ci*R*S = %lld exceeds 65536 (int32 accumulator range)", what,
              (long long)(Ci * R * S));
  const QLayout L = qlayout(Co, Ci, R, S, planes);
  SSQ_REQUIRE(L.off_mask < (1ull << 31), SSQ_E_ARG, "%s: prepared weights exceed 2^31 bytes", what);
  return SSQ_OK;
}

}  // namespace ssq

using namespace ssq;

extern "C" int64_t ssq_qinfer_cpad(int64_t C) { return C >= 1 ? rup(C, 16) : 0; }

extern "C" size_t ssq_qweight_prepared_bytes(int64_t Co, int64_t Ci, int64_t R, int64_t S) {
  if (Co < 1 || Ci < 1 || R < 1 || S < 1) return 0;
  return qlayout(Co, Ci, R, S).bytes;
}

extern "C" int ssq_act_encode(const float* x, int64_t Nb, int64_t C, int64_t H, int64_t W,
                              float delta, float zero_point, int qmin, int qmax, int8_t* codes,
                              uint32_t* bad, ssq_stream_t stream) {
  SSQ_REQUIRE(x && codes && bad, SSQ_E_ARG, "ssq_act_encode: null pointer");
  SSQ_REQUIRE(Nb >= 1 && C >= 1 && H >= 1 && W >= 1, SSQ_E_ARG, "ssq_act_encode: bad geometry");
  const int rc = qquant_ok("ssq_act_encode", "", &delta, zero_point, qmin, qmax);
  if (rc) return rc;
  const int64_t Cp = rup(C, 16);
  SSQ_REQUIRE(Nb * H * W * Cp < (1ll << 31), SSQ_E_ARG,
              "ssq_act_encode: tensor exceeds 2^31 elements");
  const uint32_t npix = (uint32_t)(Nb * H * W), HW = (uint32_t)(H * W);
  const dim3 grid(grid_for((int64_t)npix * (Cp / 16), kBlock, 8192));
  hipLaunchKernelGGL(act_encode_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, x, npix, HW,
                     (uint32_t)C, (uint32_t)Cp, make_fastdiv(npix), make_fastdiv(HW), delta,
                     zero_point, (float)qmin, (float)qmax, codes, bad);
  return check_launch("ssq_act_encode");
}

// kfac: the integer factors of a scaled weight (the SCALED kernels), or null: one per (ci, r, s)
// column, or, per_ci, one per (co, ci); wide: the two-digit blob, factors and |m| up to kQWideMax
static int qweight_prepare_launch(const char* me, bool scaled, bool per_ci, bool wide,
                                  const void* packed, const float* zp, const int32_t* kfac,
                                  int64_t Co, int64_t Ci, int64_t R, int64_t S, int n_bits,
                                  int qmin, void* prepared, uint32_t* bad, ssq_stream_t stream) {
  SSQ_REQUIRE(packed && zp && (kfac || !scaled) && prepared && bad, SSQ_E_ARG,
              "%s: null pointer", me);
  int rc = qrange_ok(me, n_bits, qmin);
  if (rc) return rc;
  rc = qgeo_ok(me, Co, Ci, R, S, wide ? 2 : 1);
  if (rc) return rc;
  const QLayout L = qlayout(Co, Ci, R, S, wide ? 2 : 1);
  int8_t* base = (int8_t*)prepared;
  const QFactor f = qfactor(kfac, per_ci, (uint32_t)Ci, (uint32_t)(R * S), wide ? kQWideMax : 127);
  auto* kernel = wide ? qweight_prepare_kernel<true, true>
                      : (scaled ? qweight_prepare_kernel<true> : qweight_prepare_kernel<false>);
  hipLaunchKernelGGL(kernel, dim3((uint32_t)L.Cop + 1), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint8_t*)packed, zp, f, packed_bits(n_bits), qmin, (uint32_t)Co,
                     (uint32_t)Ci, (uint32_t)(R * S), (uint32_t)L.Cp, (uint32_t)L.Kp,
                     (uint32_t)L.Cop, make_fastdiv((uint32_t)L.Cp), base, base + L.off_mask,
                     (int32_t*)(base + L.off_cwz), (int32_t*)(base + L.off_t), bad);
  return check_launch(me);
}

extern "C" int ssq_qweight_prepare(const void* packed, const float* zp, int64_t Co, int64_t Ci,
                                   int64_t R, int64_t S, int n_bits, int qmin, void* prepared,
                                   uint32_t* bad, ssq_stream_t stream) {
  return qweight_prepare_launch("ssq_qweight_prepare", false, false, false, packed, zp, nullptr, Co,
                                Ci, R, S, n_bits, qmin, prepared, bad, stream);
}

extern "C" int ssq_qweight_prepare_colscale(const void* packed, const float* zp,
                                            const int32_t* kcol, int64_t Co, int64_t Ci, int64_t R,
                                            int64_t S, int n_bits, int qmin, void* prepared,
                                            uint32_t* bad, ssq_stream_t stream) {
  return qweight_prepare_launch("ssq_qweight_prepare_colscale", true, false, false, packed, zp,
                                kcol, Co, Ci, R, S, n_bits, qmin, prepared, bad, stream);
}

extern "C" int ssq_qweight_prepare_perci(const void* packed, const float* zp, const int32_t* kfac,
                                         int64_t Co, int64_t Ci, int64_t R, int64_t S, int n_bits,
                                         int qmin, void* prepared, uint32_t* bad,
                                         ssq_stream_t stream) {
  return qweight_prepare_launch("ssq_qweight_prepare_perci", true, true, false, packed, zp, kfac,
                                Co, Ci, R, S, n_bits, qmin, prepared, bad, stream);
}

extern "C" size_t ssq_qweight_prepared_bytes_wide(int64_t Co, int64_t Ci, int64_t R, int64_t S) {
  if (Co < 1 || Ci < 1 || R < 1 || S < 1) return 0;
  return qlayout(Co, Ci, R, S, 2).bytes;
}

extern "C" int ssq_qweight_prepare_wide(const void* packed, const float* zp, const int32_t* kfac,
                                        int per_ci, int64_t Co, int64_t Ci, int64_t R, int64_t S,
                                        int n_bits, int qmin, void* prepared, uint32_t* bad,
                                        ssq_stream_t stream) {
  return qweight_prepare_launch("ssq_qweight_prepare_wide", true, per_ci != 0, true, packed, zp,
                                kfac, Co, Ci, R, S, n_bits, qmin, prepared, bad, stream);
}

// One form of K23 on a blob: CENTRED for a centred one (ssq_qweight_prepare_colscale), which is
// bit-identical to the plain instantiation there, one MFMA per k step less.
// `sp`: the split-K form (the ssq_qconv_i8_*splitk_* entry points): the partial kernel over
// sp->splits slices into the caller's workspace, then the finish kernel of the same form.
struct QSplit {
  int splits;
  void* ws;
  size_t ws_bytes;
};
constexpr int kQMaxSplits = 16;

// D[Z][Co][M] then, unless centred, SA[Z][M], int32
static size_t qsplit_ws_bytes(int64_t M, int64_t Co, int64_t Z, bool centred) {
  return (size_t)Z * (size_t)(Co + (centred ? 0 : 1)) * (size_t)M * 4;
}

template <bool CENTRED, bool WIDE = false>
static void qconv_i8_run(dim3 grid, ssq_stream_t stream, const int8_t* codes, const int8_t* base,
                         const QLayout& L, const float* scale, const QConvGeo& g, float* y,
                         const QEpi* epi, const QRes* res, const QSplit* sp) {
  const int8_t* mask = base + L.off_mask;
  const int32_t* cwz = (const int32_t*)(base + L.off_cwz);
  const int32_t* tt = (const int32_t*)(base + L.off_t);
  auto run = [&](auto* kernel, auto out) {
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, codes, base, mask, cwz,
                       tt, scale, g, out);
  };
  if constexpr (WIDE) {
    if (!epi) run(qconv_i8_kernel<false, 0, true, false, true>, y);
    else if (!res) run(qconv_i8_kernel<true, 0, true, false, true>, *epi);
    else if (res->f32) run(qconv_i8_kernel<true, 1, true, false, true>, QEpiRes{*epi, *res});
    else run(qconv_i8_kernel<true, 2, true, false, true>, QEpiRes{*epi, *res});
    return;
  }
  if (sp) {
    const uint32_t Z = (uint32_t)sp->splits;
    const QPartial part = {(int32_t*)sp->ws, (int32_t*)sp->ws + (size_t)Z * g.Co * g.M};
    grid.z = Z;
    run(qconv_i8_partial_kernel<CENTRED>, part);
    const uint32_t items = epi ? g.M * (epi->Cpo / 16) : g.Co * g.M;
    auto finish = [&](auto* kernel, auto out) {
      hipLaunchKernelGGL(kernel, dim3((items + kBlock - 1) / kBlock), dim3(kBlock), 0,
                         (hipStream_t)stream, (const int32_t*)part.D, (const int32_t*)part.SA, Z,
                         cwz, tt, scale, g, make_fastdiv(g.M), out);
    };
    if (!epi) finish(qconv_i8_finish_kernel<false, 0, CENTRED>, y);
    else if (!res) finish(qconv_i8_finish_kernel<true, 0, CENTRED>, *epi);
    else if (res->f32) finish(qconv_i8_finish_kernel<true, 1, CENTRED>, QEpiRes{*epi, *res});
    else finish(qconv_i8_finish_kernel<true, 2, CENTRED>, QEpiRes{*epi, *res});
    return;
  }
  if (!epi) run(qconv_i8_kernel<false, 0, CENTRED>, y);
  else if (!res) run(qconv_i8_kernel<true, 0, CENTRED>, *epi);
  else if (res->f32) run(qconv_i8_kernel<true, 1, CENTRED>, QEpiRes{*epi, *res});
  else run(qconv_i8_kernel<true, 2, CENTRED>, QEpiRes{*epi, *res});
}

// The arguments every dense conv entry point hands to the launch as they came
struct QConvIn {
  const int8_t* codes;
  const void* prepared;
  const float* scale;
  int64_t Nb, Ci, H, W, Co, R, S, stride, pad, groups;
  float act_zero_point;
  int act_qmin, act_qmax;
};

// y: the fp32 output (ssq_qconv_i8_fwd) or null with `epi` set (ssq_qconv_i8_codes_fwd); `res`
// with `epi`: the tail's residual (ssq_qconv_i8_codes_res_fwd); centred: the *_centred_* forms;
// `sp`: the split-K forms; wide: the *_wide_* forms on the two-digit blob (centred, never split)
static int qconv_i8_launch(const char* me, bool centred, const QConvIn& a, float* y, QEpi* epi,
                           const QRes* res, ssq_stream_t stream, const QSplit* sp = nullptr,
                           bool wide = false) {
  SSQ_REQUIRE(a.codes && a.prepared && a.scale && (y || epi), SSQ_E_ARG, "%s: null pointer", me);
  SSQ_REQUIRE(a.groups == 1, SSQ_E_ARG, "%s: groups = %lld (only groups == 1)", me,
              (long long)a.groups);
  const int64_t Nb = a.Nb, H = a.H, W = a.W, Co = a.Co, R = a.R, S = a.S, pad = a.pad;
  SSQ_REQUIRE(!wide || (centred && !sp), SSQ_E_ARG, "%s: the wide blob has no split-K form", me);
  int rc = qgeo_ok(me, Co, a.Ci, R, S, wide ? 2 : 1);
  if (rc) return rc;
  SSQ_REQUIRE(Nb >= 1 && H >= 1 && W >= 1 && a.stride >= 1 && pad >= 0 &&
                  H + 2 * pad >= R && W + 2 * pad >= S,
              SSQ_E_ARG, "%s: bad geometry", me);
  rc = qquant_ok(me, "activation ", nullptr, a.act_zero_point, a.act_qmin, a.act_qmax);
  if (rc) return rc;
  const QLayout L = qlayout(Co, a.Ci, R, S, wide ? 2 : 1);
  const int64_t OH = (H + 2 * pad - R) / a.stride + 1, OW = (W + 2 * pad - S) / a.stride + 1;
  SSQ_REQUIRE(Nb * H * W * L.Cp < (1ll << 31) && Nb * OH * OW * Co < (1ll << 31), SSQ_E_ARG,
              "%s: tensor exceeds 2^31 elements", me);
  QConvGeo g;
  g.M = (uint32_t)(Nb * OH * OW);
  g.P = (uint32_t)(OH * OW);
  g.OW = (uint32_t)OW;
  g.H = (uint32_t)H;
  g.W = (uint32_t)W;
  g.Cp = (uint32_t)L.Cp;
  g.Co = (uint32_t)Co;
  g.Kp = (uint32_t)L.Kp;
  g.RS = (uint32_t)(R * S);
  g.S = (uint32_t)S;
  g.stride = (int)a.stride;
  g.pad = (int)pad;
  const int ca = a.act_qmin + 128, za = (int)a.act_zero_point;
  g.az = ca - za;
  g.padv = za - ca;   // a padded tap: (q_a - z_a) = 0
  g.div_p = make_fastdiv(g.P);
  g.div_ow = make_fastdiv(g.OW);
  g.div_cp = make_fastdiv(g.Cp);
  g.div_s = make_fastdiv(g.S);
  if (epi) {
    epi->Cpo = (uint32_t)rup(Co, 16);
    SSQ_REQUIRE(Nb * OH * OW * (int64_t)epi->Cpo < (1ll << 31), SSQ_E_ARG,
                "%s: tensor exceeds 2^31 elements", me);
  }
  if (sp) {
    SSQ_REQUIRE(sp->splits >= 2 && sp->splits <= kQMaxSplits && sp->splits <= L.Kp / kQT,
                SSQ_E_ARG, "%s: splits = %d not in [2, min(%d, the %lld k steps)]", me, sp->splits,
                kQMaxSplits, (long long)(L.Kp / kQT));
    SSQ_REQUIRE(sp->ws && sp->ws_bytes >= qsplit_ws_bytes(g.M, Co, sp->splits, centred),
                SSQ_E_ARG, "%s: workspace null or smaller than %zu bytes", me,
                qsplit_ws_bytes(g.M, Co, sp->splits, centred));
  }
  const dim3 grid((g.M + kQT - 1) / kQT, (uint32_t)(L.Cop / kQT));
  const int8_t* base = (const int8_t*)a.prepared;
  if (wide) qconv_i8_run<true, true>(grid, stream, a.codes, base, L, a.scale, g, y, epi, res, nullptr);
  else if (centred) qconv_i8_run<true>(grid, stream, a.codes, base, L, a.scale, g, y, epi, res, sp);
  else qconv_i8_run<false>(grid, stream, a.codes, base, L, a.scale, g, y, epi, res, sp);
  return check_launch(me);
}

// The six dense entry points: {plain, centred blob} x {fp32 out, codes out, codes out + residual},
// each its own checks (y; the epilogue; the residual, in that order) and one launch.
extern "C" int ssq_qconv_i8_fwd(const int8_t* codes, const void* prepared, const float* scale,
                                int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t groups,
                                float act_zero_point, int act_qmin, int act_qmax, float* y,
                                ssq_stream_t stream) {
  SSQ_REQUIRE(y, SSQ_E_ARG, "ssq_qconv_i8_fwd: null pointer");
  return qconv_i8_launch("ssq_qconv_i8_fwd", false,
                         {codes, prepared, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups,
                          act_zero_point, act_qmin, act_qmax},
                         y, nullptr, nullptr, stream);
}

extern "C" int ssq_qconv_i8_centred_fwd(const int8_t* codes, const void* prepared,
                                        const float* scale, int64_t Nb, int64_t Ci, int64_t H,
                                        int64_t W, int64_t Co, int64_t R, int64_t S,
                                        int64_t stride, int64_t pad, int64_t groups,
                                        float act_zero_point, int act_qmin, int act_qmax, float* y,
                                        ssq_stream_t stream) {
  SSQ_REQUIRE(y, SSQ_E_ARG, "ssq_qconv_i8_centred_fwd: null pointer");
  return qconv_i8_launch("ssq_qconv_i8_centred_fwd", true,
                         {codes, prepared, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups,
                          act_zero_point, act_qmin, act_qmax},
                         y, nullptr, nullptr, stream);
}

extern "C" int ssq_qconv_i8_codes_fwd(const int8_t* codes, const void* prepared,
                                      const float* scale, int64_t Nb, int64_t Ci, int64_t H,
                                      int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride,
                                      int64_t pad, int64_t groups, float act_zero_point,
                                      int act_qmin, int act_qmax, const float* bias,
                                      const float* gamma, const float* phi, int act,
                                      float out_delta, float out_zero_point, int out_qmin,
                                      int out_qmax, int8_t* out_codes, uint32_t* bad,
                                      ssq_stream_t stream) {
  const char* me = "ssq_qconv_i8_codes_fwd";
  QEpi e;
  const int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin,
                           out_qmax, out_codes, bad, &e);
  if (rc) return rc;
  return qconv_i8_launch(me, false,
                         {codes, prepared, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups,
                          act_zero_point, act_qmin, act_qmax},
                         nullptr, &e, nullptr, stream);
}

extern "C" int ssq_qconv_i8_centred_codes_fwd(const int8_t* codes, const void* prepared,
                                              const float* scale, int64_t Nb, int64_t Ci,
                                              int64_t H, int64_t W, int64_t Co, int64_t R,
                                              int64_t S, int64_t stride, int64_t pad,
                                              int64_t groups, float act_zero_point, int act_qmin,
                                              int act_qmax, const float* bias, const float* gamma,
                                              const float* phi, int act, float out_delta,
                                              float out_zero_point, int out_qmin, int out_qmax,
                                              int8_t* out_codes, uint32_t* bad,
                                              ssq_stream_t stream) {
  const char* me = "ssq_qconv_i8_centred_codes_fwd";
  QEpi e;
  const int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin,
                           out_qmax, out_codes, bad, &e);
  if (rc) return rc;
  return qconv_i8_launch(me, true,
                         {codes, prepared, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups,
                          act_zero_point, act_qmin, act_qmax},
                         nullptr, &e, nullptr, stream);
}

extern "C" int ssq_qconv_i8_codes_res_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t Ci,
    int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
    int64_t groups, float act_zero_point, int act_qmin, int act_qmax, const float* bias,
    const float* gamma, const float* phi, int act, float out_delta, float out_zero_point,
    int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad, const float* res_f32,
    const int8_t* res_codes, float res_delta, float res_zero_point, int res_qmin, int res_qmax,
    ssq_stream_t stream) {
  const char* me = "ssq_qconv_i8_codes_res_fwd";
  QEpi e;
  QRes r;
  int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin, out_qmax,
                     out_codes, bad, &e);
  if (!rc) rc = qres_init(me, res_f32, res_codes, res_delta, res_zero_point, res_qmin, res_qmax, &r);
  if (rc) return rc;
  return qconv_i8_launch(me, false,
                         {codes, prepared, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups,
                          act_zero_point, act_qmin, act_qmax},
                         nullptr, &e, &r, stream);
}

extern "C" int ssq_qconv_i8_centred_codes_res_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t Ci,
    int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
    int64_t groups, float act_zero_point, int act_qmin, int act_qmax, const float* bias,
    const float* gamma, const float* phi, int act, float out_delta, float out_zero_point,
    int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad, const float* res_f32,
    const int8_t* res_codes, float res_delta, float res_zero_point, int res_qmin, int res_qmax,
    ssq_stream_t stream) {
  const char* me = "ssq_qconv_i8_centred_codes_res_fwd";
  QEpi e;
  QRes r;
  int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin, out_qmax,
                     out_codes, bad, &e);
  if (!rc) rc = qres_init(me, res_f32, res_codes, res_delta, res_zero_point, res_qmin, res_qmax, &r);
  if (rc) return rc;
  return qconv_i8_launch(me, true,
                         {codes, prepared, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups,
                          act_zero_point, act_qmin, act_qmax},
                         nullptr, &e, &r, stream);
}

// The wide forms: the centred forms' arguments, checks and epilogues on a blob of
// ssq_qweight_prepare_wide (two int8 digit planes, eight MFMAs per k step).
extern "C" int ssq_qconv_i8_wide_fwd(const int8_t* codes, const void* prepared, const float* scale,
                                     int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                     int64_t R, int64_t S, int64_t stride, int64_t pad,
                                     int64_t groups, float act_zero_point, int act_qmin,
                                     int act_qmax, float* y, ssq_stream_t stream) {
  SSQ_REQUIRE(y, SSQ_E_ARG, "ssq_qconv_i8_wide_fwd: null pointer");
  return qconv_i8_launch("ssq_qconv_i8_wide_fwd", true,
                         {codes, prepared, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups,
                          act_zero_point, act_qmin, act_qmax},
                         y, nullptr, nullptr, stream, nullptr, true);
}

extern "C" int ssq_qconv_i8_wide_codes_fwd(const int8_t* codes, const void* prepared,
                                           const float* scale, int64_t Nb, int64_t Ci, int64_t H,
                                           int64_t W, int64_t Co, int64_t R, int64_t S,
                                           int64_t stride, int64_t pad, int64_t groups,
                                           float act_zero_point, int act_qmin, int act_qmax,
                                           const float* bias, const float* gamma, const float* phi,
                                           int act, float out_delta, float out_zero_point,
                                           int out_qmin, int out_qmax, int8_t* out_codes,
                                           uint32_t* bad, ssq_stream_t stream) {
  const char* me = "ssq_qconv_i8_wide_codes_fwd";
  QEpi e;
  const int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin,
                           out_qmax, out_codes, bad, &e);
  if (rc) return rc;
  return qconv_i8_launch(me, true,
                         {codes, prepared, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups,
                          act_zero_point, act_qmin, act_qmax},
                         nullptr, &e, nullptr, stream, nullptr, true);
}

extern "C" int ssq_qconv_i8_wide_codes_res_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t Ci,
    int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
    int64_t groups, float act_zero_point, int act_qmin, int act_qmax, const float* bias,
    const float* gamma, const float* phi, int act, float out_delta, float out_zero_point,
    int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad, const float* res_f32,
    const int8_t* res_codes, float res_delta, float res_zero_point, int res_qmin, int res_qmax,
    ssq_stream_t stream) {
  const char* me = "ssq_qconv_i8_wide_codes_res_fwd";
  QEpi e;
  QRes r;
  int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin, out_qmax,
                     out_codes, bad, &e);
  if (!rc) rc = qres_init(me, res_f32, res_codes, res_delta, res_zero_point, res_qmin, res_qmax, &r);
  if (rc) return rc;
  return qconv_i8_launch(me, true,
                         {codes, prepared, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups,
                          act_zero_point, act_qmin, act_qmax},
                         nullptr, &e, &r, stream, nullptr, true);
}

extern "C" int ssq_act_decode(const int8_t* codes, int64_t Nb, int64_t C, int64_t H, int64_t W,
                              float delta, float zero_point, int qmin, float* x,
                              ssq_stream_t stream) {
  SSQ_REQUIRE(codes && x, SSQ_E_ARG, "ssq_act_decode: null pointer");
  SSQ_REQUIRE(Nb >= 1 && C >= 1 && H >= 1 && W >= 1, SSQ_E_ARG, "ssq_act_decode: bad geometry");
  SSQ_REQUIRE(qmin >= -128 && qmin <= 0, SSQ_E_ARG, "ssq_act_decode: qmin %d not in [-128, 0]",
              qmin);
  // decode has no qmax of its own: the widest range from qmin, which always fits
  const int rc = qquant_ok("ssq_act_decode", "", &delta, zero_point, qmin, qmin + 255);
  if (rc) return rc;
  const int64_t Cp = rup(C, 16);
  SSQ_REQUIRE(Nb * H * W * Cp < (1ll << 31), SSQ_E_ARG,
              "ssq_act_decode: tensor exceeds 2^31 elements");
  const uint32_t npix = (uint32_t)(Nb * H * W), HW = (uint32_t)(H * W);
  const dim3 grid(grid_for((int64_t)npix * (Cp / 16), kBlock, 8192));
  hipLaunchKernelGGL(act_decode_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, codes, npix,
                     HW, (uint32_t)C, (uint32_t)Cp, make_fastdiv(npix), make_fastdiv(HW), delta,
                     zero_point, (float)qmin, x);
  return check_launch("ssq_act_decode");
}

// ---------------------------------------------------------------- K23 split along K: the ABI
extern "C" size_t ssq_qconv_i8_splitk_workspace_size(int64_t Nb, int64_t H, int64_t W, int64_t Co,
                                                     int64_t R, int64_t S, int64_t stride,
                                                     int64_t pad, int64_t Cp, int splits,
                                                     int centred) {
  if (Nb < 1 || H < 1 || W < 1 || Co < 1 || R < 1 || S < 1 || R > 7 || S > 7 || stride < 1 ||
      pad < 0 || H + 2 * pad < R || W + 2 * pad < S || Cp < 16 || Cp % 16 != 0)
    return 0;
  const int64_t nk = rup(R * S * Cp, kQT) / kQT;
  if (splits < 2 || splits > kQMaxSplits || splits > nk) return 0;
  const int64_t OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
  if (Nb * OH * OW * Co >= (1ll << 31)) return 0;
  return qsplit_ws_bytes(Nb * OH * OW, Co, splits, centred != 0);
}

// The six dense entry points again, each with (splits, ws, ws_bytes) before the stream: the
// parent's checks, then the split's, then the partial and the finish kernel on `stream`.
#define SSQ_QCONV_IN                                                                       \
  {codes, prepared, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups, act_zero_point,    \
   act_qmin, act_qmax}

static int qsplitk_fwd(const char* me, bool centred, const QConvIn& a, float* y, const QSplit& sp,
                       ssq_stream_t stream) {
  SSQ_REQUIRE(y, SSQ_E_ARG, "%s: null pointer", me);
  return qconv_i8_launch(me, centred, a, y, nullptr, nullptr, stream, &sp);
}

extern "C" int ssq_qconv_i8_splitk_fwd(const int8_t* codes, const void* prepared,
                                       const float* scale, int64_t Nb, int64_t Ci, int64_t H,
                                       int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride,
                                       int64_t pad, int64_t groups, float act_zero_point,
                                       int act_qmin, int act_qmax, float* y, int splits, void* ws,
                                       size_t ws_bytes, ssq_stream_t stream) {
  return qsplitk_fwd("ssq_qconv_i8_splitk_fwd", false, SSQ_QCONV_IN, y, {splits, ws, ws_bytes},
                     stream);
}

extern "C" int ssq_qconv_i8_centred_splitk_fwd(const int8_t* codes, const void* prepared,
                                               const float* scale, int64_t Nb, int64_t Ci,
                                               int64_t H, int64_t W, int64_t Co, int64_t R,
                                               int64_t S, int64_t stride, int64_t pad,
                                               int64_t groups, float act_zero_point, int act_qmin,
                                               int act_qmax, float* y, int splits, void* ws,
                                               size_t ws_bytes, ssq_stream_t stream) {
  return qsplitk_fwd("ssq_qconv_i8_centred_splitk_fwd", true, SSQ_QCONV_IN, y,
                     {splits, ws, ws_bytes}, stream);
}

static int qsplitk_codes(const char* me, bool centred, const QConvIn& a, const float* bias,
                         const float* gamma, const float* phi, int act, float out_delta,
                         float out_zero_point, int out_qmin, int out_qmax, int8_t* out_codes,
                         uint32_t* bad, const QSplit& sp, ssq_stream_t stream) {
  QEpi e;
  const int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin,
                           out_qmax, out_codes, bad, &e);
  if (rc) return rc;
  return qconv_i8_launch(me, centred, a, nullptr, &e, nullptr, stream, &sp);
}

extern "C" int ssq_qconv_i8_splitk_codes_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t Ci,
    int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
    int64_t groups, float act_zero_point, int act_qmin, int act_qmax, const float* bias,
    const float* gamma, const float* phi, int act, float out_delta, float out_zero_point,
    int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad, int splits, void* ws,
    size_t ws_bytes, ssq_stream_t stream) {
  return qsplitk_codes("ssq_qconv_i8_splitk_codes_fwd", false, SSQ_QCONV_IN, bias, gamma, phi, act,
                       out_delta, out_zero_point, out_qmin, out_qmax, out_codes, bad,
                       {splits, ws, ws_bytes}, stream);
}

extern "C" int ssq_qconv_i8_centred_splitk_codes_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t Ci,
    int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
    int64_t groups, float act_zero_point, int act_qmin, int act_qmax, const float* bias,
    const float* gamma, const float* phi, int act, float out_delta, float out_zero_point,
    int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad, int splits, void* ws,
    size_t ws_bytes, ssq_stream_t stream) {
  return qsplitk_codes("ssq_qconv_i8_centred_splitk_codes_fwd", true, SSQ_QCONV_IN, bias, gamma,
                       phi, act, out_delta, out_zero_point, out_qmin, out_qmax, out_codes, bad,
                       {splits, ws, ws_bytes}, stream);
}

static int qsplitk_codes_res(const char* me, bool centred, const QConvIn& a, const float* bias,
                             const float* gamma, const float* phi, int act, float out_delta,
                             float out_zero_point, int out_qmin, int out_qmax, int8_t* out_codes,
                             uint32_t* bad, const float* res_f32, const int8_t* res_codes,
                             float res_delta, float res_zero_point, int res_qmin, int res_qmax,
                             const QSplit& sp, ssq_stream_t stream) {
  QEpi e;
  QRes r;
  int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin, out_qmax,
                     out_codes, bad, &e);
  if (!rc) rc = qres_init(me, res_f32, res_codes, res_delta, res_zero_point, res_qmin, res_qmax, &r);
  if (rc) return rc;
  return qconv_i8_launch(me, centred, a, nullptr, &e, &r, stream, &sp);
}

extern "C" int ssq_qconv_i8_splitk_codes_res_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t Ci,
    int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
    int64_t groups, float act_zero_point, int act_qmin, int act_qmax, const float* bias,
    const float* gamma, const float* phi, int act, float out_delta, float out_zero_point,
    int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad, const float* res_f32,
    const int8_t* res_codes, float res_delta, float res_zero_point, int res_qmin, int res_qmax,
    int splits, void* ws, size_t ws_bytes, ssq_stream_t stream) {
  return qsplitk_codes_res("ssq_qconv_i8_splitk_codes_res_fwd", false, SSQ_QCONV_IN, bias, gamma,
                           phi, act, out_delta, out_zero_point, out_qmin, out_qmax, out_codes, bad,
                           res_f32, res_codes, res_delta, res_zero_point, res_qmin, res_qmax,
                           {splits, ws, ws_bytes}, stream);
}

extern "C" int ssq_qconv_i8_centred_splitk_codes_res_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t Ci,
    int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
    int64_t groups, float act_zero_point, int act_qmin, int act_qmax, const float* bias,
    const float* gamma, const float* phi, int act, float out_delta, float out_zero_point,
    int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad, const float* res_f32,
    const int8_t* res_codes, float res_delta, float res_zero_point, int res_qmin, int res_qmax,
    int splits, void* ws, size_t ws_bytes, ssq_stream_t stream) {
  return qsplitk_codes_res("ssq_qconv_i8_centred_splitk_codes_res_fwd", true, SSQ_QCONV_IN, bias,
                           gamma, phi, act, out_delta, out_zero_point, out_qmin, out_qmax,
                           out_codes, bad, res_f32, res_codes, res_delta, res_zero_point, res_qmin,
                           res_qmax, {splits, ws, ws_bytes}, stream);
}
#undef SSQ_QCONV_IN
