// K25 / K26, the grouped and depthwise integer conv kernels (qinfer_grouped.hip has the contract and
// the launches).  They live in a header because they are instantiated in two translation units:
// the scalar forms in qinfer_grouped.hip, built with the library's flags as they always were, and
// the per-channel forms (CHQ) in qinfer_grouped_chq.hip, which build.py compiles without packed
// fp32 instructions (SSQ_NO_PK_F32's reason, qinfer_epi.h) -- a function attribute cannot be put
// on some instantiations of a template, and any other way of sharing the text (a device function
// both kernels inline, the attribute on the template) changes the scalar kernels' registers.
#pragma once
#include <type_traits>

#include "ssq_common.h"
#include "qinfer_epi.h"
#include "qinfer_layout.h"

namespace ssq {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kGRow = 80;    // LDS row stride in bytes (64 + 16), as K23

// ---------------------------------------------------------------- K25 depthwise direct conv
struct QDwGeo {
  uint32_t M, P, OW, H, W, C, Cp, R, S, nch, per;   // per: chunks per workgroup (blockIdx.y)
  int stride, pad, az, padv;
  FastDiv div_p, div_ow;
};

// KS: the square kernel size the s loop is unrolled for (its loads fly together); 0: any R x S
// CODES: the code-emitting epilogue (qinfer_epi.h), `y` then being the QEpi: the thread's 16
// channels of its pixel leave as one 16-B store of the NHWC codes instead of 16 fp32 stores.
// CHQ (with CODES): the output quantizer's scale is per channel (`y` a QEpiCh).  The chunk `ch` is
// wave-uniform, as the weight address is, so the chunk's 16 out_dch entries are read once per
// chunk through uniform addresses in front of the tap loop (readfirstlane: they sit in SGPRs over
// it), never per pixel.  Thread 0 of the first pixel block counts the entries that are no scale
// (qdch_bad) into its wave's count: every chunk is walked by exactly one blockIdx.y, so each
// entry is counted once per launch.
template <bool CODES, bool CHQ>
using QGOut = typename std::conditional<
    CODES, typename std::conditional<CHQ, QEpiCh, QEpi>::type, float* __restrict__>::type;

template <int KS, bool CODES, bool CHQ = false>
__global__ __launch_bounds__(kBlock) void qconv_dw_kernel(
    const int8_t* __restrict__ act, const int32_t* __restrict__ wc, const float* __restrict__ scale,
    QDwGeo g, QGOut<CODES, CHQ> y) {
  static_assert(!CHQ || CODES, "a per-channel output grid goes with the code-emitting epilogue");
  const uint32_t pix0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (!CODES && pix0 >= g.M) return;
  // CODES: a thread past M stays for the wave's count, computing pixel 0 and storing nothing
  const bool pval = pix0 < g.M;
  const uint32_t pix = pval ? pix0 : 0u;
  uint32_t nbad = 0;
  const uint32_t n = fdiv(pix, g.div_p);
  const uint32_t p = pix - n * g.P;
  const uint32_t oh = fdiv(p, g.div_ow);
  const uint32_t ow = p - oh * g.OW;
  const int ih0 = (int)oh * g.stride - g.pad, iw0 = (int)ow * g.stride - g.pad;
  const uint32_t R = KS ? KS : g.R, S = KS ? KS : g.S;
  const int pv = (g.padv & 0xff) * 0x01010101;
  const i32x4 padfill = {pv, pv, pv, pv};
  const uint32_t ch0 = blockIdx.y * g.per;
  const uint32_t ch1 = min(ch0 + g.per, g.nch);
  for (uint32_t ch = ch0; ch < ch1; ++ch) {
    // byte offsets fit 32 bits: the host checked Nb*H*W*Cp < 2^31
    const int8_t* abase = act + (n * g.H * g.W * g.Cp + ch * 16);
    int acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0;
    float od[CHQ ? 16 : 1];   // CHQ: out_dch of the chunk's channels (1 past C: never divided by)
    if constexpr (CHQ) {
      const bool counts = blockIdx.x == 0 && threadIdx.x == 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool cval = ch * 16 + j < g.C;   // uniform: nothing past dch[C) is read
        od[j] = cval ? __int_as_float(__builtin_amdgcn_readfirstlane(
                           __float_as_int(y.dch[ch * 16 + j])))
                     : 1.0f;
        if (counts && cval && qdch_bad(od[j])) nbad += 1u;
      }
    }
#pragma unroll 1
    for (uint32_t r = 0; r < R; ++r) {
      const int ih = ih0 + (int)r;
      const bool rok = (uint32_t)ih < g.H;
      const int8_t* arow = abase + (uint32_t)(rok ? ih : 0) * g.W * g.Cp;
      const int32_t* wr = wc + (r * S * g.Cp + ch * 16);   // wave-uniform
#pragma unroll
      for (uint32_t s = 0; s < S; ++s) {
        const int iw = iw0 + (int)s;
        const bool ok = rok && (uint32_t)iw < g.W;
        i32x4 v = *(const i32x4*)(arow + (uint32_t)(ok ? iw : 0) * g.Cp);   // in bounds either way
        if (!ok) v = padfill;
        const int32_t* wt = wr + s * g.Cp;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t word = (uint32_t)v[q];
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int a = ((int)(word << (24 - 8 * b)) >> 24) + g.az;   // sign-extended byte + az
            acc[q * 4 + b] += __mul24(a, wt[q * 4 + b]);   // |a| < 2^9, |wc| < 2^14
          }
        }
      }
    }
    if constexpr (CODES) {
      const QEpi& e = y;
      i32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        int c4[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint32_t c = ch * 16 + q * 4 + b;
          if constexpr (CHQ)   // qepi_code's product, then the epilogue on the channel's scale
            c4[b] = (pval && c < g.C) ? qepi_code_yd(__fmul_rn((float)acc[q * 4 + b], scale[c]), c,
                                                     e, od[q * 4 + b], nbad)
                                      : 0;
          else
            c4[b] = (pval && c < g.C) ? qepi_code((float)acc[q * 4 + b], c, scale, e, nbad) : 0;
        }
        o[q] = qepi_pack4(c4[0], c4[1], c4[2], c4[3]);
      }
      if (pval) *(i32x4*)(e.out + (size_t)pix * g.Cp + ch * 16) = o;
    } else {
      float* yo = y + (size_t)((n * g.C + ch * 16) * g.P + p);   // Nb*OH*OW*Co < 2^31, so is this
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t c = ch * 16 + j;
        if (c < g.C) yo[(size_t)(j * g.P)] = __fmul_rn((float)acc[j], scale[c]);
      }
    }
  }
  if constexpr (CODES) qepi_count(nbad, y.bad);
}

// ---------------------------------------------------------------- K26 grouped int8 MFMA conv
struct QGConvGeo {
  uint32_t M, P, OW, H, W, Cp, Co, Cig, Cog, Cogp, Wc, Kp, RS, S, tiles;
  int stride, pad, az, padv;
  FastDiv div_p, div_ow, div_wc, div_s, div_tiles;
};

// the epilogue's integer sum of channel co: I = D + cwz[co] * SA_g + az * T[co], or, WIDE (`d` is
// D_h, `dl` D_l), I = 128 D_h + D_l + az * T[co]
template <bool WIDE>
__device__ __forceinline__ long long qg_sum(int d, int dl, const int32_t* __restrict__ cwz,
                                            long long sa, int az, const int32_t* __restrict__ tt,
                                            uint32_t co) {
  if constexpr (WIDE)
    return 128ll * (long long)d + (long long)dl + (long long)az * (long long)tt[co];
  else
    return (long long)d + (long long)cwz[co] * sa + (long long)az * (long long)tt[co];
}

// one `T` per (pixel row, unit) of the transposed code tile, LDS -> the NHWC codes
template <typename T>
__device__ __forceinline__ void qg_store_units(const int8_t* lds, int8_t* out, uint32_t units,
                                               uint32_t sub) {
  for (uint32_t u = sub; u < units; u += 4) ((T*)out)[u] = ((const T*)lds)[u];
}

// CODES: the code-emitting epilogue (qinfer_epi.h), `y` then being the QEpi.  The workgroup's
// code tile is transposed through the (then free) activation tile; it owns the bytes
// [c0, c1) of every pixel, c0 = the tile's first channel, c1 one past its last real one -- or
// Cpo when that is the layer's last channel (the zero padding is its to write) -- and stores
// them at the widest power of two up to 16 B that divides both c0 and c1 - c0: two workgroups
// may own different bytes of one 16-B chunk, none writes a byte of another's.
// WIDE: the blob's two digit planes (h, then l at `plane` bytes) take the place of the weight tile
// and the 0/1 row: lB rows [0, 64) hold h, [64, 128) l; acc is D_h, accl D_l; `masks` and `cwz`
// are not read.
// CHQ (with CODES; qconv_grouped_chq_kernel): the output quantizer's scale is per channel (QEpiCh).
// A lane's channels are fixed, row0 + 16 j + 4 fq + r, so its out_dch entries -- rows < Cog of the
// fragments j < nf only -- are loaded once after the K loop, where bias / gamma / phi are read; the
// first pixel tile's wave 0 counts those of its channel tile that are no scale (qdch_bad).
template <bool CODES, bool WIDE = false, bool CHQ = false>
__global__ __launch_bounds__(kBlock) void qconv_grouped_kernel(
    const int8_t* __restrict__ act, const int8_t* __restrict__ wp, const int8_t* __restrict__ masks,
    const int32_t* __restrict__ cwz, const int32_t* __restrict__ tt,
    const float* __restrict__ scale, QGConvGeo g, QGOut<CODES, CHQ> y) {
  static_assert(!CHQ || CODES, "a per-channel output grid goes with the code-emitting epilogue");
  __shared__ __attribute__((aligned(16))) int8_t lA[kGT * kGRow];
  __shared__ __attribute__((aligned(16))) int8_t lB[(WIDE ? 2 * kGT : kGT + 1) * kGRow];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & (kWave - 1), wave = tid / kWave;
  const uint32_t fr = lane & 15, fq = lane >> 4;

  // the workgroup's group, channel tile and number of 16-row fragments (uniform)
  const uint32_t grp = fdiv(blockIdx.y, g.div_tiles);
  const uint32_t tile = blockIdx.y - grp * g.tiles;
  const uint32_t row0 = tile * kGT;                       // first row inside the group
  const uint32_t nrow = min(g.Cogp - row0, (uint32_t)kGT);   // multiple of 16
  const uint32_t nf = nrow >> 4;
  const uint32_t w0 = grp * g.Cig / 16 * 16;              // window start channel

  // staging role: one 16-byte chunk of each operand tile per thread
  const uint32_t srow = tid >> 2, sc = tid & 3;
  const uint32_t gm = blockIdx.x * kGT + srow;
  const bool mval = gm < g.M;
  const uint32_t gmc = mval ? gm : 0u;
  const uint32_t sn = fdiv(gmc, g.div_p);
  const uint32_t sp = gmc - sn * g.P;
  const uint32_t soh = fdiv(sp, g.div_ow);
  const uint32_t sow = sp - soh * g.OW;
  const int ih0 = (int)soh * g.stride - g.pad, iw0 = (int)sow * g.stride - g.pad;
  const int8_t* abase = act + (size_t)sn * g.H * g.W * g.Cp;
  const bool bval = srow < nrow;
  const int8_t* wrow = wp + (size_t)(grp * g.Cogp + row0 + (bval ? srow : 0u)) * g.Kp + sc * 16;
  const int8_t* mrow = masks + (size_t)grp * g.Kp;
  const size_t plane = WIDE ? (size_t)(gridDim.y / g.tiles) * g.Cogp * g.Kp : 0;   // G * Cogp * Kp
  const int pv = (g.padv & 0xff) * 0x01010101;
  const i32x4 padfill = {pv, pv, pv, pv};
  const i32x4 zero4 = {0, 0, 0, 0};

  auto load_a = [&](uint32_t kt) -> i32x4 {
    const uint32_t k = kt * kGT + sc * 16;
    const uint32_t tap = fdiv(k, g.div_wc);
    const uint32_t c0 = w0 + (k - tap * g.Wc);
    const uint32_t r = fdiv(tap, g.div_s);
    const uint32_t s = tap - r * g.S;
    const int ih = ih0 + (int)r, iw = iw0 + (int)s;
    if (mval && tap < g.RS && c0 < g.Cp && (uint32_t)ih < g.H && (uint32_t)iw < g.W)
      return *(const i32x4*)(abase + ((size_t)ih * g.W + (size_t)iw) * g.Cp + c0);
    return padfill;
  };

  i32x4 ra = load_a(0);
  i32x4 rb = bval ? *(const i32x4*)wrow : zero4;
  i32x4 rm = zero4;   // WIDE: the thread's chunk of the l plane
  if constexpr (WIDE) {
    if (bval) rm = *(const i32x4*)(wrow + plane);
  } else {
    if (tid < 4) rm = *(const i32x4*)(mrow + tid * 16);
  }

  i32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = zero4;
  i32x4 accl[WIDE ? 4 : 1];
#pragma unroll
  for (int j = 0; j < (WIDE ? 4 : 1); ++j) accl[j] = zero4;
  i32x4 accs = zero4;

  const uint32_t nk = g.Kp / kGT;
  for (uint32_t kt = 0; kt < nk; ++kt) {
    __syncthreads();   // the previous step's fragment reads are done
    *(i32x4*)(lA + srow * kGRow + sc * 16) = ra;
    if (bval) *(i32x4*)(lB + srow * kGRow + sc * 16) = rb;
    if constexpr (WIDE) {
      if (bval) *(i32x4*)(lB + (kGT + srow) * kGRow + sc * 16) = rm;
    } else {
      if (tid < 4) *(i32x4*)(lB + kGT * kGRow + tid * 16) = rm;
    }
    __syncthreads();
    if (kt + 1 < nk) {
      ra = load_a(kt + 1);
      if (bval) rb = *(const i32x4*)(wrow + (size_t)(kt + 1) * kGT);
      if constexpr (WIDE) {
        if (bval) rm = *(const i32x4*)(wrow + plane + (size_t)(kt + 1) * kGT);
      } else {
        if (tid < 4) rm = *(const i32x4*)(mrow + (size_t)(kt + 1) * kGT + tid * 16);
      }
    }
    const i32x4 af = *(const i32x4*)(lA + (wave * 16 + fr) * kGRow + fq * 16);
    if constexpr (!WIDE) {
      const i32x4 mf = *(const i32x4*)(lB + kGT * kGRow + fq * 16);
      accs = __builtin_amdgcn_mfma_i32_16x16x64_i8(mf, af, accs, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((uint32_t)j < nf) {
        const i32x4 wf = *(const i32x4*)(lB + (j * 16 + fr) * kGRow + fq * 16);
        acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, af, acc[j], 0, 0, 0);
        if constexpr (WIDE) {
          const i32x4 lf = *(const i32x4*)(lB + (kGT + j * 16 + fr) * kGRow + fq * 16);
          accl[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(lf, af, accl[j], 0, 0, 0);
        }
      }
    }
  }

  // C/D map: column (pixel) = lane & 15, row (channel) = 4 * (lane >> 4) + reg
  const uint32_t pixel = blockIdx.x * kGT + wave * 16 + fr;
  const long long sa = (long long)accs[0];
  if constexpr (CODES) {
    const QEpi& e = y;
    const bool pval = pixel < g.M;
    uint32_t nbad = 0;
    float od[CHQ ? 16 : 1];   // out_dch of the lane's channels
    if constexpr (CHQ) {
      const bool counts = blockIdx.x == 0 && wave == 0 && fr == 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t rl = row0 + j * 16 + fq * 4 + r;
          const bool cval = (uint32_t)j < nf && rl < g.Cog;
          od[j * 4 + r] = cval ? y.dch[grp * g.Cog + rl] : 1.0f;
          if (counts && cval && qdch_bad(od[j * 4 + r])) nbad += 1u;
        }
      }
    }
    __syncthreads();   // the last step's fragment reads are done: lA is free
    // chunks the codes below do not write: zero (the layer's channel padding lies there)
    if (sc + 1 >= nf) *(i32x4*)(lA + srow * kGRow + (sc + 1) * 16) = zero4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((uint32_t)j >= nf) continue;
      int c[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t rl = row0 + j * 16 + fq * 4 + r;
        c[r] = 0;
        if (pval && rl < g.Cog) {
          const uint32_t co = grp * g.Cog + rl;
          const long long I = qg_sum<WIDE>(acc[j][r], accl[WIDE ? j : 0][r], cwz, sa, g.az, tt, co);
          if constexpr (CHQ)   // qepi_code's product, then the epilogue on the channel's scale
            c[r] = qepi_code_yd(__fmul_rn((float)I, scale[co]), co, e, od[j * 4 + r], nbad);
          else
            c[r] = qepi_code((float)I, co, scale, e, nbad);
        }
      }
      *(int*)(lA + (wave * 16 + fr) * kGRow + j * 16 + fq * 4) = qepi_pack4(c[0], c[1], c[2], c[3]);
    }
    __syncthreads();
    const uint32_t c0 = grp * g.Cog + row0;
    uint32_t c1 = grp * g.Cog + min(row0 + nrow, g.Cog);
    if (c1 == g.Co) c1 = e.Cpo;          // at most row0's 64 + 15 bytes: inside the 80-B row
    const uint32_t len = c1 - c0;
    const uint32_t a = (c0 | len | 16u);
    const uint32_t w = a & (0u - a);     // lowest set bit: 1, 2, 4, 8 or 16
    if (mval) {
      const int8_t* src = lA + srow * kGRow;
      int8_t* dst = e.out + (size_t)gm * e.Cpo + c0;
      if (w == 16) qg_store_units<i32x4>(src, dst, len >> 4, sc);
      else if (w == 8) qg_store_units<uint64_t>(src, dst, len >> 3, sc);
      else if (w == 4) qg_store_units<uint32_t>(src, dst, len >> 2, sc);
      else if (w == 2) qg_store_units<uint16_t>(src, dst, len >> 1, sc);
      else qg_store_units<uint8_t>(src, dst, len, sc);
    }
    qepi_count(nbad, e.bad);
  } else {
    if (pixel >= g.M) return;
    const uint32_t n = fdiv(pixel, g.div_p);
    const uint32_t p = pixel - n * g.P;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((uint32_t)j >= nf) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t rl = row0 + j * 16 + fq * 4 + r;
        if (rl < g.Cog) {
          const uint32_t co = grp * g.Cog + rl;
          const long long I = qg_sum<WIDE>(acc[j][r], accl[WIDE ? j : 0][r], cwz, sa, g.az, tt, co);
          y[((size_t)n * g.Co + co) * g.P + p] = __fmul_rn((float)I, scale[co]);
        }
      }
    }
  }
}

// The CHQ instantiations' launches (qinfer_grouped_chq.hip); R, S pick K25's KS as the scalar
// launch does
void qconv_dw_chq_launch(int64_t R, int64_t S, dim3 grid, hipStream_t stream, const int8_t* codes,
                         const int32_t* wc, const float* scale, const QDwGeo& g, const QEpiCh& e);
void qconv_grouped_chq_launch(bool wide, dim3 grid, hipStream_t stream, const int8_t* codes,
                              const int8_t* wp, const int8_t* masks, const int32_t* cwz,
                              const int32_t* tt, const float* scale, const QGConvGeo& g,
                              const QEpiCh& e);

}  // namespace ssq
