// K24-K26: integer inference of grouped and depthwise convs (groups >= 2).
//
// Same contract as K23 (qinfer.hip): y[n, co, p] = fp32(I) * s[co] with
//     I = sum over the K = Cig*R*S taps of co's group of (q_a - z_a)(q_w - z_w[co])
// exact, one int -> fp32 conversion and one __fmul_rn.  The activation operand is K21's as it
// stands: dense NHWC int8 a_s = q_a - ca with C padded to Cp = 16*ceil(C/16) at the end only.
// One rule (qg_kind) picks the kernel in prepare and in the conv:
//
// kind 1, depthwise (groups == C == Co), K25 qconv_dw_kernel.  K is 1..49 taps: nothing for
// the MFMA.  One thread per output pixel, the 64 lanes of a wave on 64 consecutive pixels; a
// workgroup walks a run of consecutive 16-channel chunks for its 256 pixels, so the chunks
// that share a cache line of the NHWC codes are read by one CU.  Per tap one 16-B code load
// (a padded tap takes the pad value z_a - ca instead, its (q_a - z_a) = 0), 16 x
// (a_s + az) * wc into int32 (an int8-range blob: |I| <= 49 * 255^2 < 2^24, exact, and so is the
// conversion; the wide blob below: exact sum, rounding conversion);
// 16 fp32 stores per chunk, each coalesced across the wave's pixels of one NCHW channel
// plane.  The prepared blob is the centred weight wc = q_w - z_w[c] as int32 [R*S][Cp] (0 on
// padded channels); its address is wave-uniform, so the 16 values of a (tap, chunk) come
// through the scalar cache into SGPRs: no LDS, no barrier.
//
// kind 2, everything else, K26 qconv_grouped_kernel: K23's tile and shift-and-correct identity
// per group,  I = D + cwz[co] * SA_g + az * T[co],  K = Cig*R*S.  A group's channels need not
// start or end on a 16-B chunk, so group g reads the 16-aligned channel window that covers it,
//     [w0_g, w0_g + Wc),  w0_g = 16*floor(g*Cig/16),  Wc = max_g (16*ceil((g+1)*Cig/16) - w0_g),
// k = tap * Wc + (c - w0_g).  Its prepared weight rows and its own 0/1 row are zero on window
// channels outside the group (and on the k tail), so D and SA_g see the group only whatever
// the neighbouring channels hold; a chunk past Cp is not loaded.  A workgroup owns 64 output
// pixels x one tile of up to 64 channels of one group; rows are stored per group padded to
// Cogp = 16*ceil(Cog/16) and a tile runs only the 16-row fragments it has (Cog = 8: one MFMA
// + the SA MFMA per k step, not four).
// Blob: int8 [G*Cogp][Kp], Kp = 64*ceil(R*S*Wc/64); the 0/1 rows [G][Kp]; cwz[Co], T[Co] (int32).
//
// The wide operand (ssq_qweight_prepare_grouped_wide and the *_grouped_wide_* convs), for a scaled
// weight whose centred m = (q - z_w[co]) * k leaves int8 (|m| <= 16319, qinfer_prepare.h):
// kind 2 holds m = 128 h + l as two int8 digit planes of the rows above (qinfer_layout.h) and K26's
// WIDE instantiations stage one chunk of each plane per k step, 2 nf MFMAs, no 0/1 row and no SA
// MFMA:  I = 128 D_h + D_l + az * T[co]  in int64 (K <= 65536 keeps D_h, D_l below 2^30 and T
// inside int32); the epilogues are K26's own, and wherever |m| <= 127 the result is K26's on the
// centred int8 blob bit for bit.  LDS 15 360 B.
// kind 1 holds m in its int32 blob as it stands, column factors only (a depthwise row has no
// per-(co, ci) form): |a| * |m| < 2^9 * 2^14 keeps __mul24 exact and |I| <= 49 * 255 * 16319 < 2^31
// the int32 accumulator, but |I| may pass 2^24, so fp32(I) may round there: that is the
// contract's one conversion, round to nearest even, as K23's -- it is exact for the int8 blobs only.
#include <type_traits>

#include "ssq_common.h"
#include "qinfer_epi.h"
#include "qinfer_layout.h"
#include "qinfer_prepare.h"

namespace ssq {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kGRow = 80;    // LDS row stride in bytes (64 + 16), as K23
constexpr uint32_t kDwBlocks = 2048;   // workgroups K25 aims for: 8 per CU

// ---------------------------------------------------------------- K24 weight prepare
// Plain and COLSCALE as K22 (qinfer.hip): COLSCALE stores the centred integer
// m = (q - z_w[co]) * k, k the QFactor's entry of the element (qinfer_prepare.h): a column scale's
// k[j], j = (ci, r, s) within the group (J = Cig*R*S, shared by all groups), or a per-(co, ci)
// scale's k[co * Cig + ci]; *bad also counts what qscaled() counts.
//
// depthwise: one thread per (tap, padded channel) of K25's centred int32 blob [R*S][Cp],
// wc = q - z_w[c]; COLSCALE multiplies it by kcol[tap], factors and |m| up to `lim` (127, or
// kQWideMax for the wide form)
template <bool COLSCALE>
__global__ __launch_bounds__(kBlock) void qweight_prepare_dw_kernel(
    const uint8_t* __restrict__ packed, const float* __restrict__ zp,
    const int32_t* __restrict__ kcol, int lim, int bs, int qmin, uint32_t C, uint32_t RS,
    uint32_t Cp, FastDiv div_cp, int32_t* __restrict__ wc, uint32_t* __restrict__ bad) {
  const uint32_t total = RS * Cp;
  uint32_t nbad = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const uint32_t tap = fdiv(i, div_cp);
    const uint32_t c = i - tap * Cp;
    int v = 0;
    if (c < C) {
      const float zf = zp[c];
      const bool ok = zp_is_code(zf, qmin);
      const int z = ok ? (int)zf : qmin;
      if (!ok && tap == 0) ++nbad;   // counted once per channel
      v = (int)packed_code(packed, (size_t)c * RS + tap, bs) + qmin - z;
      if constexpr (COLSCALE) v = qscaled(v, kcol[tap], lim, nbad);
    }
    wc[i] = v;
  }
  if (nbad) atomicAdd(bad, nbad);
}

// grouped: one workgroup per padded row (g, rl), then one per group for its 0/1 row.  K26's blob;
// COLSCALE: m as the int8 operand, cwz = 0, T[co] = sum m, the 0/1 rows all the same.  WIDE (with
// COLSCALE): m leaves as its two digits, h into the first plane and l into the second,
// G * Cogp * Kp bytes behind
template <bool COLSCALE, bool WIDE = false>
__global__ __launch_bounds__(kBlock) void qweight_prepare_grouped_kernel(
    const uint8_t* __restrict__ packed, const float* __restrict__ zp, QFactor f, int bs, int qmin,
    uint32_t groups, uint32_t Cig,
    uint32_t Cog, uint32_t Cogp, uint32_t RS, uint32_t Wc, uint32_t Kp, FastDiv div_wc,
    FastDiv div_cogp, int8_t* __restrict__ wp, int8_t* __restrict__ mask,
    int32_t* __restrict__ cwz, int32_t* __restrict__ tt, uint32_t* __restrict__ bad) {
  static_assert(COLSCALE || !WIDE, "the wide blob holds a centred operand");
  __shared__ int red[kBlock / kWave];
  const uint32_t row = blockIdx.x;
  const uint32_t nrows = groups * Cogp;
  const uint32_t g = row >= nrows ? row - nrows : fdiv(row, div_cogp);
  const uint32_t lo = g * Cig - g * Cig / 16 * 16;   // the group's offset inside its window
  if (row >= nrows) {
    for (uint32_t k = threadIdx.x; k < Kp; k += blockDim.x) {
      const uint32_t tap = fdiv(k, div_wc);
      const uint32_t cw = k - tap * Wc;
      mask[(size_t)g * Kp + k] = (tap < RS && cw >= lo && cw < lo + Cig) ? 1 : 0;
    }
    return;
  }
  const uint32_t rl = row - g * Cogp;
  const uint32_t co = g * Cog + rl;
  const bool real = rl < Cog;
  const bool zok = !real || zp_is_code(zp[co], qmin);
  const int z = real && zok ? (int)zp[co] : qmin;
  int sum = 0;
  uint32_t nbad = 0;
  for (uint32_t k = threadIdx.x; k < Kp; k += blockDim.x) {
    const uint32_t tap = fdiv(k, div_wc);
    const uint32_t cw = k - tap * Wc;
    int v = 0;
    if (real && tap < RS && cw >= lo && cw < lo + Cig) {
      const size_t j = (size_t)(cw - lo) * RS + tap;
      const int u = (int)packed_code(packed, (size_t)co * Cig * RS + j, bs);   // q - qmin
      if constexpr (COLSCALE) v = qscaled(u + qmin - z, qfactor_at(f, co, cw - lo, tap), f.lim, nbad);
      else v = u - 128;   // q - cw, cw = qmin + 128
      sum += v;   // WIDE: |sum| <= 65536 * 16319 < 2^31
    }
    if constexpr (WIDE) {
      wp[(size_t)row * Kp + k] = (int8_t)qdigit_hi(v);
      wp[((size_t)nrows + row) * Kp + k] = (int8_t)qdigit_lo(v);
    } else {
      wp[(size_t)row * Kp + k] = (int8_t)v;
    }
  }
  sum = (int)wave_sum((uint32_t)sum);
  nbad = wave_sum(nbad);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red[threadIdx.x / kWave] = sum;
    if (nbad) atomicAdd(bad, nbad);
  }
  __syncthreads();
  if (threadIdx.x == 0 && real) {   // cwz and T have no padded rows
    int total = 0;
    for (int i = 0; i < kBlock / kWave; ++i) total += red[i];
    if (!zok) atomicAdd(bad, 1u);
    const int c = COLSCALE ? 0 : qmin + 128 - z;
    cwz[co] = c;
    tt[co] = total + (int)(Cig * RS) * c;
  }
}

// ---------------------------------------------------------------- K25 depthwise direct conv
struct QDwGeo {
  uint32_t M, P, OW, H, W, C, Cp, R, S, nch, per;   // per: chunks per workgroup (blockIdx.y)
  int stride, pad, az, padv;
  FastDiv div_p, div_ow;
};

// KS: the square kernel size the s loop is unrolled for (its loads fly together); 0: any R x S
// CODES: the code-emitting epilogue (qinfer_epi.h), `y` then being the QEpi: the thread's 16
// channels of its pixel leave as one 16-B store of the NHWC codes instead of 16 fp32 stores.
template <int KS, bool CODES>
__global__ __launch_bounds__(kBlock) void qconv_dw_kernel(
    const int8_t* __restrict__ act, const int32_t* __restrict__ wc, const float* __restrict__ scale,
    QDwGeo g, typename std::conditional<CODES, QEpi, float* __restrict__>::type y) {
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
template <bool CODES, bool WIDE = false>
__global__ __launch_bounds__(kBlock) void qconv_grouped_kernel(
    const int8_t* __restrict__ act, const int8_t* __restrict__ wp, const int8_t* __restrict__ masks,
    const int32_t* __restrict__ cwz, const int32_t* __restrict__ tt,
    const float* __restrict__ scale, QGConvGeo g,
    typename std::conditional<CODES, QEpi, float* __restrict__>::type y) {
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

// C < 0: the caller has no C of its own (prepare); else C must be Cig * groups
static int ggeo_ok(const char* what, const char* plain, int64_t C, int64_t Co, int64_t Cig,
                   int64_t R, int64_t S, int64_t groups, int planes = 1) {
  SSQ_REQUIRE(groups >= 2, SSQ_E_ARG, "%s: groups = %lld (groups >= 2 only; groups == 1 is %s)",
              what, (long long)groups, plain);
  SSQ_REQUIRE(C < 0 || (C >= 1 && C % groups == 0), SSQ_E_ARG,
              "%s: C = %lld is not divisible by groups = %lld", what, (long long)C,
              (long long)groups);
  SSQ_REQUIRE(Co >= 1 && Co % groups == 0, SSQ_E_ARG,
              "%s: Co = %lld is not divisible by groups = %lld", what, (long long)Co,
              (long long)groups);
  SSQ_REQUIRE(Cig >= 1 && R >= 1 && S >= 1 && R <= 7 && S <= 7, SSQ_E_ARG,
              "%s: bad geometry (Cig >= 1; R, S in [1, 7]; got R = %lld, S = %lld)", what,
              (long long)R, (long long)S);
  SSQ_REQUIRE(Cig * R * S <= kGMaxK, SSQ_E_ARG,
              "%s: K = Cig*R*S = %lld exceeds 65536 (int32 accumulator range)", what,
              (long long)(Cig * R * S));
  SSQ_REQUIRE(Cig <= (1ll << 31) / groups, SSQ_E_ARG, "%s: C = Cig*groups exceeds 2^31", what);
  const GLayout L = glayout(Co, Cig, R, S, groups, planes);
  SSQ_REQUIRE(L.kind != 0, SSQ_E_ARG, "%s: bad geometry", what);
  SSQ_REQUIRE(L.bytes < (1ull << 31), SSQ_E_ARG, "%s: prepared weights exceed 2^31 bytes", what);
  SSQ_REQUIRE(L.kind == 1 ? L.Cp / 16 <= 65535 : groups * L.tiles <= 65535, SSQ_E_ARG,
              "%s: too many channel tiles for one launch", what);
  return SSQ_OK;
}

}  // namespace ssq

using namespace ssq;

extern "C" int ssq_qconv_grouped_kind(int64_t Co, int64_t Cig, int64_t groups) {
  return qg_kind(Co, Cig, groups);
}

extern "C" size_t ssq_qweight_prepared_bytes_grouped(int64_t Co, int64_t Cig, int64_t R, int64_t S,
                                                     int64_t groups) {
  if (R > 7 || S > 7 || Cig > kGMaxK || groups > (1ll << 31)) return 0;
  return glayout(Co, Cig, R, S, groups).bytes;
}

// kcol: the factors of a scaled weight (the COLSCALE kernels), or null: one per column, or,
// per_ci, one per (co, ci) (grouped only: a depthwise weight has no such form); `plain`: the
// groups == 1 entry point an error message points to; wide: the wide forms (kind 2 the two-plane
// blob, kind 1 its int32 blob), factors and |m| up to kQWideMax
static int qweight_prepare_grouped_launch(const char* me, const char* plain, bool colscale,
                                          bool per_ci, bool wide, const void* packed, const float* zp,
                                          const int32_t* kcol, int64_t Co, int64_t Cig, int64_t R,
                                          int64_t S, int64_t groups, int n_bits, int qmin,
                                          void* prepared, uint32_t* bad, ssq_stream_t stream) {
  SSQ_REQUIRE(packed && zp && (kcol || !colscale) && prepared && bad, SSQ_E_ARG,
              "%s: null pointer", me);
  int rc = qrange_ok(me, n_bits, qmin);
  if (rc) return rc;
  SSQ_REQUIRE(colscale || !wide, SSQ_E_ARG, "%s: the wide blob holds a scaled weight", me);
  rc = ggeo_ok(me, plain, -1, Co, Cig, R, S, groups, wide ? 2 : 1);
  if (rc) return rc;
  const GLayout L = glayout(Co, Cig, R, S, groups, wide ? 2 : 1);
  const int lim = wide ? kQWideMax : 127;
  int8_t* base = (int8_t*)prepared;
  const int bs = packed_bits(n_bits);
  const uint32_t RS = (uint32_t)(R * S);
  SSQ_REQUIRE(!per_ci || L.kind == 2, SSQ_E_ARG,
              "%s: a depthwise weight has one input channel per row: no per-(co, ci) scale", me);
  if (L.kind == 1) {
    auto* kernel = colscale ? qweight_prepare_dw_kernel<true> : qweight_prepare_dw_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid_for((int64_t)RS * L.Cp, kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, (const uint8_t*)packed, zp, kcol, lim, bs, qmin,
                       (uint32_t)L.C, RS, (uint32_t)L.Cp, make_fastdiv((uint32_t)L.Cp),
                       (int32_t*)base, bad);
  } else {
    auto* kernel = wide ? qweight_prepare_grouped_kernel<true, true>
                        : (colscale ? qweight_prepare_grouped_kernel<true>
                                    : qweight_prepare_grouped_kernel<false>);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)(groups * L.Cogp + groups)), dim3(kBlock), 0,
                       (hipStream_t)stream, (const uint8_t*)packed, zp,
                       qfactor(kcol, per_ci, (uint32_t)Cig, RS, lim), bs, qmin,
                       (uint32_t)groups, (uint32_t)Cig, (uint32_t)L.Cog, (uint32_t)L.Cogp, RS,
                       (uint32_t)L.Wc, (uint32_t)L.Kp, make_fastdiv((uint32_t)L.Wc),
                       make_fastdiv((uint32_t)L.Cogp), base, base + L.off_mask,
                       (int32_t*)(base + L.off_cwz), (int32_t*)(base + L.off_t), bad);
  }
  return check_launch(me);
}

extern "C" int ssq_qweight_prepare_grouped(const void* packed, const float* zp, int64_t Co,
                                           int64_t Cig, int64_t R, int64_t S, int64_t groups,
                                           int n_bits, int qmin, void* prepared, uint32_t* bad,
                                           ssq_stream_t stream) {
  return qweight_prepare_grouped_launch("ssq_qweight_prepare_grouped", "ssq_qweight_prepare",
                                        false, false, false, packed, zp, nullptr, Co, Cig, R, S, groups,
                                        n_bits, qmin, prepared, bad, stream);
}

extern "C" int ssq_qweight_prepare_grouped_colscale(const void* packed, const float* zp,
                                                    const int32_t* kcol, int64_t Co, int64_t Cig,
                                                    int64_t R, int64_t S, int64_t groups,
                                                    int n_bits, int qmin, void* prepared,
                                                    uint32_t* bad, ssq_stream_t stream) {
  return qweight_prepare_grouped_launch("ssq_qweight_prepare_grouped_colscale",
                                        "ssq_qweight_prepare_colscale", true, false, false, packed, zp,
                                        kcol, Co, Cig, R, S, groups, n_bits, qmin, prepared, bad,
                                        stream);
}

extern "C" int ssq_qweight_prepare_grouped_perci(const void* packed, const float* zp,
                                                 const int32_t* kfac, int64_t Co, int64_t Cig,
                                                 int64_t R, int64_t S, int64_t groups, int n_bits,
                                                 int qmin, void* prepared, uint32_t* bad,
                                                 ssq_stream_t stream) {
  return qweight_prepare_grouped_launch("ssq_qweight_prepare_grouped_perci",
                                        "ssq_qweight_prepare_perci", true, true, false, packed, zp, kfac,
                                        Co, Cig, R, S, groups, n_bits, qmin, prepared, bad, stream);
}

extern "C" size_t ssq_qweight_prepared_bytes_grouped_wide(int64_t Co, int64_t Cig, int64_t R,
                                                          int64_t S, int64_t groups) {
  if (R > 7 || S > 7 || Cig > kGMaxK || groups > (1ll << 31)) return 0;
  return glayout(Co, Cig, R, S, groups, 2).bytes;
}

extern "C" int ssq_qweight_prepare_grouped_wide(const void* packed, const float* zp,
                                                const int32_t* kfac, int per_ci, int64_t Co,
                                                int64_t Cig, int64_t R, int64_t S, int64_t groups,
                                                int n_bits, int qmin, void* prepared, uint32_t* bad,
                                                ssq_stream_t stream) {
  return qweight_prepare_grouped_launch("ssq_qweight_prepare_grouped_wide",
                                        "ssq_qweight_prepare_wide", true, per_ci != 0, true, packed,
                                        zp, kfac, Co, Cig, R, S, groups, n_bits, qmin, prepared,
                                        bad, stream);
}

// y: the fp32 output (ssq_qconv_i8_grouped_fwd) or null with `epi` set (..._codes_fwd); wide: the
// *_grouped_wide_* forms on a blob of ssq_qweight_prepare_grouped_wide
static int qconv_grouped_launch(const char* me, bool wide, const int8_t* codes, const void* prepared,
                                const float* scale, int64_t Nb, int64_t C, int64_t H, int64_t W,
                                int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
                                int64_t groups, float act_zero_point, int act_qmin, int act_qmax,
                                float* y, QEpi* epi, ssq_stream_t stream) {
  SSQ_REQUIRE(codes && prepared && scale && (y || epi), SSQ_E_ARG, "%s: null pointer", me);
  SSQ_REQUIRE(groups >= 2, SSQ_E_ARG,
              "%s: groups = %lld (groups >= 2 only; groups == 1 is ssq_qconv_i8_fwd)", me,
              (long long)groups);
  SSQ_REQUIRE(C >= 1 && C % groups == 0, SSQ_E_ARG,
              "%s: C = %lld is not divisible by groups = %lld", me, (long long)C,
              (long long)groups);
  const int64_t Cig = C / groups;
  int rc = ggeo_ok(me, "ssq_qconv_i8_fwd", C, Co, Cig, R, S, groups, wide ? 2 : 1);
  if (rc) return rc;
  SSQ_REQUIRE(Nb >= 1 && H >= 1 && W >= 1 && stride >= 1 && pad >= 0 && H + 2 * pad >= R &&
                  W + 2 * pad >= S,
              SSQ_E_ARG, "%s: bad geometry", me);
  rc = qquant_ok(me, "activation ", nullptr, act_zero_point, act_qmin, act_qmax);
  if (rc) return rc;
  const GLayout L = glayout(Co, Cig, R, S, groups, wide ? 2 : 1);
  const int64_t OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
  SSQ_REQUIRE(Nb * H * W * L.Cp < (1ll << 31) && Nb * OH * OW * Co < (1ll << 31), SSQ_E_ARG,
              "%s: tensor exceeds 2^31 elements", me);
  const int ca = act_qmin + 128, za = (int)act_zero_point;
  const int8_t* base = (const int8_t*)prepared;
  if (epi) {
    epi->Cpo = (uint32_t)rup(Co, 16);
    SSQ_REQUIRE(Nb * OH * OW * (int64_t)epi->Cpo < (1ll << 31), SSQ_E_ARG,
                "%s: tensor exceeds 2^31 elements", me);
  }
  if (L.kind == 1) {
    QDwGeo g;
    g.M = (uint32_t)(Nb * OH * OW);
    g.P = (uint32_t)(OH * OW);
    g.OW = (uint32_t)OW;
    g.H = (uint32_t)H;
    g.W = (uint32_t)W;
    g.C = (uint32_t)C;
    g.Cp = (uint32_t)L.Cp;
    g.R = (uint32_t)R;
    g.S = (uint32_t)S;
    g.stride = (int)stride;
    g.pad = (int)pad;
    g.az = ca - za;
    g.padv = za - ca;   // a padded tap: (q_a - z_a) = 0
    g.div_p = make_fastdiv(g.P);
    g.div_ow = make_fastdiv(g.OW);
    // enough workgroups to fill the device, as few chunk runs per pixel block as that allows
    const uint32_t pixblocks = (g.M + kBlock - 1) / kBlock;
    g.nch = (uint32_t)(L.Cp / 16);
    const uint32_t runs = min(g.nch, max(1u, (kDwBlocks + pixblocks - 1) / pixblocks));
    g.per = (g.nch + runs - 1) / runs;
    const dim3 grid(pixblocks, (g.nch + g.per - 1) / g.per);
    const int32_t* wc = (const int32_t*)base;
#define SSQ_DW_LAUNCH(KS)                                                                       \
  do {                                                                                          \
    if (epi)                                                                                    \
      hipLaunchKernelGGL((qconv_dw_kernel<KS, true>), grid, dim3(kBlock), 0, (hipStream_t)stream, \
                         codes, wc, scale, g, *epi);                                            \
    else                                                                                        \
      hipLaunchKernelGGL((qconv_dw_kernel<KS, false>), grid, dim3(kBlock), 0,                   \
                         (hipStream_t)stream, codes, wc, scale, g, y);                          \
  } while (0)
    if (R == S && R == 3) SSQ_DW_LAUNCH(3);
    else if (R == S && R == 5) SSQ_DW_LAUNCH(5);
    else if (R == S && R == 7) SSQ_DW_LAUNCH(7);
    else SSQ_DW_LAUNCH(0);
#undef SSQ_DW_LAUNCH
    return check_launch(me);
  }
  QGConvGeo g;
  g.M = (uint32_t)(Nb * OH * OW);
  g.P = (uint32_t)(OH * OW);
  g.OW = (uint32_t)OW;
  g.H = (uint32_t)H;
  g.W = (uint32_t)W;
  g.Cp = (uint32_t)L.Cp;
  g.Co = (uint32_t)Co;
  g.Cig = (uint32_t)Cig;
  g.Cog = (uint32_t)L.Cog;
  g.Cogp = (uint32_t)L.Cogp;
  g.Wc = (uint32_t)L.Wc;
  g.Kp = (uint32_t)L.Kp;
  g.RS = (uint32_t)(R * S);
  g.S = (uint32_t)S;
  g.tiles = (uint32_t)L.tiles;
  g.stride = (int)stride;
  g.pad = (int)pad;
  g.az = ca - za;
  g.padv = za - ca;   // a padded tap: (q_a - z_a) = 0
  g.div_p = make_fastdiv(g.P);
  g.div_ow = make_fastdiv(g.OW);
  g.div_wc = make_fastdiv(g.Wc);
  g.div_s = make_fastdiv(g.S);
  g.div_tiles = make_fastdiv(g.tiles);
  const dim3 grid((g.M + kGT - 1) / kGT, (uint32_t)(groups * L.tiles));
  const int8_t* masks = base + L.off_mask;
  const int32_t* cwz = (const int32_t*)(base + L.off_cwz);
  const int32_t* tt = (const int32_t*)(base + L.off_t);
  if (epi) {
    auto* kernel = wide ? qconv_grouped_kernel<true, true> : qconv_grouped_kernel<true>;
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, codes, base, masks, cwz,
                       tt, scale, g, *epi);
    return check_launch(me);
  }
  auto* kernel = wide ? qconv_grouped_kernel<false, true> : qconv_grouped_kernel<false>;
  hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, codes, base, masks, cwz,
                     tt, scale, g, y);
  return check_launch(me);
}

extern "C" int ssq_qconv_i8_grouped_fwd(const int8_t* codes, const void* prepared,
                                        const float* scale, int64_t Nb, int64_t C, int64_t H,
                                        int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride,
                                        int64_t pad, int64_t groups, float act_zero_point,
                                        int act_qmin, int act_qmax, float* y, ssq_stream_t stream) {
  SSQ_REQUIRE(y, SSQ_E_ARG, "ssq_qconv_i8_grouped_fwd: null pointer");
  return qconv_grouped_launch("ssq_qconv_i8_grouped_fwd", false, codes, prepared, scale, Nb, C, H, W, Co,
                              R, S, stride, pad, groups, act_zero_point, act_qmin, act_qmax, y,
                              nullptr, stream);
}

extern "C" int ssq_qconv_i8_grouped_codes_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t C, int64_t H,
    int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t groups,
    float act_zero_point, int act_qmin, int act_qmax, const float* bias, const float* gamma,
    const float* phi, int act, float out_delta, float out_zero_point, int out_qmin, int out_qmax,
    int8_t* out_codes, uint32_t* bad, ssq_stream_t stream) {
  const char* me = "ssq_qconv_i8_grouped_codes_fwd";
  QEpi e;
  const int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin,
                           out_qmax, out_codes, bad, &e);
  if (rc) return rc;
  return qconv_grouped_launch(me, false, codes, prepared, scale, Nb, C, H, W, Co, R, S, stride,
                              pad, groups, act_zero_point, act_qmin, act_qmax, nullptr, &e, stream);
}

// The wide forms: the grouped forms' arguments, checks and epilogues on a blob of
// ssq_qweight_prepare_grouped_wide (kind 2: two int8 digit planes, 2 nf MFMAs per k step;
// kind 1: K25 on its int32 blob).
extern "C" int ssq_qconv_i8_grouped_wide_fwd(const int8_t* codes, const void* prepared,
                                             const float* scale, int64_t Nb, int64_t C, int64_t H,
                                             int64_t W, int64_t Co, int64_t R, int64_t S,
                                             int64_t stride, int64_t pad, int64_t groups,
                                             float act_zero_point, int act_qmin, int act_qmax,
                                             float* y, ssq_stream_t stream) {
  SSQ_REQUIRE(y, SSQ_E_ARG, "ssq_qconv_i8_grouped_wide_fwd: null pointer");
  return qconv_grouped_launch("ssq_qconv_i8_grouped_wide_fwd", true, codes, prepared, scale, Nb, C,
                              H, W, Co, R, S, stride, pad, groups, act_zero_point, act_qmin,
                              act_qmax, y, nullptr, stream);
}

extern "C" int ssq_qconv_i8_grouped_wide_codes_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t C, int64_t H,
    int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t groups,
    float act_zero_point, int act_qmin, int act_qmax, const float* bias, const float* gamma,
    const float* phi, int act, float out_delta, float out_zero_point, int out_qmin, int out_qmax,
    int8_t* out_codes, uint32_t* bad, ssq_stream_t stream) {
  const char* me = "ssq_qconv_i8_grouped_wide_codes_fwd";
  QEpi e;
  const int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin,
                           out_qmax, out_codes, bad, &e);
  if (rc) return rc;
  return qconv_grouped_launch(me, true, codes, prepared, scale, Nb, C, H, W, Co, R, S, stride, pad,
                              groups, act_zero_point, act_qmin, act_qmax, nullptr, &e, stream);
}
