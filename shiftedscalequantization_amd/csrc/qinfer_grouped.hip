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
// kind 1 holds m in its int32 blob as it stands, with column factors and per-channel ones
// (ssq_qweight_prepare_grouped_chfac; a depthwise row has no per-(co, ci) form):
// |a| * |m| < 2^9 * 2^14 keeps __mul24 exact and |I| <= 49 * 255 * 16319 < 2^31 stays inside
// the int32 accumulator, but |I| may pass 2^24, so fp32(I) may round there: that is the
// contract's one conversion, round to nearest even, as K23's -- it is exact for the int8 blobs only.
//
// Per-channel act grids (a hard shifted-scale act quantizer's d[c] = fp32(delta * s_k(c))).  Read:
// the conv kernels are unchanged, the grid's integer k_a[ci] is multiplied into the operand by K24
// (kind 2 as per-(co, ci) factors k_a[g(co) * Cig + ci], kind 1 as the per-channel factors above).
// Emitted (ssq_qconv_i8_grouped_codes_chq_fwd): the CHQ instantiations of the two kernel templates
// (qinfer_grouped_kernels.h, built in qinfer_grouped_chq.hip) are the code-emitting kernels with the
// output scale out_dch[co] for the scalar one, fetched once per chunk (K25) or per lane (K26).
#include "qinfer_grouped_kernels.h"
#include "qinfer_prepare.h"

namespace ssq {

constexpr uint32_t kDwBlocks = 2048;   // workgroups K25 aims for: 8 per CU

// ---------------------------------------------------------------- K24 weight prepare
// Plain and COLSCALE as K22 (qinfer.hip): COLSCALE stores the centred integer
// m = (q - z_w[co]) * k, k the QFactor's entry of the element (qinfer_prepare.h): a column scale's
// k[j], j = (ci, r, s) within the group (J = Cig*R*S, shared by all groups), or a per-(co, ci)
// scale's k[co * Cig + ci]; *bad also counts what qscaled() counts.
//
// depthwise: one thread per (tap, padded channel) of K25's centred int32 blob [R*S][Cp],
// wc = q - z_w[c]; COLSCALE multiplies it by kcol[tap], factors and |m| up to `lim` (127, or
// kQWideMax for the wide form).  CHFAC (ssq_qweight_prepare_grouped_chfac): a per-channel factor
// kch[c] beside it, m = (q - z_w[c]) * kcol[tap] * kch[c] (kcol null: 1) -- a shifted act grid's
// k_a[c], which a depthwise row cannot take as a per-(co, ci) factor; each factor and each product
// is held to `lim` (factors are >= 1, so a product that leaves it on the way has left it at the end)
template <bool COLSCALE, bool CHFAC = false>
__global__ __launch_bounds__(kBlock) void qweight_prepare_dw_kernel(
    const uint8_t* __restrict__ packed, const float* __restrict__ zp,
    const int32_t* __restrict__ kcol, const int32_t* __restrict__ kch, int lim, int bs, int qmin,
    uint32_t C, uint32_t RS, uint32_t Cp, FastDiv div_cp, int32_t* __restrict__ wc,
    uint32_t* __restrict__ bad) {
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
      if constexpr (CHFAC) v = qscaled(v, kch[c], lim, nbad);   // |v| <= lim, kch <= lim: < 2^31
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
// blob, kind 1 its int32 blob), factors and |m| up to kQWideMax; kch: a depthwise weight's
// per-channel factors beside kcol (ssq_qweight_prepare_grouped_chfac), or null
static int qweight_prepare_grouped_launch(const char* me, const char* plain, bool colscale,
                                          bool per_ci, bool wide, const void* packed, const float* zp,
                                          const int32_t* kcol, int64_t Co, int64_t Cig, int64_t R,
                                          int64_t S, int64_t groups, int n_bits, int qmin,
                                          void* prepared, uint32_t* bad, ssq_stream_t stream,
                                          const int32_t* kch = nullptr) {
  SSQ_REQUIRE(packed && zp && (kcol || !colscale) && prepared && bad, SSQ_E_ARG,
              "%s: null pointer", me);
  int rc = qrange_ok(me, n_bits, qmin);
  if (rc) return rc;
  SSQ_REQUIRE(colscale || kch || !wide, SSQ_E_ARG, "%s: the wide blob holds a scaled weight", me);
  rc = ggeo_ok(me, plain, -1, Co, Cig, R, S, groups, wide ? 2 : 1);
  if (rc) return rc;
  const GLayout L = glayout(Co, Cig, R, S, groups, wide ? 2 : 1);
  const int lim = wide ? kQWideMax : 127;
  int8_t* base = (int8_t*)prepared;
  const int bs = packed_bits(n_bits);
  const uint32_t RS = (uint32_t)(R * S);
  SSQ_REQUIRE(!per_ci || L.kind == 2, SSQ_E_ARG,
              "%s: a depthwise weight has one input channel per row: no per-(co, ci) scale", me);
  SSQ_REQUIRE(!kch || L.kind == 1, SSQ_E_ARG,
              "%s: per-channel factors go with a depthwise weight (a grouped one takes them per "
              "(co, ci): ssq_qweight_prepare_grouped_perci)", me);
  if (L.kind == 1) {
    auto* kernel = kch ? (colscale ? qweight_prepare_dw_kernel<true, true>
                                   : qweight_prepare_dw_kernel<false, true>)
                       : (colscale ? qweight_prepare_dw_kernel<true> : qweight_prepare_dw_kernel<false>);
    hipLaunchKernelGGL(kernel, dim3(grid_for((int64_t)RS * L.Cp, kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, (const uint8_t*)packed, zp, kcol, kch, lim, bs, qmin,
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

// A depthwise weight (ssq_qconv_grouped_kind 1) with per-channel factors kch[C] -- a shifted act
// grid's k_a[c] -- beside its column factors kcol[R*S], or alone (kcol null):
// m[tap][c] = (q - z_w[c]) * kcol[tap] * kch[c] in K25's int32 blob; wide: factors and |m| up to
// kQWideMax for 127, as ssq_qweight_prepare_grouped_wide holds a depthwise weight
extern "C" int ssq_qweight_prepare_grouped_chfac(const void* packed, const float* zp,
                                                 const int32_t* kcol, const int32_t* kch, int wide,
                                                 int64_t Co, int64_t Cig, int64_t R, int64_t S,
                                                 int64_t groups, int n_bits, int qmin,
                                                 void* prepared, uint32_t* bad, ssq_stream_t stream) {
  const char* me = "ssq_qweight_prepare_grouped_chfac";
  SSQ_REQUIRE(kch, SSQ_E_ARG, "%s: null pointer (kch)", me);
  return qweight_prepare_grouped_launch(me, "ssq_qweight_prepare_colscale", kcol != nullptr, false,
                                        wide != 0, packed, zp, kcol, Co, Cig, R, S, groups, n_bits,
                                        qmin, prepared, bad, stream, kch);
}

// y: the fp32 output (ssq_qconv_i8_grouped_fwd) or null with `epi` set (..._codes_fwd); wide: the
// *_grouped_wide_* forms on a blob of ssq_qweight_prepare_grouped_wide; chq: `epi` is a QEpiCh, the
// per-channel forms (ssq_qconv_i8_grouped_codes_chq_fwd)
static int qconv_grouped_launch(const char* me, bool wide, const int8_t* codes, const void* prepared,
                                const float* scale, int64_t Nb, int64_t C, int64_t H, int64_t W,
                                int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
                                int64_t groups, float act_zero_point, int act_qmin, int act_qmax,
                                float* y, QEpi* epi, ssq_stream_t stream, bool chq = false) {
  SSQ_REQUIRE(codes && prepared && scale && (y || epi), SSQ_E_ARG, "%s: null pointer", me);
  SSQ_REQUIRE(!chq || epi, SSQ_E_ARG, "%s: a per-channel grid goes with the code-emitting form", me);
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
    if (chq) {
      qconv_dw_chq_launch(R, S, grid, (hipStream_t)stream, codes, wc, scale, g,
                          *static_cast<QEpiCh*>(epi));
      return check_launch(me);
    }
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
  if (chq) {
    qconv_grouped_chq_launch(wide, grid, (hipStream_t)stream, codes, base, masks, cwz, tt, scale, g,
                             *static_cast<QEpiCh*>(epi));
    return check_launch(me);
  }
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

// The code-emitting grouped and depthwise convs on a per-channel output grid: the arguments of
// ssq_qconv_i8_grouped_codes_fwd with out_dch[Co] in the place of the scalar out_delta (null is
// refused: a per-tensor grid is the scalar entry points'), and `wide` in front of it: 0 a blob of
// the int8 prepares, 1 one of ssq_qweight_prepare_grouped_wide (for a depthwise weight the same
// kernel either way).  *bad also counts, once per launch, the out_dch entries that are no scale.
extern "C" int ssq_qconv_i8_grouped_codes_chq_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t C, int64_t H,
    int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t groups,
    float act_zero_point, int act_qmin, int act_qmax, const float* bias, const float* gamma,
    const float* phi, int act, int wide, const float* out_dch, float out_zero_point, int out_qmin,
    int out_qmax, int8_t* out_codes, uint32_t* bad, ssq_stream_t stream) {
  const char* me = "ssq_qconv_i8_grouped_codes_chq_fwd";
  QEpiCh e;
  const int rc = qepi_init_ch(me, bias, gamma, phi, act, out_dch, 0.0f, false, out_zero_point,
                              out_qmin, out_qmax, out_codes, bad, &e);
  if (rc) return rc;
  return qconv_grouped_launch(me, wide != 0, codes, prepared, scale, Nb, C, H, W, Co, R, S, stride,
                              pad, groups, act_zero_point, act_qmin, act_qmax, nullptr, &e, stream,
                              true);
}
