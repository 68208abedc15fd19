// K31: the stem conv on the fp32 MFMA, leaving as fp32 NCHW or as K21's stored codes
// (quant/integer.py, fused_stem).
//
// Contract (both forms): for an fp32 NCHW image x and an fp32 OIHW weight W, stride (sh, sw),
// padding (ph, pw), dilation 1, groups 1,
//     y[n, co, oh, ow] = acc_K,  acc_0 = +0.0f,  acc_{k+1} = fmaf(x_k, W[co, k], acc_k),
// k over (ci, r, s) in the memory order of W[co], x_k the pixel under tap k or +0.0f outside the
// image: one rounding per tap and no other.  v_mfma_f32_16x16x4_f32 is that chain over its four
// k, C first, so the walk of the k steps in ascending order is the contract itself, and the host
// reproduces it bit for bit (tests/test_qinfer_stemconv_host.py, chain_conv).  The last step's
// padded k carry -0 in the weight and +0 in the pixel (SLayout, qinfer_layout.h).
//
// ssq_stem_conv_fwd stores acc_K; ssq_stem_conv_codes_fwd runs qepi_code_y (qinfer_epi.h) on it,
// the function K27 runs on the stored fp32 value, so its bytes are K27's of the fp32 form.
//
// One workgroup: TH rows x 32 columns of one image's output plane (TH in {2, 4, 8}, one wave per
// two rows) and up to 16 * NCH output channels.  The input patch under the tile is staged once in
// LDS, zero outside the image; along an axis whose stride exceeds the kernel the windows are
// disjoint and the patch keeps only them (LDS index o * K + tap instead of o * stride + tap), so
// its size is bounded by the tile, not by the stride.  The MFMA's A operand is the weight
// (row = channel), its B operand the pixels (column = pixel): a lane's four results are four
// consecutive channels of one pixel, one dword of the NHWC code row.
#include <type_traits>

#include "ssq_common.h"
#include "qinfer_epi.h"
#include "qinfer_layout.h"

namespace ssq {

typedef int i32x4s __attribute__((ext_vector_type(4)));

constexpr int kStemTW = 32;                  // tile columns
constexpr int kStemMaxTH = 8;                // tile rows at most (kBlock / kStemTW)
constexpr size_t kStemMaxLds = 64 * 1024;

struct StemGeo {
  uint32_t Ci, H, W, Co, OH, OW, sh, sw;
  int ph, pw;
  uint32_t R, S, K, Kp, nch;        // nch: 16-channel chunks of the blob (Cop / 16)
  uint32_t TH, eh, ew;              // tile rows; LDS units per output row / column
  uint32_t PH, PW, PWs;             // patch rows, columns, row stride (odd)
  uint32_t tiles_h, tiles_w;
  FastDiv div_tw, div_th, div_pws, div_ph, div_s, div_rs;
};

// the image coordinate of patch index l along one axis (tile origin o0, stride st, kernel kk)
__device__ __forceinline__ int stem_coord(uint32_t l, uint32_t o0, uint32_t st, uint32_t kk,
                                          int pad) {
  if (st <= kk) return (int)(o0 * st + l) - pad;
  const uint32_t o = l / kk;
  return (int)((o0 + o) * st + (l - o * kk)) - pad;
}

template <int NCH, bool CODES>
__global__ __launch_bounds__(kBlock) void stem_conv_kernel(
    const float* __restrict__ x, const float* __restrict__ wp, StemGeo g,
    typename std::conditional<CODES, QEpi, float* __restrict__>::type y) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int* koff = (int*)smem;            // [Kp + 8]: tap k's offset inside the patch, 0 from K on
  float* patch = smem + g.Kp + 8;    // [Ci][PH][PWs]; then the code tile [TH * 32][16 * NCH]
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const uint32_t nthr = g.TH * kStemTW;
  const uint32_t q1 = fdiv(blockIdx.x, g.div_tw), tw = blockIdx.x - q1 * g.tiles_w;
  const uint32_t n = fdiv(q1, g.div_th), th = q1 - n * g.tiles_h;
  const uint32_t oh0 = th * g.TH, ow0 = tw * kStemTW;

  for (uint32_t k = tid; k < g.Kp + 8; k += nthr) {
    int o = 0;
    if (k < g.K) {
      const uint32_t ci = fdiv(k, g.div_rs), rem = k - ci * g.R * g.S;
      const uint32_t r = fdiv(rem, g.div_s), s = rem - r * g.S;
      o = (int)((ci * g.PH + r) * g.PWs + s);
    }
    koff[k] = o;
  }
  // the patch, four loads in flight per thread
  const uint32_t total = g.Ci * g.PH * g.PWs;
  const float* xn = x + (size_t)n * g.Ci * g.H * g.W;
  for (uint32_t i0 = tid; i0 < total; i0 += 4 * nthr) {
    float v[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t i = i0 + u * nthr;
      const uint32_t row = fdiv(i, g.div_pws), lc = i - row * g.PWs;
      const uint32_t ci = fdiv(row, g.div_ph), lr = row - ci * g.PH;
      const int gh = stem_coord(lr, oh0, g.sh, g.R, g.ph);
      const int gw = stem_coord(lc, ow0, g.sw, g.S, g.pw);
      ok[u] = i < total && lc < g.PW && gh >= 0 && gh < (int)g.H && gw >= 0 && gw < (int)g.W;
      // an outside position reads element 0 of the image and is replaced: no load leaves the
      // tensor
      const size_t at = ok[u] ? ((size_t)ci * g.H + (uint32_t)gh) * g.W + (uint32_t)gw : 0;
      v[u] = xn[at];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t i = i0 + u * nthr;
      if (i < total) patch[i] = ok[u] ? v[u] : 0.0f;
    }
  }
  __syncthreads();

  // fragment maps: lane l holds W[16 c + (l & 15)][4 t + (l >> 4)] and pixel (l & 15) of pixel
  // group gi at k = 4 t + (l >> 4); its results are channels 16 c + 4 (l >> 4) + {0..3} of
  // pixel (l & 15)
  const uint32_t fj = lane & 15, fq = lane >> 4;
  const uint32_t c0 = blockIdx.y * NCH;
  uint32_t pbase[4];
#pragma unroll
  for (int gi = 0; gi < 4; ++gi) {
    const uint32_t row = 2 * wave + (gi >> 1), col = (gi & 1) * 16 + fj;
    pbase[gi] = row * g.eh * g.PWs + col * g.ew;
  }
  const float* wl[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    // a chunk past the blob's last reads the last again; its results are not stored
    const uint32_t cc = c0 + c < g.nch ? c0 + c : g.nch - 1;
    wl[c] = wp + (size_t)cc * 64 + lane;
  }
  const size_t wstep = (size_t)g.nch * 64;
  f32x4 acc[4][NCH];
#pragma unroll
  for (int gi = 0; gi < 4; ++gi)
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[gi][c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  // Step t's operands are loaded during step t - 1's MFMAs and its patch offset during step
  // t - 2's: the loads are issued ahead of the MFMAs (the scheduling barrier keeps them there)
  // and waited for behind them.  A k from K on has offset 0 (an in-bounds read) and enters as +0.
  const uint32_t nsteps = g.Kp / 4;
  float a[NCH], b[4];
#pragma unroll
  for (int c = 0; c < NCH; ++c) a[c] = wl[c][0];
  {
    const int ko = koff[fq];
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
      const float v = patch[pbase[gi] + ko];
      b[gi] = fq < g.K ? v : 0.0f;
    }
  }
  int ko_n = koff[4 + fq];
  for (uint32_t t = 0; t < nsteps; ++t) {
    const uint32_t kn = 4 * (t + 1) + fq;
    const uint32_t tn = t + 1 < nsteps ? t + 1 : t;
    float an[NCH], bn[4];
#pragma unroll
    for (int c = 0; c < NCH; ++c) an[c] = wl[c][(size_t)tn * wstep];
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) bn[gi] = patch[pbase[gi] + ko_n];
    const int ko_n2 = koff[kn + 4];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int gi = 0; gi < 4; ++gi)
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        acc[gi][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[gi], acc[gi][c], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NCH; ++c) a[c] = an[c];
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) b[gi] = kn < g.K ? bn[gi] : 0.0f;
    ko_n = ko_n2;
  }

  if constexpr (CODES) {
    const QEpi& e = y;
    uint32_t nbad = 0;
    int8_t* stage = (int8_t*)patch;
    __syncthreads();   // every wave's last patch read is done: the code tile takes its place
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
      const uint32_t row = 2 * wave + (gi >> 1), col = (gi & 1) * 16 + fj;
      const bool pval = oh0 + row < g.OH && ow0 + col < g.OW;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        int cd[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t co = (c0 + c) * 16 + fq * 4 + r;
          cd[r] = (pval && co < g.Co) ? qepi_code_y(acc[gi][c][r], co, e, nbad) : 0;
        }
        *(int*)(stage + ((row * kStemTW + col) * NCH + c) * 16 + fq * 4) =
            qepi_pack4(cd[0], cd[1], cd[2], cd[3]);
      }
    }
    __syncthreads();
    // thread (pixel, chunk) stores the 16 channels of one chunk of one pixel
    for (uint32_t u = tid; u < nthr * NCH; u += nthr) {
      const uint32_t p = u / NCH, c = u - p * NCH;
      const uint32_t oh = oh0 + p / kStemTW, ow = ow0 + p % kStemTW;
      if (oh < g.OH && ow < g.OW && c0 + c < g.nch)
        *(i32x4s*)(e.out + (((size_t)n * g.OH + oh) * g.OW + ow) * e.Cpo + (c0 + c) * 16) =
            *(const i32x4s*)(stage + (size_t)u * 16);
    }
    qepi_count(nbad, e.bad);
  } else {
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
      const uint32_t oh = oh0 + 2 * wave + (gi >> 1), ow = ow0 + (gi & 1) * 16 + fj;
      if (oh >= g.OH || ow >= g.OW) continue;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t co = (c0 + c) * 16 + fq * 4 + r;
          if (co < g.Co) y[(((size_t)n * g.Co + co) * g.OH + oh) * g.OW + ow] = acc[gi][c][r];
        }
    }
  }
}

// fp32 OIHW -> SLayout
__global__ __launch_bounds__(kBlock) void stem_weight_prepare_kernel(const float* __restrict__ w,
                                                                     float* __restrict__ out,
                                                                     uint32_t Co, uint32_t K,
                                                                     uint32_t nch, uint32_t total) {
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
    const uint32_t j = i & 15, kk = (i >> 4) & 3, tc = i >> 6;
    const uint32_t t = tc / nch, c = tc - t * nch;
    const uint32_t co = c * 16 + j, k = 4 * t + kk;
    out[i] = k >= K ? -0.0f : (co < Co ? w[(size_t)co * K + k] : 0.0f);
  }
}

// The geometry both forms share, checked and gathered; the launch's tile rows and LDS bytes.
static int stem_geo(const char* me, const float* x, const void* prepared, size_t prepared_bytes,
                    int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S,
                    int64_t sh, int64_t sw, int64_t ph, int64_t pw, StemGeo* g, dim3* grid,
                    size_t* lds, int* nchunks) {
  SSQ_REQUIRE(x && prepared, SSQ_E_ARG, "%s: null pointer", me);
  const SLayout L = slayout(Co, Ci, R, S);
  SSQ_REQUIRE(L.bytes, SSQ_E_ARG,
              "%s: outside the stem geometry (1 <= Ci <= 4, 1 <= R, S <= 7, Co >= 1)", me);
  SSQ_REQUIRE(prepared_bytes >= L.bytes, SSQ_E_ARG, "%s: prepared blob of %zu bytes, %zu needed",
              me, prepared_bytes, L.bytes);
  SSQ_REQUIRE(Nb >= 1 && H >= 1 && W >= 1 && sh >= 1 && sw >= 1 && sh < (1ll << 24) &&
                  sw < (1ll << 24),
              SSQ_E_ARG, "%s: bad geometry (sizes and strides >= 1)", me);
  SSQ_REQUIRE(ph >= 0 && ph < R && pw >= 0 && pw < S, SSQ_E_ARG,
              "%s: padding (%lld, %lld) not below the kernel (%lld, %lld)", me, (long long)ph,
              (long long)pw, (long long)R, (long long)S);
  SSQ_REQUIRE(H + 2 * ph >= R && W + 2 * pw >= S, SSQ_E_ARG, "%s: empty output", me);
  const int64_t OH = (H + 2 * ph - R) / sh + 1, OW = (W + 2 * pw - S) / sw + 1;
  SSQ_REQUIRE(Nb * Ci * H * W < (1ll << 31) && Nb * OH * OW * L.Cop < (1ll << 31), SSQ_E_ARG,
              "%s: tensor exceeds 2^31 elements", me);
  const int64_t tiles_w = (OW + kStemTW - 1) / kStemTW;
  const int nch = (int)(L.Cop / 16);
  const int NCH = nch >= 3 ? 4 : nch;
  const int64_t ctiles = (nch + NCH - 1) / NCH;
  const int64_t eh = sh < R ? sh : R, ew = sw < S ? sw : S;
  const int64_t PW = ew * (kStemTW - 1) + S, PWs = PW | 1;
  // the tallest tile that leaves two workgroups per compute unit of a 256-CU part and fits LDS
  int64_t TH = kStemMaxTH, PH = 0;
  size_t bytes = 0;
  for (;; TH /= 2) {
    PH = eh * (TH - 1) + R;
    const size_t patch = (size_t)(Ci * PH * PWs) * 4, tile = (size_t)(TH * kStemTW * 16 * NCH);
    bytes = (size_t)(L.Kp + 8) * 4 + (patch > tile ? patch : tile);
    const int64_t wgs = Nb * ((OH + TH - 1) / TH) * tiles_w * ctiles;
    if (TH == 2 || (bytes <= kStemMaxLds && wgs >= 512)) break;
  }
  SSQ_REQUIRE(bytes <= kStemMaxLds, SSQ_E_ARG, "%s: patch exceeds LDS", me);
  const int64_t tiles_h = (OH + TH - 1) / TH;
  SSQ_REQUIRE(Nb * tiles_h * tiles_w < (1ll << 31) && ctiles < 65536, SSQ_E_ARG,
              "%s: grid too large", me);
  *g = {(uint32_t)Ci, (uint32_t)H,  (uint32_t)W,  (uint32_t)Co, (uint32_t)OH, (uint32_t)OW,
        (uint32_t)sh, (uint32_t)sw, (int)ph,      (int)pw,      (uint32_t)R,  (uint32_t)S,
        (uint32_t)L.K, (uint32_t)L.Kp, (uint32_t)nch, (uint32_t)TH, (uint32_t)eh, (uint32_t)ew,
        (uint32_t)PH, (uint32_t)PW, (uint32_t)PWs, (uint32_t)tiles_h, (uint32_t)tiles_w,
        make_fastdiv((uint32_t)tiles_w), make_fastdiv((uint32_t)tiles_h),
        make_fastdiv((uint32_t)PWs), make_fastdiv((uint32_t)PH), make_fastdiv((uint32_t)S),
        make_fastdiv((uint32_t)(R * S))};
  *grid = dim3((unsigned)(Nb * tiles_h * tiles_w), (unsigned)ctiles);
  *lds = bytes;
  *nchunks = NCH;
  return SSQ_OK;
}

template <bool CODES, typename Y>
static void stem_launch(int NCH, dim3 grid, size_t lds, hipStream_t stream, const float* x,
                        const float* wp, const StemGeo& g, Y y) {
  const dim3 block(g.TH * kStemTW);
  if (NCH == 4)
    hipLaunchKernelGGL((stem_conv_kernel<4, CODES>), grid, block, lds, stream, x, wp, g, y);
  else if (NCH == 2)
    hipLaunchKernelGGL((stem_conv_kernel<2, CODES>), grid, block, lds, stream, x, wp, g, y);
  else
    hipLaunchKernelGGL((stem_conv_kernel<1, CODES>), grid, block, lds, stream, x, wp, g, y);
}

}  // namespace ssq

using namespace ssq;

extern "C" size_t ssq_stem_weight_prepared_bytes(int64_t Co, int64_t Ci, int64_t R, int64_t S) {
  return slayout(Co, Ci, R, S).bytes;
}

extern "C" int ssq_stem_weight_prepare(const float* w, int64_t Co, int64_t Ci, int64_t R,
                                       int64_t S, void* prepared, ssq_stream_t stream) {
  const char* me = "ssq_stem_weight_prepare";
  SSQ_REQUIRE(w && prepared, SSQ_E_ARG, "%s: null pointer", me);
  const SLayout L = slayout(Co, Ci, R, S);
  SSQ_REQUIRE(L.bytes && L.bytes / 4 < (1ull << 31), SSQ_E_ARG,
              "%s: outside the stem geometry (1 <= Ci <= 4, 1 <= R, S <= 7, Co >= 1)", me);
  const uint32_t total = (uint32_t)(L.bytes / 4);
  hipLaunchKernelGGL(stem_weight_prepare_kernel, dim3(grid_for(total, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, w, (float*)prepared, (uint32_t)Co, (uint32_t)L.K,
                     (uint32_t)(L.Cop / 16), total);
  return check_launch(me);
}

extern "C" int ssq_stem_conv_fwd(const float* x, const void* prepared, size_t prepared_bytes,
                                 int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                 int64_t R, int64_t S, int64_t stride_h, int64_t stride_w,
                                 int64_t pad_h, int64_t pad_w, float* y, ssq_stream_t stream) {
  const char* me = "ssq_stem_conv_fwd";
  SSQ_REQUIRE(y, SSQ_E_ARG, "%s: null pointer", me);
  StemGeo g;
  dim3 grid;
  size_t lds;
  int NCH;
  const int rc = stem_geo(me, x, prepared, prepared_bytes, Nb, Ci, H, W, Co, R, S, stride_h,
                          stride_w, pad_h, pad_w, &g, &grid, &lds, &NCH);
  if (rc) return rc;
  SSQ_REQUIRE(Nb * Co * (int64_t)g.OH * g.OW < (1ll << 31), SSQ_E_ARG,
              "%s: tensor exceeds 2^31 elements", me);
  stem_launch<false>(NCH, grid, lds, (hipStream_t)stream, x, (const float*)prepared, g, y);
  return check_launch(me);
}

extern "C" int ssq_stem_conv_codes_fwd(const float* x, const void* prepared, size_t prepared_bytes,
                                       int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                       int64_t R, int64_t S, int64_t stride_h, int64_t stride_w,
                                       int64_t pad_h, int64_t pad_w, const float* bias,
                                       const float* gamma, const float* phi, int act,
                                       float out_delta, float out_zero_point, int out_qmin,
                                       int out_qmax, int8_t* out_codes, uint32_t* bad,
                                       ssq_stream_t stream) {
  const char* me = "ssq_stem_conv_codes_fwd";
  QEpi e;
  int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin, out_qmax,
                     out_codes, bad, &e);
  if (rc) return rc;
  StemGeo g;
  dim3 grid;
  size_t lds;
  int NCH;
  rc = stem_geo(me, x, prepared, prepared_bytes, Nb, Ci, H, W, Co, R, S, stride_h, stride_w, pad_h,
                pad_w, &g, &grid, &lds, &NCH);
  if (rc) return rc;
  e.Cpo = g.nch * 16;
  stem_launch<true>(NCH, grid, lds, (hipStream_t)stream, x, (const float*)prepared, g, e);
  return check_launch(me);
}
