// K32: the stem conv of a uint8 image on the int8 MFMA, leaving as fp32 NCHW or as K21's stored
// codes (quant/integer.py, image_u8).
//
// Contract ("uint8 stem (K32)"; include/ssq.h).  The image is x = (u/255 - mean_c)/std_c
// with u in 0..255, the weight (q_w - z_w[co]) * d[co, c].  Per (pixel, co) and input channel c,
// over the taps of the window that lie inside the image,
//     B_c = sum (q_w - z_w[co])          A_c = sum (q_w - z_w[co]) * u
// are exact integers (a padded tap stands for x = 0 and enters neither), and
//     t_c = fp32(A_c) - M[c] * fp32(B_c)       M[c] = fp32(255 * mean[c])
//     y   = t_0 * s[co, 0] (+ t_c * s[co, c], c ascending)
// with every product and sum rounded once (no FMA).  Neither operand fits int8, so both are
// stored shifted, w_s = q_w - (qmin_w + 128) and u_s = u - 128 (0 on a padded tap), and with
// cwz[co] = qmin_w + 128 - z_w[co], over the valid taps D = sum w_s u_s, E = sum w_s, SU = sum u_s,
// NV their number:
//     B_c = E_c + cwz * NV          A_c = D_c + cwz * SU_c + 128 * B_c.
// D is one v_mfma_i32_16x16x64_i8 per input channel (R*S <= 49 taps are one k step) with K23's
// lane map: the weight rows are the A operand, so a lane's four results are four consecutive
// channels of one pixel.  SU is the same MFMA against an all-ones row; E and NV are the two
// against the 0/1 validity of the taps instead of u_s.  A workgroup whose whole tile has every
// tap inside the image takes B_c = T_c[co] from the blob (the full-window sum, which B_c then is)
// and stages no validity: the same integers, so the same bits.
//
// One workgroup: TH rows x 32 columns of one image's output plane (TH in {2, 4, 8}, one wave per
// two rows) and up to 16 * NCH output channels, K31's tile.  The uint8 patch under the tile is
// staged once in LDS as u_s (K31's patch, a quarter of its bytes); the B operand of (pixel, c) is
// gathered from it through a table of the taps' offsets.
//
// Strided views.  The image is read through four byte strides (sN, sC, sH, sW), all >= 0, by the
// one address rule u8_at; only the staging below knows of them.  Planar (sW == 1) and generic walk
// the patch channel by channel; interleaved (sC == 1, Ci <= sW <= 4: HWC pixels) walks it in
// memory order, a row's bytes one after the other, scatters them into the planar patch and drops
// a pixel's pad byte.  No load touches a byte outside [0, u8_at(Nb-1, Ci-1, H-1, W-1)]: a padded
// position and a pad byte read element 0 of their image and are replaced.
#include <type_traits>

#include "ssq_common.h"
#include "qinfer_epi.h"
#include "qinfer_layout.h"
#include "qinfer_prepare.h"

namespace ssq {

typedef int i32x4q __attribute__((ext_vector_type(4)));

constexpr int kU8TW = 32;                  // tile columns
constexpr int kU8MaxTH = 8;                // tile rows at most (kBlock / kU8TW)
constexpr size_t kU8MaxLds = 64 * 1024;

// the staging forms (ssq_stem_u8_view_span's `form`)
constexpr int kU8Planar = 0, kU8Interleaved = 1, kU8Generic = 2;

// the byte offset of element (n, c, h, w) of a view with byte strides (sN, sC, sH, sW): the one
// address rule, of the staging loops and of the host's span query
template <typename T>
__host__ __device__ __forceinline__ T u8_at(T n, T c, T h, T w, T sN, T sC, T sH, T sW) {
  return n * sN + c * sC + h * sH + w * sW;
}

struct U8Geo {
  uint32_t Ci, H, W, Co, Cop, OH, OW, sh, sw;
  int ph, pw;
  uint32_t R, S, RS, nch;           // nch: 16-channel chunks of the blob (Cop / 16)
  uint32_t TH, eh, ew;              // tile rows; LDS units per output row / column
  uint32_t PH, PW;                  // patch rows, columns
  uint32_t pbytes, vbytes;          // LDS bytes of the u_s patch and of the validity patch
  uint32_t tiles_h, tiles_w, all_border;
  FastDiv div_tw, div_th, div_pw, div_ph, div_s;
  // the view (stem_u8_view fills these; stem_u8_geo leaves them 0)
  uint32_t sN, sC, sH, sW;          // the view's byte strides
  uint32_t form, rowb;              // staging form; interleaved: the bytes of a patch row (PW * sW)
  FastDiv div_rowb, div_px;         // interleaved: by rowb, by the pixel's bytes sW
};

// the image coordinate of patch index l along one axis (tile origin o0, stride st, kernel kk):
// K31's patch, which along an axis whose stride exceeds the kernel keeps the windows only
__device__ __forceinline__ int u8_coord(uint32_t l, uint32_t o0, uint32_t st, uint32_t kk, int pad) {
  if (st <= kk) return (int)(o0 * st + l) - pad;
  const uint32_t o = l / kk;
  return (int)((o0 + o) * st + (l - o * kk)) - pad;
}

// every tap of every pixel of the tile at (oh0, ow0), stored or not, lies inside the image
__host__ __device__ __forceinline__ bool u8_interior(int64_t oh0, int64_t ow0, int64_t TH,
                                                     int64_t H, int64_t W, int64_t sh, int64_t sw,
                                                     int64_t ph, int64_t pw, int64_t R, int64_t S) {
  return oh0 * sh - ph >= 0 && (oh0 + TH - 1) * sh - ph + R - 1 < H && ow0 * sw - pw >= 0 &&
         (ow0 + kU8TW - 1) * sw - pw + S - 1 < W;
}

// the lane's 16 k of one pixel's B operand: bytes p[ko[0]] .. p[ko[15]]
__device__ __forceinline__ i32x4q u8_gather(const int8_t* __restrict__ p, const int (&ko)[16]) {
  i32x4q v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t b0 = (uint8_t)p[ko[4 * q]], b1 = (uint8_t)p[ko[4 * q + 1]];
    const uint32_t b2 = (uint8_t)p[ko[4 * q + 2]], b3 = (uint8_t)p[ko[4 * q + 3]];
    v[q] = (int)(b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
  }
  return v;
}

// At least two waves per SIMD: left alone, the 64-channel forms spread over VGPRs and AGPRs (242 +
// 61) and run one.
template <int NCH, bool CODES>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void stem_u8_kernel(
    const uint8_t* __restrict__ u, const int8_t* __restrict__ wp, const int32_t* __restrict__ cwz,
    const int32_t* __restrict__ tt, const float* __restrict__ Mt, const float* __restrict__ st,
    U8Geo g, typename std::conditional<CODES, QEpi, float* __restrict__>::type y) {
  extern __shared__ __attribute__((aligned(16))) int8_t smem8[];
  int* koff = (int*)smem8;                 // [64]: tap k's offset inside a channel's patch, 0 from RS on
  int8_t* patch = smem8 + 256;             // [Ci][PH][PW]: u - 128, 0 outside the image
  int8_t* vpatch = patch + g.pbytes;       // [PH][PW]: 1 inside the image (a border tile only)
  int8_t* stage = vpatch + g.vbytes;       // CODES: the code tile [TH * 32][16 * NCH]
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const uint32_t nthr = g.TH * kU8TW;
  const uint32_t q1 = fdiv(blockIdx.x, g.div_tw), tw = blockIdx.x - q1 * g.tiles_w;
  const uint32_t n = fdiv(q1, g.div_th), th = q1 - n * g.tiles_h;
  const uint32_t oh0 = th * g.TH, ow0 = tw * kU8TW;
  const bool border = g.all_border ||
                      !u8_interior(oh0, ow0, g.TH, g.H, g.W, g.sh, g.sw, g.ph, g.pw, g.R, g.S);

  if (tid < 64) {
    const uint32_t r = fdiv(tid, g.div_s), s = tid - r * g.S;
    koff[tid] = tid < g.RS ? (int)(r * g.PW + s) : 0;
  }
  // the patch, four loads in flight per thread
  const uint32_t plane = g.PH * g.PW;
  // element 0 of this image: what an outside position or a pad byte reads before it is replaced,
  // so no load leaves the view's span
  const uint32_t at0 = u8_at<uint32_t>(n, 0, 0, 0, g.sN, g.sC, g.sH, g.sW);
  if (g.form == kU8Interleaved) {
    // memory order: patch row, then the row's bytes (column, then channel or pad byte), so
    // consecutive lanes read consecutive bytes
    const uint32_t total = g.PH * g.rowb;
    for (uint32_t i0 = tid; i0 < total; i0 += 4 * nthr) {
      uint8_t v[4];
      bool ok[4];
      uint32_t to[4];                      // b * plane + lr * PW + lc, or none (~0u)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t i = i0 + k * nthr;
        const uint32_t lr = fdiv(i, g.div_rowb), rem = i - lr * g.rowb;
        const uint32_t lc = fdiv(rem, g.div_px), b = rem - lc * g.sW;
        const int gh = u8_coord(lr, oh0, g.sh, g.R, g.ph);
        const int gw = u8_coord(lc, ow0, g.sw, g.S, g.pw);
        const bool real = i < total && b < g.Ci;
        ok[k] = real && gh >= 0 && gh < (int)g.H && gw >= 0 && gw < (int)g.W;
        to[k] = real ? b * plane + lr * g.PW + lc : ~0u;
        const uint32_t at =
            ok[k] ? u8_at<uint32_t>(n, b, (uint32_t)gh, (uint32_t)gw, g.sN, g.sC, g.sH, g.sW) : at0;
        v[k] = u[at];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (to[k] != ~0u) {
          patch[to[k]] = ok[k] ? (int8_t)(v[k] ^ 0x80u) : (int8_t)0;
          if (border && to[k] < plane) vpatch[to[k]] = ok[k] ? 1 : 0;
        }
      }
    }
  } else {
    // planar (sW == 1) and generic: channel, patch row, column
    const uint32_t total = g.Ci * plane;
    for (uint32_t i0 = tid; i0 < total; i0 += 4 * nthr) {
      uint8_t v[4];
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t i = i0 + k * nthr;
        const uint32_t row = fdiv(i, g.div_pw), lc = i - row * g.PW;
        const uint32_t ci = fdiv(row, g.div_ph), lr = row - ci * g.PH;
        const int gh = u8_coord(lr, oh0, g.sh, g.R, g.ph);
        const int gw = u8_coord(lc, ow0, g.sw, g.S, g.pw);
        ok[k] = i < total && gh >= 0 && gh < (int)g.H && gw >= 0 && gw < (int)g.W;
        const uint32_t at =
            ok[k] ? u8_at<uint32_t>(n, ci, (uint32_t)gh, (uint32_t)gw, g.sN, g.sC, g.sH, g.sW) : at0;
        v[k] = u[at];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t i = i0 + k * nthr;
        if (i < total) {
          patch[i] = ok[k] ? (int8_t)(v[k] ^ 0x80u) : (int8_t)0;
          if (border && i < plane) vpatch[i] = ok[k] ? 1 : 0;
        }
      }
    }
  }
  __syncthreads();

  // fragment maps (K23's): lane l holds row (l & 15) of the A operand and pixel (l & 15) of the
  // B operand at k = 16 (l >> 4) .. + 15; its results are channels 4 (l >> 4) + {0..3} of the
  // chunk at pixel (l & 15)
  const uint32_t fj = lane & 15, fq = lane >> 4;
  const uint32_t c0 = blockIdx.y * NCH;
  int ko[16];
  i32x4q ones;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ko[4 * q + j] = koff[fq * 16 + 4 * q + j];
      w |= (fq * 16 + 4 * q + j < g.RS ? 1u : 0u) << (8 * j);
    }
    ones[q] = (int)w;
  }
  const i32x4q zero = {0, 0, 0, 0};
  uint32_t nbad = 0;

  // one pixel group and one input channel at a time: unrolled, the groups' gathers and tables
  // are all live at once (256 VGPRs, one wave per SIMD)
#pragma unroll 1
  for (int gi = 0; gi < 4; ++gi) {
    const uint32_t row = 2 * wave + (gi >> 1), col = (gi & 1) * 16 + fj;
    const uint32_t pb = row * g.eh * g.PW + col * g.ew;
    i32x4q vb = zero;
    int nv = 0;
    if (border) {
      vb = u8_gather(vpatch + pb, ko);
      nv = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, vb, zero, 0, 0, 0)[0];
    }
    float yv[NCH][4] = {};
#pragma unroll 1
    for (uint32_t c = 0; c < g.Ci; ++c) {
      const i32x4q ub = u8_gather(patch + c * plane + pb, ko);
      const int su = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, ub, zero, 0, 0, 0)[0];
      const float Mc = Mt[c];
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        // a chunk past the blob's last reads the last again; its results are not stored
        const uint32_t cc = c0 + ch < g.nch ? c0 + ch : g.nch - 1;
        const i32x4q wf =
            *(const i32x4q*)(wp + ((size_t)(c * g.Cop + cc * 16 + fj)) * 64 + fq * 16);
        const i32x4q d = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, ub, zero, 0, 0, 0);
        i32x4q e = zero;
        if (border) e = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, vb, zero, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t cop = cc * 16 + fq * 4 + r;           // < Cop: the int32 tables hold it
          const uint32_t co = cop < g.Co ? cop : g.Co - 1;     // the caller's s has Co rows
          const int cw = cwz[cop];
          const int bc = border ? e[r] + cw * nv : tt[c * g.Cop + cop];
          const int ac = d[r] + cw * su + 128 * bc;
          const float t = __fsub_rn((float)ac, __fmul_rn(Mc, (float)bc));
          const float p = __fmul_rn(t, st[(size_t)co * g.Ci + c]);
          yv[ch][r] = c == 0 ? p : __fadd_rn(yv[ch][r], p);
        }
      }
    }
    const uint32_t oh = oh0 + row, ow = ow0 + col;
    const bool pval = oh < g.OH && ow < g.OW;
    if constexpr (CODES) {
      const QEpi& ep = y;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        int cd[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t co = (c0 + ch) * 16 + fq * 4 + r;
          cd[r] = (pval && co < g.Co) ? qepi_code_y(yv[ch][r], co, ep, nbad) : 0;
        }
        *(int*)(stage + ((row * kU8TW + col) * NCH + ch) * 16 + fq * 4) =
            qepi_pack4(cd[0], cd[1], cd[2], cd[3]);
      }
    } else {
      if (pval) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const uint32_t co = (c0 + ch) * 16 + fq * 4 + r;
            if (co < g.Co) y[(((size_t)n * g.Co + co) * g.OH + oh) * g.OW + ow] = yv[ch][r];
          }
      }
    }
  }

  if constexpr (CODES) {
    const QEpi& ep = y;
    __syncthreads();
    // thread (pixel, chunk) stores the 16 channels of one chunk of one pixel
    for (uint32_t k = tid; k < nthr * NCH; k += nthr) {
      const uint32_t p = k / NCH, c = k - p * NCH;
      const uint32_t oh = oh0 + p / kU8TW, ow = ow0 + p % kU8TW;
      if (oh < g.OH && ow < g.OW && c0 + c < g.nch)
        *(i32x4q*)(ep.out + (((size_t)n * g.OH + oh) * g.OW + ow) * ep.Cpo + (c0 + c) * 16) =
            *(const i32x4q*)(stage + (size_t)k * 16);
    }
    qepi_count(nbad, ep.bad);
  }
}

// packed codes -> ULayout: one workgroup per padded output channel, wave c its input channel c
__global__ __launch_bounds__(kBlock) void stem_u8_weight_prepare_kernel(
    const uint8_t* __restrict__ packed, const float* __restrict__ zp, int bs, int qmin, uint32_t Co,
    uint32_t Ci, uint32_t RS, uint32_t Cop, int8_t* __restrict__ wp, int32_t* __restrict__ cwz,
    int32_t* __restrict__ tt, uint32_t* __restrict__ bad) {
  const uint32_t co = blockIdx.x, c = threadIdx.x / kWave, k = threadIdx.x & (kWave - 1);
  const bool real = co < Co;
  const bool zok = !real || zp_is_code(zp[co], qmin);
  const int z = real && zok ? (int)zp[co] : qmin;
  const int cw = real ? qmin + 128 - z : 0;
  if (c < Ci) {
    int v = 0;
    if (real && k < RS)
      v = (int)packed_code(packed, ((size_t)co * Ci + c) * RS + k, bs) - 128;   // q - (qmin + 128)
    wp[((size_t)c * Cop + co) * 64 + k] = (int8_t)v;
    const int sum = (int)wave_sum((uint32_t)v);
    if (k == 0) tt[c * Cop + co] = sum + (int)RS * cw;   // a padded channel: 0
  }
  if (threadIdx.x == 0) {
    cwz[co] = cw;
    if (!zok) atomicAdd(bad, 1u);
  }
}

// The geometry both forms share, checked and gathered; the launch's grid, tile rows and LDS bytes.
static int stem_u8_geo(const char* me, bool codes, int64_t Nb, int64_t Ci, int64_t H, int64_t W,
                       int64_t Co, int64_t R, int64_t S, int64_t sh, int64_t sw, int64_t ph,
                       int64_t pw, U8Geo* g, dim3* grid, size_t* lds, int* nchunks) {
  const ULayout L = ulayout(Co, Ci, R, S);
  SSQ_REQUIRE(L.bytes, SSQ_E_ARG,
              "%s: outside the stem geometry (1 <= Ci <= 4, 1 <= R, S <= 7, Co >= 1)", me);
  SSQ_REQUIRE(Nb >= 1 && H >= 1 && W >= 1 && sh >= 1 && sw >= 1 && sh < (1ll << 24) &&
                  sw < (1ll << 24),
              SSQ_E_ARG, "%s: bad geometry (sizes and strides >= 1)", me);
  SSQ_REQUIRE(ph >= 0 && ph < R && pw >= 0 && pw < S, SSQ_E_ARG,
              "%s: padding (%lld, %lld) not below the kernel (%lld, %lld)", me, (long long)ph,
              (long long)pw, (long long)R, (long long)S);
  SSQ_REQUIRE(H + 2 * ph >= R && W + 2 * pw >= S, SSQ_E_ARG, "%s: empty output", me);
  const int64_t OH = (H + 2 * ph - R) / sh + 1, OW = (W + 2 * pw - S) / sw + 1;
  SSQ_REQUIRE(Nb * Ci * H * W < (1ll << 31) && Nb * OH * OW * L.Cop < (1ll << 31) &&
                  Nb * Co * OH * OW < (1ll << 31),
              SSQ_E_ARG, "%s: tensor exceeds 2^31 elements", me);
  const int64_t tiles_w = (OW + kU8TW - 1) / kU8TW;
  const int nch = (int)(L.Cop / 16);
  const int NCH = nch >= 3 ? 4 : nch;
  const int64_t ctiles = (nch + NCH - 1) / NCH;
  const int64_t eh = sh < R ? sh : R, ew = sw < S ? sw : S;
  const int64_t PW = ew * (kU8TW - 1) + S;
  // K31's rule: the tallest tile that leaves two workgroups per compute unit of a 256-CU part
  int64_t TH = kU8MaxTH, PH = 0;
  size_t bytes = 0, pbytes = 0, vbytes = 0;
  for (;; TH /= 2) {
    PH = eh * (TH - 1) + R;
    pbytes = (size_t)rup(Ci * PH * PW, 16);
    vbytes = (size_t)rup(PH * PW, 16);
    bytes = 256 + pbytes + vbytes + (codes ? (size_t)(TH * kU8TW * 16 * NCH) : 0);
    const int64_t wgs = Nb * ((OH + TH - 1) / TH) * tiles_w * ctiles;
    if (TH == 2 || (bytes <= kU8MaxLds && wgs >= 512)) break;
  }
  SSQ_REQUIRE(bytes <= kU8MaxLds, SSQ_E_ARG, "%s: patch exceeds LDS", me);
  const int64_t tiles_h = (OH + TH - 1) / TH;
  SSQ_REQUIRE(Nb * tiles_h * tiles_w < (1ll << 31) && ctiles < 65536, SSQ_E_ARG,
              "%s: grid too large", me);
  *g = {(uint32_t)Ci, (uint32_t)H,  (uint32_t)W,  (uint32_t)Co, (uint32_t)L.Cop, (uint32_t)OH,
        (uint32_t)OW, (uint32_t)sh, (uint32_t)sw, (int)ph,      (int)pw,         (uint32_t)R,
        (uint32_t)S,  (uint32_t)L.RS, (uint32_t)nch, (uint32_t)TH, (uint32_t)eh, (uint32_t)ew,
        (uint32_t)PH, (uint32_t)PW, (uint32_t)pbytes, (uint32_t)vbytes, (uint32_t)tiles_h,
        (uint32_t)tiles_w, 0u,
        make_fastdiv((uint32_t)tiles_w), make_fastdiv((uint32_t)tiles_h),
        make_fastdiv((uint32_t)PW), make_fastdiv((uint32_t)PH), make_fastdiv((uint32_t)S)};
  *grid = dim3((unsigned)(Nb * tiles_h * tiles_w), (unsigned)ctiles);
  *lds = bytes;
  *nchunks = NCH;
  return SSQ_OK;
}

// The view's span and staging form, checked: byte offsets lo .. hi are what a launch may read.
static int stem_u8_view(const char* me, int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t sN,
                        int64_t sC, int64_t sH, int64_t sW, int64_t* lo, int64_t* hi, int* form) {
  SSQ_REQUIRE(Nb >= 1 && Ci >= 1 && H >= 1 && W >= 1 && Nb < (1ll << 31) && Ci < (1ll << 31) &&
                  H < (1ll << 31) && W < (1ll << 31),
              SSQ_E_ARG, "%s: bad geometry (sizes >= 1)", me);
  SSQ_REQUIRE(sN >= 0 && sC >= 0 && sH >= 0 && sW >= 0, SSQ_E_ARG,
              "%s: negative stride (%lld, %lld, %lld, %lld)", me, (long long)sN, (long long)sC,
              (long long)sH, (long long)sW);
  // sizes and the strides that count below 2^31: each term below 2^62, and below 2^31 before the
  // four are summed (the stride of a dimension of size 1 addresses nothing)
  const auto term = [](int64_t n, int64_t st) {
    return n == 1 || (st < (1ll << 31) && (n - 1) * st < (1ll << 31));
  };
  SSQ_REQUIRE(term(Nb, sN) && term(Ci, sC) && term(H, sH) && term(W, sW) &&
                  u8_at<int64_t>(Nb - 1, Ci - 1, H - 1, W - 1, sN, sC, sH, sW) < (1ll << 31),
              SSQ_E_ARG, "%s: the view spans 2^31 bytes or more", me);
  *lo = u8_at<int64_t>(0, 0, 0, 0, sN, sC, sH, sW);
  *hi = u8_at<int64_t>(Nb - 1, Ci - 1, H - 1, W - 1, sN, sC, sH, sW);
  // one channel has no channel stride to speak of
  *form = sW == 1 ? kU8Planar
                  : ((Ci == 1 || sC == 1) && sW >= Ci && sW <= 4) ? kU8Interleaved : kU8Generic;
  return SSQ_OK;
}

template <bool CODES, typename Y>
static int stem_u8_run(const char* me, const uint8_t* u, const void* prepared,
                       size_t prepared_bytes, const float* M, const float* s, int64_t Nb,
                       int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S,
                       int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t sN, int64_t sC,
                       int64_t sH, int64_t sW, int every_tile_border, Y y, ssq_stream_t stream) {
  SSQ_REQUIRE(u && prepared && M && s, SSQ_E_ARG, "%s: null pointer", me);
  // the weight rows leave the blob as 16-byte vectors, cwz and T as int32 behind whole 64-byte rows
  SSQ_REQUIRE(((uintptr_t)prepared & 15u) == 0, SSQ_E_ARG,
              "%s: the prepared blob must be 16-byte aligned", me);
  U8Geo g;
  dim3 grid;
  size_t lds;
  int NCH;
  const int rc = stem_u8_geo(me, CODES, Nb, Ci, H, W, Co, R, S, sh, sw, ph, pw, &g, &grid, &lds,
                             &NCH);
  if (rc) return rc;
  const ULayout L = ulayout(Co, Ci, R, S);
  SSQ_REQUIRE(prepared_bytes >= L.bytes, SSQ_E_ARG, "%s: prepared blob of %zu bytes, %zu needed",
              me, prepared_bytes, L.bytes);
  int64_t lo, hi;
  int form;
  const int rv = stem_u8_view(me, Nb, Ci, H, W, sN, sC, sH, sW, &lo, &hi, &form);
  if (rv) return rv;
  g.sN = (uint32_t)sN, g.sC = (uint32_t)sC, g.sH = (uint32_t)sH, g.sW = (uint32_t)sW;
  g.form = (uint32_t)form;
  if (form == kU8Interleaved) {
    g.rowb = g.PW * g.sW;
    g.div_rowb = make_fastdiv(g.rowb);
    g.div_px = make_fastdiv(g.sW);
  }
  g.all_border = every_tile_border ? 1u : 0u;
  const int8_t* base = (const int8_t*)prepared;
  const int32_t* cwz = (const int32_t*)(base + L.off_cwz);
  const int32_t* tt = (const int32_t*)(base + L.off_t);
  const dim3 block(g.TH * kU8TW);
  hipStream_t hs = (hipStream_t)stream;
  if (NCH == 4)
    hipLaunchKernelGGL((stem_u8_kernel<4, CODES>), grid, block, lds, hs, u, base, cwz, tt, M, s, g, y);
  else if (NCH == 2)
    hipLaunchKernelGGL((stem_u8_kernel<2, CODES>), grid, block, lds, hs, u, base, cwz, tt, M, s, g, y);
  else
    hipLaunchKernelGGL((stem_u8_kernel<1, CODES>), grid, block, lds, hs, u, base, cwz, tt, M, s, g, y);
  return check_launch(me);
}

}  // namespace ssq

using namespace ssq;

extern "C" size_t ssq_stem_u8_weight_prepared_bytes(int64_t Co, int64_t Ci, int64_t R, int64_t S) {
  return ulayout(Co, Ci, R, S).bytes;
}

extern "C" int ssq_stem_u8_weight_prepare(const void* packed, const float* zp, int64_t Co,
                                          int64_t Ci, int64_t R, int64_t S, int n_bits, int qmin,
                                          void* prepared, uint32_t* bad, ssq_stream_t stream) {
  const char* me = "ssq_stem_u8_weight_prepare";
  SSQ_REQUIRE(packed && zp && prepared && bad, SSQ_E_ARG, "%s: null pointer", me);
  SSQ_REQUIRE(((uintptr_t)prepared & 15u) == 0, SSQ_E_ARG,
              "%s: the prepared blob must be 16-byte aligned", me);
  const int rc = qrange_ok(me, n_bits, qmin);
  if (rc) return rc;
  const ULayout L = ulayout(Co, Ci, R, S);
  SSQ_REQUIRE(L.bytes && L.bytes < (1ull << 31), SSQ_E_ARG,
              "%s: outside the stem geometry (1 <= Ci <= 4, 1 <= R, S <= 7, Co >= 1)", me);
  int8_t* base = (int8_t*)prepared;
  hipLaunchKernelGGL(stem_u8_weight_prepare_kernel, dim3((uint32_t)L.Cop), dim3(kBlock), 0,
                     (hipStream_t)stream, (const uint8_t*)packed, zp, packed_bits(n_bits), qmin,
                     (uint32_t)Co, (uint32_t)Ci, (uint32_t)L.RS, (uint32_t)L.Cop, base,
                     (int32_t*)(base + L.off_cwz), (int32_t*)(base + L.off_t), bad);
  return check_launch(me);
}

extern "C" int ssq_stem_u8_tiles(int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                 int64_t R, int64_t S, int64_t stride_h, int64_t stride_w,
                                 int64_t pad_h, int64_t pad_w, int codes, int64_t* interior,
                                 int64_t* border) {
  const char* me = "ssq_stem_u8_tiles";
  SSQ_REQUIRE(interior && border, SSQ_E_ARG, "%s: null pointer", me);
  U8Geo g;
  dim3 grid;
  size_t lds;
  int NCH;
  const int rc = stem_u8_geo(me, codes != 0, Nb, Ci, H, W, Co, R, S, stride_h, stride_w, pad_h,
                             pad_w, &g, &grid, &lds, &NCH);
  if (rc) return rc;
  int64_t in = 0;
  for (uint32_t th = 0; th < g.tiles_h; ++th)
    for (uint32_t tw = 0; tw < g.tiles_w; ++tw)
      in += u8_interior((int64_t)th * g.TH, (int64_t)tw * kU8TW, g.TH, H, W, stride_h, stride_w,
                        pad_h, pad_w, R, S);
  *interior = in * Nb * grid.y;
  *border = ((int64_t)g.tiles_h * g.tiles_w - in) * Nb * grid.y;
  return SSQ_OK;
}

extern "C" int ssq_stem_u8_view_span(int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t sN,
                                     int64_t sC, int64_t sH, int64_t sW, int64_t* lo, int64_t* hi,
                                     int* form) {
  const char* me = "ssq_stem_u8_view_span";
  SSQ_REQUIRE(lo && hi && form, SSQ_E_ARG, "%s: null pointer", me);
  return stem_u8_view(me, Nb, Ci, H, W, sN, sC, sH, sW, lo, hi, form);
}

extern "C" int ssq_stem_conv_u8_strided_fwd(
    const uint8_t* u, const void* prepared, size_t prepared_bytes, const float* M, const float* s,
    int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S,
    int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t sN, int64_t sC,
    int64_t sH, int64_t sW, int every_tile_border, float* y, ssq_stream_t stream) {
  const char* me = "ssq_stem_conv_u8_strided_fwd";
  SSQ_REQUIRE(y, SSQ_E_ARG, "%s: null pointer", me);
  return stem_u8_run<false>(me, u, prepared, prepared_bytes, M, s, Nb, Ci, H, W, Co, R, S,
                            stride_h, stride_w, pad_h, pad_w, sN, sC, sH, sW, every_tile_border, y,
                            stream);
}

extern "C" int ssq_stem_conv_u8_strided_codes_fwd(
    const uint8_t* u, const void* prepared, size_t prepared_bytes, const float* M, const float* s,
    int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S,
    int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t sN, int64_t sC,
    int64_t sH, int64_t sW, int every_tile_border, const float* bias, const float* gamma,
    const float* phi, int act, float out_delta, float out_zero_point, int out_qmin, int out_qmax,
    int8_t* out_codes, uint32_t* bad, ssq_stream_t stream) {
  const char* me = "ssq_stem_conv_u8_strided_codes_fwd";
  QEpi e;
  const int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin,
                           out_qmax, out_codes, bad, &e);
  if (rc) return rc;
  e.Cpo = (uint32_t)((Co + 15) / 16 * 16);
  return stem_u8_run<true>(me, u, prepared, prepared_bytes, M, s, Nb, Ci, H, W, Co, R, S, stride_h,
                           stride_w, pad_h, pad_w, sN, sC, sH, sW, every_tile_border, e, stream);
}

// the dense NCHW calls of the same run function
extern "C" int ssq_stem_conv_u8_fwd(const uint8_t* u, const void* prepared, size_t prepared_bytes,
                                    const float* M, const float* s, int64_t Nb, int64_t Ci,
                                    int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S,
                                    int64_t stride_h, int64_t stride_w, int64_t pad_h,
                                    int64_t pad_w, int every_tile_border, float* y,
                                    ssq_stream_t stream) {
  const char* me = "ssq_stem_conv_u8_fwd";
  SSQ_REQUIRE(y, SSQ_E_ARG, "%s: null pointer", me);
  return stem_u8_run<false>(me, u, prepared, prepared_bytes, M, s, Nb, Ci, H, W, Co, R, S,
                            stride_h, stride_w, pad_h, pad_w, Ci * H * W, H * W, W, 1,
                            every_tile_border, y, stream);
}

extern "C" int ssq_stem_conv_u8_codes_fwd(
    const uint8_t* u, const void* prepared, size_t prepared_bytes, const float* M, const float* s,
    int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S,
    int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int every_tile_border,
    const float* bias, const float* gamma, const float* phi, int act, float out_delta,
    float out_zero_point, int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad,
    ssq_stream_t stream) {
  const char* me = "ssq_stem_conv_u8_codes_fwd";
  QEpi e;
  const int rc = qepi_init(me, bias, gamma, phi, act, out_delta, out_zero_point, out_qmin,
                           out_qmax, out_codes, bad, &e);
  if (rc) return rc;
  e.Cpo = (uint32_t)((Co + 15) / 16 * 16);
  return stem_u8_run<true>(me, u, prepared, prepared_bytes, M, s, Nb, Ci, H, W, Co, R, S, stride_h,
                           stride_w, pad_h, pad_w, Ci * H * W, H * W, W, 1, every_tile_border, e,
                           stream);
}
