// K19: one BRECQ AdaRound iteration of a Linear layer in two launches.
//
// The end-to-end flow reconstructs the network's last layer (ResNet-18's fc, 512 -> 1000)
// with BRECQ's layer loop, 20000 iterations at batch 32 (layer_recon.py:10-104, called from
// main_imagenet.py for the fc).  Per iteration the reference gathers the batch
// (cached[randperm(N)[:32]]), runs the quantized layer (AdaRoundQuantizer soft rounding,
// adaptive_rounding.py:38-67, then F.linear), the loss (lp_loss p = 2 + the rounding
// regulariser, block_recon.py:119-182 / layer_recon.py:107-170), its backward and Adam.
// Each of those is microseconds of GPU work on this layer, so as separate launches the loop
// is bound by dependent-launch boundaries (8 launches: 32 us per iteration replayed back to
// back; in two launches 19.5 us, profiles/r5_fc_replay_probe.txt).  Here:
//
//   fc_fwd_loss  (one workgroup per 16 x 16 tile of y, 8 waves splitting C_in): y = x W^T
//     + bias on fp32 MFMA (v_mfma_f32_16x16x4_f32, every operand load of a wave issued
//     before its first MFMA), the 8 partial tiles added in wave order, then the lp_loss
//     p = 2 term and gradient of every output (lp_elem: the lp_loss_kernel ops) -> g = dL/dy
//     and one double loss partial per workgroup;
//   fc_bwd_adam  (one workgroup per 16 x 16 tile of dW): dW = g^T x on the same MFMA, then
//     per element (one a thread) AdaRound's backward with the rounding regulariser folded in
//     (the adaround_bwd_kernel ops, lambda and b from the iteration's device words), V's Adam step
//     (ssq_adam's ops), and W^ of the NEXT iteration from the updated V (the
//     adaround_fwd_kernel ops) -- so the forward reads W^ instead of evaluating the soft
//     rounding (a divide and an exp per weight) itself; workgroup 0 also sums the loss
//     partials.
//
// Under data parallel the gradient all-reduce sits between the backward and Adam
// (block_recon.py:100-102), so the second launch also exists split where V's gradient exists:
//
//   fc_bwd_grad   fc_bwd_adam's tiling, dW and AdaRound's backward, up to the store of V's
//     gradient (to the caller's pointer: a slice of the flat all-reduce bucket, 4-B aligned
//     is enough); V, m, v and W^ are not touched;
//   fc_adam_what  elementwise over C_out x C_in, a float4 per thread: V's Adam step from the
//     (reduced) gradient and W^ of the next iteration.
//
// ssq_fc_recon_grad = fc_fwd_loss + fc_bwd_grad, ssq_fc_recon_apply = fc_adam_what.  The
// per-element arithmetic of the three backward kernels is one set of helpers (fc_vgrad,
// fc_step), so the pair fed its own gradient gives ssq_fc_recon_iter's bits
// (tests/test_fc_split_gpu.py).
//
// W^ of the first iteration comes from ssq_adaround_fwd (the caller's).  The batch indices
// and the iteration's scalars are read from one device slot (BatchFeeder's words: idx, then
// (lambda, b), then Adam's (-lr/bc1, sqrt(bc2))), so a graph of several iterations reads one
// slot each (quant/block_recon.py ChunkGraph).  Deterministic: fixed summation orders, no
// atomics.  The GEMMs' summation order is this kernel's, not hipBLASLt's: values agree with
// the unfused launches to fp32 rounding (tests/test_recon_gpu.py).
#include "fin_tasks.h"
#include "ssq_common.h"

namespace ssq {

constexpr uint32_t kFcRows = 64;      // max batch rows
constexpr uint32_t kFcMaxCi = 4096;
constexpr uint32_t kFcKW = 8;         // forward: waves per output tile = K chunks
constexpr uint32_t kFcBwdW = 4;       // backward: waves per workgroup (one 16x16 dW tile)

// W^ of one element: adaround_fwd_kernel's ops (per-row delta, scale 1)
__device__ __forceinline__ float fc_what(float w, float v, float d, float z, float lo, float hi) {
  const float q = clampf(__fadd_rn(__fadd_rn(floorf(w / d), rect_sigmoid(v)), z), lo, hi);
  return __fmul_rn(__fsub_rn(q, z), d);
}

// V's gradient of one element from its dW: adaround_bwd_kernel's ops with the rounding
// regulariser (lambda, b) folded in
__device__ __forceinline__ float fc_vgrad(float w, float v, float d, float z, float lo, float hi,
                                          float dw, float lam, float rb) {
  const float u0 = __fadd_rn(__fadd_rn(floorf(w / d), rect_sigmoid(v)), z);
  const float gi = (u0 >= lo && u0 <= hi) ? __fmul_rn(dw, d) : 0.0f;
  const float ga = rect_sigmoid_grad(v, gi);
  return lam != 0.0f ? __fadd_rn(ga, round_reg_grad(v, lam, rb)) : ga;
}

// V's Adam step of one element (ssq_adam's ops; p, m, v updated in place) and the next
// iteration's W^ from the updated V (adaround_fwd_kernel's ops), returned
__device__ __forceinline__ float fc_step(const AdamConst& ac, float g, float w, float d, float z,
                                         float lo, float hi, float& p, float& m, float& v) {
  adam_update(ac, g, p, m, v);
  return fc_what(w, p, d, z, lo, hi);
}

// 16 consecutive floats (4 x 16 B) from a 16-B aligned row, or zeros
__device__ __forceinline__ void ld16(const float* p, bool ok, f32x4* v) {
#pragma unroll
  for (int u = 0; u < 4; ++u) v[u] = ok ? ((const f32x4*)p)[u] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// Forward: workgroup = one 16 x 16 tile of y (rows r0.., columns o0..), 8 waves; wave w
// sums k in its chunk [w*ck, (w+1)*ck) with v_mfma_f32_16x16x4_f32 (A = x rows, B = W^^T),
// 64 k per round: lane l (k slot q = l >> 4) feeds k = k0 + 16 q + s at step s, so its 16
// A and 16 B values are 4 float4 loads each, all issued before the first MFMA.  The 8
// partial tiles are added in wave order through LDS, then the epilogue: bias, the lp_loss
// p = 2 term and gradient (lp_elem), one loss partial per workgroup.
__global__ __launch_bounds__(kBlock * 2) void fc_fwd_loss(
    const float* __restrict__ x, const int64_t* __restrict__ slot, uint32_t bs,
    const float* __restrict__ what, const float* __restrict__ bias, uint32_t Co, uint32_t Ci,
    uint32_t ck, const float* __restrict__ tgt, float inv_m, float* __restrict__ g,
    double* __restrict__ part) {
  __shared__ f32x4 red[kFcKW][kWave];
  __shared__ double lred[kWave];
  const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const uint32_t i16 = lane & 15, q = lane >> 4;
  const uint32_t o0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  const uint32_t ra = r0 + i16, ob = o0 + i16;          // this lane's A row / B column
  const bool aok = ra < bs, bok = ob < Co;
  const float* xr = x + (aok ? slot[ra] : 0) * (int64_t)Ci;
  const float* wr = what + (int64_t)(bok ? ob : 0) * Ci;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  const uint32_t k1 = min(Ci, (w + 1) * ck);
  for (uint32_t k0 = w * ck; k0 < k1; k0 += 64) {
    const uint32_t kq = k0 + 16 * q;
    const bool in = kq < k1;                          // Ci % 64 == 0 -> whole 16-runs
    f32x4 av[4], bv[4];
    ld16(xr + kq, aok && in, av);
    ld16(wr + kq, bok && in, bv);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].x, bv[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].y, bv[u].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].z, bv[u].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].w, bv[u].w, acc, 0, 0, 0);
    }
  }
  red[w][lane] = acc;
  __syncthreads();
  if (w != 0) return;
  f32x4 y = red[0][lane];
#pragma unroll
  for (uint32_t k = 1; k < kFcKW; ++k) {
    const f32x4 t = red[k][lane];
    y.x = __fadd_rn(y.x, t.x);
    y.y = __fadd_rn(y.y, t.y);
    y.z = __fadd_rn(y.z, t.z);
    y.w = __fadd_rn(y.w, t.w);
  }
  // D layout: column o = o0 + (lane & 15), rows r0 + 4 (lane >> 4) + v
  const uint32_t o = o0 + i16;
  double la = 0.0;
  if (o < Co) {
    const float b = bias ? bias[o] : 0.0f;
    float yv[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const uint32_t r = r0 + 4 * q + v;
      if (r < bs) {
        const float yy = bias ? __fadd_rn(yv[v], b) : yv[v];
        g[(int64_t)r * Co + o] = lp_elem<0>(yy, tgt[slot[r] * (int64_t)Co + o], 2.0f, inv_m, 1.0f, 0,
                                            la);
      }
    }
  }
  la = wave_sum(la);
  if (lane == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = la;
}

// One 16 x 16 tile of dW = g^T x (rows o0.., columns c0..) into LDS, by wave 0 of the
// workgroup with v_mfma_f32_16x16x4_f32 (lane slot q feeds rows r = 4 s + q in a fixed
// order); workgroup 0 also sums the forward's loss partials in order.  Ends with the
// workgroup's barrier: tile[row][column] is then every wave's to read.
__device__ __forceinline__ void fc_dw_tile(
    const float* __restrict__ x, const int64_t* __restrict__ slot, uint32_t bs,
    const float* __restrict__ g, uint32_t Co, uint32_t Ci, uint32_t o0, uint32_t c0,
    const double* __restrict__ part, uint32_t nparts, double M, float* __restrict__ loss_out,
    float (*tile)[17]) {
  const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const uint32_t i16 = lane & 15, q = lane >> 4;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // the loss value: the forward's workgroup partials in order
    double s = 0.0;
    for (uint32_t k = 0; k < nparts; ++k) s += part[k];
    loss_out[0] = (float)(s / M);
  }
  if (w == 0) {
    // the operands: A[i][k] = g[r][o0 + i], B[k][j] = x[idx[r]][c0 + j], r = 4 s + q over
    // the 16 steps (bs <= 64)
    float av[16], bv[16];
    const uint32_t oa = o0 + i16;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const uint32_t r = 4 * s + q;
      const bool rk = r < bs;
      av[s] = (rk && oa < Co) ? g[(int64_t)r * Co + oa] : 0.0f;
      bv[s] = rk ? x[slot[r] * (int64_t)Ci + c0 + i16] : 0.0f;
    }
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t steps = (bs + 3) / 4;               // uniform
    for (uint32_t s = 0; s < 16; ++s)
      if (s < steps) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
    // D layout: column i16, rows 4 q + e
    tile[4 * q + 0][i16] = acc.x;
    tile[4 * q + 1][i16] = acc.y;
    tile[4 * q + 2][i16] = acc.z;
    tile[4 * q + 3][i16] = acc.w;
  }
  __syncthreads();
}

// Backward + Adam + the next W^: workgroup = one 16 x 16 tile of dW (rows o0.., columns
// c0..), 4 waves.  Wave 0 forms the tile (fc_dw_tile); then each of the 4 waves takes 4 of
// its rows, one element per lane: AdaRound's backward with the rounding regulariser
// (fc_vgrad, lambda and b from the iteration's words), V's Adam step and W^ of the updated V
// for the next iteration (fc_step).  The per-element math (a divide, two exps, a pow, a
// sqrt, Adam's divides) is most of the kernel, so it is spread over 4x the waves of a
// wave-per-tile form (traced on the ResNet-18 fc: 13.1-15.1 -> 11.7-13.1 us,
// profiles/r5_fc_anatomy_wavetile.txt vs r5_fc_anatomy.txt).  Every load of a wave is
// issued before its first use.
__global__ __launch_bounds__(kBlock) void fc_bwd_adam(
    const float* __restrict__ x, const int64_t* __restrict__ slot, uint32_t bs,
    const float* __restrict__ g, const float* __restrict__ W, float* __restrict__ V,
    const float* __restrict__ delta, const float* __restrict__ zp, float lo, float hi,
    uint32_t Co, uint32_t Ci, const float* __restrict__ regp, AdamConst ac,
    float* __restrict__ m, float* __restrict__ v, float* __restrict__ gv_out,
    float* __restrict__ what, const double* __restrict__ part, uint32_t nparts, double M,
    float* __restrict__ loss_out) {
  __shared__ float tile_dw[16][17];
  const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const uint32_t nct = Ci / 16;                       // column tiles (Ci % 16 == 0)
  const uint32_t o0 = (blockIdx.x / nct) * 16, c0 = (blockIdx.x % nct) * 16;
  const uint32_t i16 = lane & 15, q = lane >> 4;
  // this thread's element: row o = o0 + 4 w + q, column c = c0 + i16
  const uint32_t o = o0 + 4 * w + q, c = c0 + i16;
  const bool ok = o < Co;
  const int64_t i = (int64_t)(ok ? o : 0) * Ci + c;
  const float wv = ok ? W[i] : 0.0f, b = ok ? V[i] : 0.0f;
  const float mv = ok ? m[i] : 0.0f, vv = ok ? v[i] : 0.0f;
  const float d = ok ? delta[o] : 1.0f, z = ok ? zp[o] : 0.0f;
  const float lam = regp[0], rb = regp[1];
  fc_dw_tile(x, slot, bs, g, Co, Ci, o0, c0, part, nparts, M, loss_out, tile_dw);
  if (!ok) return;
  const float gb = fc_vgrad(wv, b, d, z, lo, hi, tile_dw[4 * w + q][i16], lam, rb);
  if (gv_out) gv_out[i] = gb;
  float pn = b, mn = mv, vn = vv;
  what[i] = fc_step(ac, gb, wv, d, z, lo, hi, pn, mn, vn);
  V[i] = pn;
  m[i] = mn;
  v[i] = vn;
}

// fc_bwd_adam up to V's gradient (the same tiling, fc_dw_tile and fc_vgrad): gv_out is the
// only array written -- the caller's, possibly a slice of a flat all-reduce bucket (one
// 4-B store per lane, 16 lanes a 64-B run).  The step follows in fc_adam_what, after the
// gradient's all-reduce.
__global__ __launch_bounds__(kBlock) void fc_bwd_grad(
    const float* __restrict__ x, const int64_t* __restrict__ slot, uint32_t bs,
    const float* __restrict__ g, const float* __restrict__ W, const float* __restrict__ V,
    const float* __restrict__ delta, const float* __restrict__ zp, float lo, float hi,
    uint32_t Co, uint32_t Ci, const float* __restrict__ regp, float* __restrict__ gv_out,
    const double* __restrict__ part, uint32_t nparts, double M, float* __restrict__ loss_out) {
  __shared__ float tile_dw[16][17];
  const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const uint32_t nct = Ci / 16;
  const uint32_t o0 = (blockIdx.x / nct) * 16, c0 = (blockIdx.x % nct) * 16;
  const uint32_t i16 = lane & 15, q = lane >> 4;
  const uint32_t o = o0 + 4 * w + q, c = c0 + i16;
  const bool ok = o < Co;
  const int64_t i = (int64_t)(ok ? o : 0) * Ci + c;
  const float wv = ok ? W[i] : 0.0f, b = ok ? V[i] : 0.0f;
  const float d = ok ? delta[o] : 1.0f, z = ok ? zp[o] : 0.0f;
  const float lam = regp[0], rb = regp[1];
  fc_dw_tile(x, slot, bs, g, Co, Ci, o0, c0, part, nparts, M, loss_out, tile_dw);
  if (!ok) return;
  gv_out[i] = fc_vgrad(wv, b, d, z, lo, hi, tile_dw[4 * w + q][i16], lam, rb);
}

// V's Adam step from a given gradient and the next W^ (fc_step), elementwise: thread t takes
// elements 4 t .. 4 t + 3 of the [Co, Ci] arrays as one float4 each (Ci % 64 == 0: a float4
// never crosses a row, so delta / zp are read once).  The gradient may be a 4-B aligned slice
// of the all-reduce bucket: G4 says it is 16-B aligned and read as a float4 too.  n4 = Co Ci / 4.
template <bool G4>
__global__ __launch_bounds__(kBlock) void fc_adam_what(
    const float* __restrict__ W, float* __restrict__ V, const float* __restrict__ grad,
    const float* __restrict__ delta, const float* __restrict__ zp, float lo, float hi,
    uint32_t n4, FastDiv ci4, AdamConst ac, float* __restrict__ m, float* __restrict__ v,
    float* __restrict__ what) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n4) return;
  const uint32_t o = fdiv(t, ci4);                    // row: t / (Ci / 4)
  const f32x4 w4 = ((const f32x4*)W)[t];
  f32x4 p4 = ((const f32x4*)V)[t], m4 = ((const f32x4*)m)[t], v4 = ((const f32x4*)v)[t];
  f32x4 g4;
  if constexpr (G4) {
    g4 = ((const f32x4*)grad)[t];
  } else {
    const float* gp = grad + 4 * (int64_t)t;
    g4 = f32x4{gp[0], gp[1], gp[2], gp[3]};
  }
  const float d = delta[o], z = zp[o];
  float pe[4] = {p4.x, p4.y, p4.z, p4.w}, me[4] = {m4.x, m4.y, m4.z, m4.w};
  float ve[4] = {v4.x, v4.y, v4.z, v4.w}, he[4];
  const float ge[4] = {g4.x, g4.y, g4.z, g4.w}, we[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) he[e] = fc_step(ac, ge[e], we[e], d, z, lo, hi, pe[e], me[e], ve[e]);
  ((f32x4*)V)[t] = f32x4{pe[0], pe[1], pe[2], pe[3]};
  ((f32x4*)m)[t] = f32x4{me[0], me[1], me[2], me[3]};
  ((f32x4*)v)[t] = f32x4{ve[0], ve[1], ve[2], ve[3]};
  ((f32x4*)what)[t] = f32x4{he[0], he[1], he[2], he[3]};
}

}  // namespace ssq

using namespace ssq;

extern "C" size_t ssq_fc_recon_workspace_size(int64_t Co, int64_t Ci, int64_t bs) {
  (void)Ci;
  const size_t nwg = (size_t)((Co + 15) / 16) * (size_t)((bs + 15) / 16);
  return nwg * sizeof(double);
}

namespace {

// The rules of the fc iteration's shapes (shared by every entry point below)
bool fc_shape_ok(int64_t bs, int64_t Co, int64_t Ci, int qmin, int qmax) {
  return bs >= 1 && bs <= (int64_t)kFcRows && Co >= 1 && Ci >= 64 && Ci % 64 == 0 &&
         Ci <= (int64_t)kFcMaxCi && Co * Ci < (1ll << 31) && qmin < qmax;
}
bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The argument checks ssq_fc_recon_iter and ssq_fc_recon_grad share, then the forward launch
// (`who` names the entry point in the messages)
int fc_forward(const char* who, const float* x_cache, const float* tgt_cache,
               const int64_t* slot, int64_t bs, const float* W, const float* V,
               const float* What, const float* delta, const float* zp, int qmin, int qmax,
               const float* bias, int64_t Co, int64_t Ci, float* g, float* loss_out, void* ws,
               size_t ws_bytes, hipStream_t s) {
  SSQ_REQUIRE(x_cache && tgt_cache && slot && W && V && What && delta && zp && g && loss_out,
              SSQ_E_ARG, "%s: null pointer", who);
  SSQ_REQUIRE(fc_shape_ok(bs, Co, Ci, qmin, qmax), SSQ_E_ARG,
              "%s: 1 <= batch <= %u, 64 <= C_in <= %u, C_in %% 64 == 0", who, kFcRows, kFcMaxCi);
  SSQ_REQUIRE(al16(x_cache) && al16(What), SSQ_E_ARG, "%s: 16-B aligned x / W^", who);
  SSQ_REQUIRE(ws && ws_bytes >= ssq_fc_recon_workspace_size(Co, Ci, bs), SSQ_E_WS,
              "%s: workspace too small", who);
  // K chunk per wave: C_in / 8 rounded up to whole 64-k rounds
  const uint32_t ck = (uint32_t)(((Ci + kFcKW - 1) / kFcKW + 63) / 64 * 64);
  const dim3 gf((unsigned)((Co + 15) / 16), (unsigned)((bs + 15) / 16));
  hipLaunchKernelGGL(fc_fwd_loss, gf, dim3(kWave * kFcKW), 0, s, x_cache, slot, (uint32_t)bs,
                     What, bias, (uint32_t)Co, (uint32_t)Ci, ck, tgt_cache, 1.0f / (float)bs, g,
                     (double*)ws);
  return check_launch(who);
}

}  // namespace

extern "C" int ssq_fc_recon_iter(const float* x_cache, const float* tgt_cache,
                                 const int64_t* slot, int64_t bs, const float* W, float* V,
                                 float* What, const float* delta, const float* zp, int qmin,
                                 int qmax, const float* bias, int64_t Co, int64_t Ci,
                                 float one_minus_beta1, float beta2, float one_minus_beta2,
                                 float eps, float* exp_avg, float* exp_avg_sq, float* g,
                                 float* gv_out, float* loss_out, void* ws, size_t ws_bytes,
                                 ssq_stream_t stream) {
  SSQ_REQUIRE(exp_avg && exp_avg_sq, SSQ_E_ARG, "ssq_fc_recon_iter: null pointer");
  hipStream_t s = (hipStream_t)stream;
  int rc = fc_forward("ssq_fc_recon_iter", x_cache, tgt_cache, slot, bs, W, V, What, delta, zp,
                      qmin, qmax, bias, Co, Ci, g, loss_out, ws, ws_bytes, s);
  if (rc) return rc;
  // the slot: bs indices, then (lambda, b) and Adam's (-lr/bc1, sqrt(bc2)) as fp32 pairs
  const float* words = (const float*)(slot + bs);
  const uint32_t nparts = (uint32_t)(((Co + 15) / 16) * ((bs + 15) / 16));
  const uint32_t ntile = (uint32_t)(((Co + 15) / 16) * (Ci / 16));
  const AdamConst ac{one_minus_beta1, beta2, one_minus_beta2, eps, words + 2};
  hipLaunchKernelGGL(fc_bwd_adam, dim3(ntile), dim3(kWave * kFcBwdW), 0,
                     s, x_cache, slot, (uint32_t)bs, g, W, V, delta, zp, (float)qmin, (float)qmax,
                     (uint32_t)Co, (uint32_t)Ci, words, ac, exp_avg, exp_avg_sq, gv_out, What,
                     (const double*)ws, nparts, (double)bs, loss_out);
  return check_launch("ssq_fc_recon_iter (backward + Adam + next W^)");
}

extern "C" int ssq_fc_recon_grad(const float* x_cache, const float* tgt_cache,
                                 const int64_t* slot, int64_t bs, const float* W, const float* V,
                                 const float* What, const float* delta, const float* zp, int qmin,
                                 int qmax, const float* bias, int64_t Co, int64_t Ci, float* g,
                                 float* gv_out, float* loss_out, void* ws, size_t ws_bytes,
                                 ssq_stream_t stream) {
  SSQ_REQUIRE(gv_out && ((uintptr_t)gv_out & 3u) == 0, SSQ_E_ARG,
              "ssq_fc_recon_grad: gv_out is required (4-B aligned)");
  hipStream_t s = (hipStream_t)stream;
  int rc = fc_forward("ssq_fc_recon_grad", x_cache, tgt_cache, slot, bs, W, V, What, delta, zp,
                      qmin, qmax, bias, Co, Ci, g, loss_out, ws, ws_bytes, s);
  if (rc) return rc;
  const float* words = (const float*)(slot + bs);      // (lambda, b) first
  const uint32_t nparts = (uint32_t)(((Co + 15) / 16) * ((bs + 15) / 16));
  const uint32_t ntile = (uint32_t)(((Co + 15) / 16) * (Ci / 16));
  hipLaunchKernelGGL(fc_bwd_grad, dim3(ntile), dim3(kWave * kFcBwdW), 0, s, x_cache, slot,
                     (uint32_t)bs, g, W, V, delta, zp, (float)qmin, (float)qmax, (uint32_t)Co,
                     (uint32_t)Ci, words, gv_out, (const double*)ws, nparts, (double)bs, loss_out);
  return check_launch("ssq_fc_recon_grad (backward)");
}

extern "C" int ssq_fc_recon_apply(const float* W, float* V, float* What, const float* delta,
                                  const float* zp, int qmin, int qmax, int64_t Co, int64_t Ci,
                                  const int64_t* slot, int64_t bs, const float* grad,
                                  float one_minus_beta1, float beta2, float one_minus_beta2,
                                  float eps, float* exp_avg, float* exp_avg_sq,
                                  ssq_stream_t stream) {
  SSQ_REQUIRE(W && V && What && delta && zp && slot && grad && exp_avg && exp_avg_sq, SSQ_E_ARG,
              "ssq_fc_recon_apply: null pointer");
  SSQ_REQUIRE(fc_shape_ok(bs, Co, Ci, qmin, qmax), SSQ_E_ARG,
              "ssq_fc_recon_apply: 1 <= batch <= %u, 64 <= C_in <= %u, C_in %% 64 == 0", kFcRows,
              kFcMaxCi);
  SSQ_REQUIRE(al16(W) && al16(V) && al16(What) && al16(exp_avg) && al16(exp_avg_sq) &&
                  ((uintptr_t)grad & 3u) == 0, SSQ_E_ARG,
              "ssq_fc_recon_apply: 16-B aligned W / V / W^ / moments, 4-B aligned gradient");
  hipStream_t s = (hipStream_t)stream;
  // Adam's (-lr/bc1, sqrt(bc2)) follow the slot's bs indices and (lambda, b)
  const AdamConst ac{one_minus_beta1, beta2, one_minus_beta2, eps,
                     (const float*)(slot + bs) + 2};
  const uint32_t n4 = (uint32_t)(Co * Ci / 4);
  const dim3 grid((n4 + kBlock - 1) / kBlock);
  const FastDiv ci4 = make_fastdiv((uint32_t)(Ci / 4));
  if (al16(grad))
    hipLaunchKernelGGL(fc_adam_what<true>, grid, dim3(kBlock), 0, s, W, V, grad, delta, zp,
                       (float)qmin, (float)qmax, n4, ci4, ac, exp_avg, exp_avg_sq, What);
  else
    hipLaunchKernelGGL(fc_adam_what<false>, grid, dim3(kBlock), 0, s, W, V, grad, delta, zp,
                       (float)qmin, (float)qmax, n4, ci4, ac, exp_avg, exp_avg_sq, What);
  return check_launch("ssq_fc_recon_apply (Adam + next W^)");
}
