// K20: BRECQ's Fisher-weighted reconstruction losses (block_recon.py:156-162,
// layer_recon.py:144-148), value + gradient wrt pred, for the device loop.
//
//   fisher_diag: loss = sum (pred-tgt)^2 * g^2 / M,  M = n / C
//                grad = fl(fl(fl(1/M) * fl(g*g)) * (2*d)),  d = fl(pred - tgt): torch autograd's
//                own operations in its own order (mean, mul, pow backward) -> bit-identical
//   fisher_full: a = |pred-tgt|, s_n = sum_{c,h,w} a*|g| per sample,
//                loss = sum_n s_n * sum(a*|g|) / (100*n)
//                grad = 2 * s_n * |g| * sgn(d) / (100*n)
//
// Like K11 (recon.hip): float4 nontemporal streams when every pointer is 16-B aligned, a
// scalar tail otherwise; the target AND the Fisher rows read in place from their
// [N_cache, row] caches through the same idx; relu_mask folds the block's final ReLU
// backward; double workgroup partials in ws summed in index order by a finalize launch, or
// by a kind-0 finalize task when deferral is on (fin_tasks.h).  fisher_diag is one pass of
// 16 B/elem (pred, target row, Fisher row in, gradient out).  fisher_full is two dependent
// passes -- 12 B/elem for the per-sample sums, 16 B/elem for the gradient -- as two
// launches: the per-(sample, chunk) partials of s_n cross the launch boundary, never a
// workgroup hand-off inside one launch.
#include "fin_tasks.h"
#include "ssq_common.h"

namespace ssq {

struct FisRows {
  const int64_t* idx;   // nullptr: tgt / fis are the batch itself
  uint32_t row;
  FastDiv div_row;
};

template <bool GATHER>
__device__ __forceinline__ int64_t fis_index(uint32_t i, const FisRows& r) {
  if (!GATHER) return i;
  const uint32_t q = fdiv(i, r.div_row);
  return r.idx[q] * (int64_t)r.row + (i - q * r.row);
}

__device__ __forceinline__ float diag_elem(float x, float t, float g, float inv_m, float gs,
                                           int relu_mask, double& acc) {
  const float d = __fsub_rn(x, t);
  const float g2 = __fmul_rn(g, g);
  const double dd = (double)x - (double)t, gg = (double)g;   // exact: the loss in double
  acc += (dd * dd) * (gg * gg);
  const float gv = __fmul_rn(__fmul_rn(__fmul_rn(inv_m, g2), __fmul_rn(2.0f, d)), gs);
  return (relu_mask && x <= 0.0f) ? 0.0f : gv;
}

// float4 body over the first n & ~3 elements (when aligned), scalar tail; one double partial
// per block.  GATHER: r4 is in float4 units in the body, r1 in elements in the tail.
template <bool GATHER>
__global__ __launch_bounds__(kBlock) void fisher_diag_kernel(
    const float* __restrict__ pred, const float* __restrict__ tgt, const float* __restrict__ fis,
    int64_t n, float inv_m, float* __restrict__ grad, const float* __restrict__ gscale,
    int relu_mask, int vec, FisRows r4, FisRows r1, double* __restrict__ part) {
  __shared__ double red[16];
  double acc = 0.0;
  const float gs = gscale ? gscale[0] : 1.0f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n4 = vec ? n >> 2 : 0;
  const f32x4* P = (const f32x4*)pred;
  const f32x4* T = (const f32x4*)tgt;
  const f32x4* F = (const f32x4*)fis;
  f32x4* G = (f32x4*)grad;
  for (int64_t i = tid; i < n4; i += stride) {
    const int64_t j = GATHER ? fis_index<GATHER>((uint32_t)i, r4) : i;
    const f32x4 x = __builtin_nontemporal_load(P + i);
    const f32x4 t = __builtin_nontemporal_load(T + j);
    const f32x4 f = __builtin_nontemporal_load(F + j);
    f32x4 g;
    g.x = diag_elem(x.x, t.x, f.x, inv_m, gs, relu_mask, acc);
    g.y = diag_elem(x.y, t.y, f.y, inv_m, gs, relu_mask, acc);
    g.z = diag_elem(x.z, t.z, f.z, inv_m, gs, relu_mask, acc);
    g.w = diag_elem(x.w, t.w, f.w, inv_m, gs, relu_mask, acc);
    if (grad) __builtin_nontemporal_store(g, G + i);
  }
  for (int64_t i = (n4 << 2) + tid; i < n; i += stride) {
    const int64_t j = GATHER ? fis_index<GATHER>((uint32_t)i, r1) : i;
    const float g = diag_elem(pred[i], tgt[j], fis[j], inv_m, gs, relu_mask, acc);
    if (grad) grad[i] = g;
  }
  if (!part) return;
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// the loss partials summed in index order (fin_tasks.h fin_loss, as K11's finalize)
__global__ void fisher_finalize(const double* __restrict__ part, int nblk, double m,
                                float* __restrict__ out) {
  fin_loss(part, nblk, m, out);
}

// fisher_full's task t = sample * chunks + chunk: elements [chunk * len, min(row, + len)) of
// one sample, len a multiple of 4.  Both passes walk the same tasks, workgroup b taking
// t = b, b + gridDim.x, ...
struct FullGeo {
  int64_t row;        // elements per sample
  int64_t len;        // elements per chunk
  int chunks;         // chunks per sample
  int64_t tasks;      // samples * chunks
};

// PASS 1: sp[t] = sum a*|g| over the task's elements.  PASS 2: s_n = sp[n*chunks + 0..] added
// in index order, the gradient, and the workgroup's loss partial sum s_n * a*|g|.
template <int PASS>
__global__ __launch_bounds__(kBlock) void fisher_full_kernel(
    const float* __restrict__ pred, const float* __restrict__ tgt, const float* __restrict__ fis,
    const int64_t* __restrict__ idx, FullGeo geo, double gcoef, float* __restrict__ grad,
    const float* __restrict__ gscale, int relu_mask, int vec, double* __restrict__ sp,
    double* __restrict__ part) {
  __shared__ double red[16];
  const float gs = (PASS == 2 && gscale) ? gscale[0] : 1.0f;
  double lacc = 0.0;
  for (int64_t t = blockIdx.x; t < geo.tasks; t += gridDim.x) {
    const int64_t smp = t / geo.chunks;
    const int64_t lo = (t - smp * geo.chunks) * geo.len;
    const int64_t cnt = min(geo.len, geo.row - lo);          // >= 1 by the host's geometry
    const int64_t src = (idx ? idx[smp] : smp) * geo.row + lo;
    const float* p = pred + smp * geo.row + lo;
    const float* q = tgt + src;
    const float* f = fis + src;
    float* g = (PASS == 2 && grad) ? grad + smp * geo.row + lo : nullptr;
    double s = 0.0;
    float sc = 0.0f;
    if (PASS == 2) {
      for (int c = 0; c < geo.chunks; ++c) s += sp[smp * geo.chunks + c];
      sc = (float)(s * gcoef);                               // 2 * s_n / (100 * n)
    }
    double acc = 0.0;
    const int64_t c4 = vec ? cnt >> 2 : 0;   // vec: bases 16-B aligned, row and len % 4 == 0
    for (int64_t i = threadIdx.x; i < c4; i += kBlock) {
      const f32x4 x = __builtin_nontemporal_load((const f32x4*)p + i);
      const f32x4 y = __builtin_nontemporal_load((const f32x4*)q + i);
      const f32x4 w = __builtin_nontemporal_load((const f32x4*)f + i);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = __fsub_rn(x[k], y[k]);
        const float aw = fabsf(w[k]);
        acc += fabs((double)x[k] - (double)y[k]) * (double)aw;   // exact difference
        if (PASS == 2) {
          const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
          const float gv = __fmul_rn(__fmul_rn(__fmul_rn(sc, aw), sg), gs);
          o[k] = (relu_mask && x[k] <= 0.0f) ? 0.0f : gv;
        }
      }
      if (PASS == 2 && g) __builtin_nontemporal_store(o, (f32x4*)g + i);
    }
    for (int64_t i = (c4 << 2) + threadIdx.x; i < cnt; i += kBlock) {
      const float x = p[i];
      const float y = q[i];
      const float d = __fsub_rn(x, y);
      const float aw = fabsf(f[i]);
      acc += fabs((double)x - (double)y) * (double)aw;
      if (PASS == 2 && g) {
        const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
        const float gv = __fmul_rn(__fmul_rn(__fmul_rn(sc, aw), sg), gs);
        g[i] = (relu_mask && x <= 0.0f) ? 0.0f : gv;
      }
    }
    if (PASS == 1) {
      acc = block_sum(acc, red);
      if (threadIdx.x == 0) sp[t] = acc;
    } else {
      lacc += s * acc;
    }
  }
  if (PASS == 2 && part) {
    lacc = block_sum(lacc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = lacc;
  }
}

constexpr int64_t kFullChunk = 4096;   // elements of a sample one workgroup takes at a time
constexpr int kFullMaxChunks = 64;

static FullGeo full_geo(int64_t n, int64_t N) {
  FullGeo g;
  g.row = n / N;
  int64_t ch = (g.row + kFullChunk - 1) / kFullChunk;
  if (ch > kFullMaxChunks) ch = kFullMaxChunks;
  if (ch < 1) ch = 1;
  int64_t len = (g.row + ch - 1) / ch;
  len = (len + 3) & ~(int64_t)3;
  g.len = len;
  g.chunks = (int)((g.row + len - 1) / len);   // every chunk holds at least one element
  g.tasks = N * g.chunks;
  return g;
}

}  // namespace ssq

using namespace ssq;

extern "C" size_t ssq_fisher_loss_workspace_size(int64_t n, int64_t N) {
  size_t w = kLossBlocks * sizeof(double);
  if (N >= 1 && n >= N && n % N == 0) w += (size_t)full_geo(n, N).tasks * sizeof(double);
  return w;
}

static int fisher_finish(const char* what, hipStream_t s, double* part, int grid, double m,
                         float* loss_out) {
  if (!loss_out) return check_launch(what);
  if (fin_defer_on()) {
    FinTask t{};
    t.kind = 0;
    t.nwg = 1;
    t.part = part;
    t.a = (uint32_t)grid;
    t.m = m;
    t.o[0] = loss_out;
    const int rc = check_launch(what);
    return rc ? rc : fin_push(s, t);
  }
  hipLaunchKernelGGL(fisher_finalize, dim3(1), dim3(kBlock), 0, s, (const double*)part, grid, m,
                     loss_out);
  return check_launch(what);
}

static int fisher_diag(const char* what, const float* pred, const float* tgt, const float* fis,
                       const int64_t* idx, int64_t row, int64_t n, int64_t M, float* loss_out,
                       float* grad, const float* gscale, int relu_mask, void* ws, size_t ws_bytes,
                       hipStream_t s) {
  SSQ_REQUIRE(pred && tgt && fis && n >= 1 && M >= 1 && (loss_out || grad), SSQ_E_ARG,
              "%s: bad args", what);
  SSQ_REQUIRE(!loss_out || (ws && ws_bytes >= kLossBlocks * sizeof(double)), SSQ_E_WS,
              "%s: workspace too small", what);
  const bool gather = idx != nullptr;
  SSQ_REQUIRE(!gather || (row >= 1 && n % row == 0 && n < (1ll << 31)), SSQ_E_ARG,
              "%s: n must be a whole number of cache rows (< 2^31 elements)", what);
  {  // a queued loss task reads the workspace this launch is about to overwrite
    const int rc = fin_flush(s);
    if (rc) return rc;
  }
  const int grid = grid_for(n, kBlock * 4, kLossBlocks);
  const float inv_m = 1.0f / (float)M;  // mean backward: 1.0 / numel in fp32
  double* part = loss_out ? (double*)ws : nullptr;
  int vec = ((((uintptr_t)pred) | ((uintptr_t)tgt) | ((uintptr_t)fis) | ((uintptr_t)grad)) & 15) == 0;
  if (gather && row % 4 != 0) vec = 0;  // float4s must not straddle cache rows
  FisRows r4{idx, 1, make_fastdiv(1)}, r1 = r4;
  if (gather) {
    r1 = FisRows{idx, (uint32_t)row, make_fastdiv((uint32_t)row)};
    if (vec) r4 = FisRows{idx, (uint32_t)(row / 4), make_fastdiv((uint32_t)(row / 4))};
  }
  auto k = gather ? fisher_diag_kernel<true> : fisher_diag_kernel<false>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, s, pred, tgt, fis, n, inv_m, grad, gscale,
                     relu_mask, vec, r4, r1, part);
  return fisher_finish(what, s, part, grid, (double)M, loss_out);
}

extern "C" int ssq_fisher_diag_loss(const float* pred, const float* tgt, const float* fis,
                                    int64_t n, int64_t M, float* loss_out, float* grad,
                                    const float* gscale, int relu_mask, void* ws, size_t ws_bytes,
                                    ssq_stream_t stream) {
  return fisher_diag("ssq_fisher_diag_loss", pred, tgt, fis, nullptr, 0, n, M, loss_out, grad,
                     gscale, relu_mask, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int ssq_fisher_diag_loss_rows(const float* pred, const float* tgt_cache,
                                         const float* fis_cache, const int64_t* idx, int64_t row,
                                         int64_t n, int64_t M, float* loss_out, float* grad,
                                         const float* gscale, int relu_mask, void* ws,
                                         size_t ws_bytes, ssq_stream_t stream) {
  SSQ_REQUIRE(idx, SSQ_E_ARG, "ssq_fisher_diag_loss_rows: idx is required");
  return fisher_diag("ssq_fisher_diag_loss_rows", pred, tgt_cache, fis_cache, idx, row, n, M,
                     loss_out, grad, gscale, relu_mask, ws, ws_bytes, (hipStream_t)stream);
}

static int fisher_full(const char* what, const float* pred, const float* tgt, const float* fis,
                       const int64_t* idx, int64_t n, int64_t N, int ndim, float* loss_out,
                       float* grad, const float* gscale, int relu_mask, void* ws, size_t ws_bytes,
                       hipStream_t s) {
  SSQ_REQUIRE(ndim == 4, SSQ_E_ARG,
              "%s: a 4-D prediction is required (the per-sample sum runs over dims 1, 2, 3)", what);
  SSQ_REQUIRE(pred && tgt && fis && N >= 1 && n >= N && n % N == 0 && (loss_out || grad),
              SSQ_E_ARG, "%s: bad args", what);
  SSQ_REQUIRE(ws && ws_bytes >= ssq_fisher_loss_workspace_size(n, N), SSQ_E_WS,
              "%s: workspace too small", what);
  {
    const int rc = fin_flush(s);
    if (rc) return rc;
  }
  const FullGeo geo = full_geo(n, N);
  const int grid = (int)(geo.tasks < kLossBlocks ? geo.tasks : kLossBlocks);
  double* part = (double*)ws;
  double* sp = part + kLossBlocks;
  const int vec = geo.row % 4 == 0 &&
                  ((((uintptr_t)pred) | ((uintptr_t)tgt) | ((uintptr_t)fis) | ((uintptr_t)grad)) & 15) == 0;
  const double denom = 100.0 * (double)n;
  hipLaunchKernelGGL(fisher_full_kernel<1>, dim3(grid), dim3(kBlock), 0, s, pred, tgt, fis, idx,
                     geo, 0.0, (float*)nullptr, (const float*)nullptr, 0, vec, sp,
                     (double*)nullptr);
  {
    const int rc = check_launch(what);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(fisher_full_kernel<2>, dim3(grid), dim3(kBlock), 0, s, pred, tgt, fis, idx,
                     geo, 2.0 / denom, grad, gscale, relu_mask, vec, sp,
                     loss_out ? part : (double*)nullptr);
  return fisher_finish(what, s, part, grid, denom, loss_out);
}

extern "C" int ssq_fisher_full_loss(const float* pred, const float* tgt, const float* fis,
                                    int64_t n, int64_t N, int ndim, float* loss_out, float* grad,
                                    const float* gscale, int relu_mask, void* ws, size_t ws_bytes,
                                    ssq_stream_t stream) {
  return fisher_full("ssq_fisher_full_loss", pred, tgt, fis, nullptr, n, N, ndim, loss_out, grad,
                     gscale, relu_mask, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int ssq_fisher_full_loss_rows(const float* pred, const float* tgt_cache,
                                         const float* fis_cache, const int64_t* idx, int64_t n,
                                         int64_t N, int ndim, float* loss_out, float* grad,
                                         const float* gscale, int relu_mask, void* ws,
                                         size_t ws_bytes, ssq_stream_t stream) {
  SSQ_REQUIRE(idx, SSQ_E_ARG, "ssq_fisher_full_loss_rows: idx is required");
  return fisher_full("ssq_fisher_full_loss_rows", pred, tgt_cache, fis_cache, idx, n, N, ndim,
                     loss_out, grad, gscale, relu_mask, ws, ws_bytes, (hipStream_t)stream);
}
