/*
 * ssq.h -- C ABI of libssq.so, the MI355X (gfx950) kernels of the shifted-scale
 * PTQ calibration path.  Plain pointers and sizes only: every pointer is DEVICE
 * memory owned by the caller (PyTorch's caching allocator in the Python host layer),
 * borrowed for the duration of the call.  Launches are asynchronous on `stream`
 * (a hipStream_t passed as void*); no entry point allocates or synchronizes, and none
 * keeps state except the opt-in deferred-finalize queue (ssq_set_deferred_finalize), the
 * opt-in deferred prepared forward (ssq_set_deferred_prep_fwd), the opt-in deferred
 * multi-tensor q/dq (ssq_set_deferred_fq_multi) and the armed optimizer step
 * (ssq_adam_arm), so
 * every call is graph-capturable.
 *
 * Return value: 0 on success; a negative SSQ_E* code for an argument error; otherwise
 * the hipError_t of a failed launch.  ssq_last_error() returns a thread-local message.
 *
 * Streams and workspaces (every entry point): calls on one stream run in issue order;
 * calls on different streams may run concurrently provided no two calls in flight share a
 * workspace (`ws`) or an output buffer.  The library holds no device-global state: every
 * reduction's partials -- and the one in-launch last-arriver counter (the epilogue
 * backward's act-delta reduction, zeroed by the launch that writes its partials) -- live in
 * the call's own workspace, which needs no initialisation.  The host-state deferrals and
 * the armed step below are per stream but not thread-safe: issue them from one host thread.
 *
 * The reference (jai1215snu/ShiftedScaleQuantization) is pure PyTorch: it has no FFI.
 * Each entry point below replaces the eager-op sequence cited beside it; the reference
 * "binding" that calls it is the quantizer module's forward/backward, whose Python
 * mirror (shiftedscalequantization_amd.quant) calls this ABI through ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Common geometry: a weight tensor is viewed as (Co, Ci, K) with K = kh*kw (K = 1 for
 * Linear).  "delta_per_ci" selects a delta of shape (Co,) (0) or (Co, Ci) (1, after
 * ChannelQuant.update_delta).  Quantized codes are written as one byte per element:
 * uint8 for asymmetric ranges, int8 (two's complement) for symmetric ones.
 */
#ifndef SSQ_H_
#define SSQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSQ_OK 0
#define SSQ_E_ARG (-1)      /* invalid size / pointer / enum */
#define SSQ_E_WS (-2)       /* workspace too small */

typedef void* ssq_stream_t; /* hipStream_t */

const char* ssq_last_error(void);
int ssq_version(void);
/* Cache-policy variant of the streaming kernels (0 plain, 1 non-temporal); returns the
 * previous value.  Used by bench.py for A/B measurements only.                        */
int ssq_set_variant(int variant);

/* ---------------------------------------------------------------- K1/K2 uniform affine q/dq
 * UniformAffineQuantizer.forward (quant_layer.py:77-98), with round_ste (:18-22):
 *   d = delta[c]*scale; t = x/d; q = clamp((rint(t) - t) + t + zp[c], qmin, qmax);
 *   y = (q - zp[c]) * d
 * (rint(t) - t) + t == rint(t) for finite t and NaN at t = +-inf, as the reference's
 * round_ste; clamp keeps NaN (torch.clamp).  Element i belongs to channel
 * c = (i / inner) % nch   (nch == 1: per-tensor).                                     */
int ssq_fq_fwd(const float* x, float* y, void* codes_or_null, const float* delta,
               const float* zp, int64_t n, int64_t inner, int64_t nch, float scale,
               int qmin, int qmax, ssq_stream_t stream);
/* The same q/dq with plain torch.round (t = +-inf clamps to an edge): ChannelQuant
 * opt_mode 'none' (channelQuant.py:79-94), ChannelQuantAct 'none'
 * (channelQuantAct.py:56-67), AdaRound 'nearest' (adaptive_rounding.py:40-41).       */
int ssq_fq_round_fwd(const float* x, float* y, void* codes_or_null, const float* delta,
                     const float* zp, int64_t n, int64_t inner, int64_t nch, float scale,
                     int qmin, int qmax, ssq_stream_t stream);

/* Several tensors in ONE launch (e.g. every conv weight of a network): segment s is
 * the tensor x[s] (n[s] elements, inner[s] per channel, nch[s] channels). Per-channel
 * delta/zp of the tile a workgroup covers are staged in LDS. Arrays are HOST arrays of
 * length nseg; the pointers they hold are device pointers.                          */
int ssq_fq_fwd_multi(int nseg, const float* const* x, float* const* y,
                     const float* const* delta, const float* const* zp,
                     const int64_t* n, const int64_t* inner, const int64_t* nch,
                     const int* qmin, const int* qmax, ssq_stream_t stream);
/* With this deferral on, ssq_fq_fwd_multi (<= 48 segments) does not launch: it queues its
 * table on its stream, and the next per-tensor ssq_fq_fwd on that stream (float4 path, no
 * codes, the default streaming geometry) runs the table's tiles in extra workgroups of its
 * own launch -- e.g. an activation cache and every weight of a network quantized in one
 * launch (bench.py's step).  Same code: bit-identical outputs.  One table is queued at a
 * time (a second call launches the first); ssq_flush_fq_multi launches a table still queued
 * on `stream`.  The caller must not read the queued outputs before that launch or flush.
 * Host state, not thread-safe; ssq_set_deferred_fq_multi returns the previous setting;
 * turning it off launches a table still queued (on its own stream), and only a table queued
 * under deferral rides on a per-tensor launch. */
int ssq_set_deferred_fq_multi(int on);
int ssq_flush_fq_multi(ssq_stream_t stream);

/* STE backward of ssq_fq_fwd (autograd of quant_layer.py:92-98):
 *   gx = where(qmin <= rint(x/d)+zp <= qmax, gy*d, 0) / d
 *   gdelta[c] = sum gy*(q-zp) - sum g_int*((x/d)/d) ; gzp[c] = sum g_int - sum gy*d
 * gx / gdelta / gzp may each be NULL. Channel reductions are deterministic (fixed
 * order partials in `ws`, reduced in double).                                         */
size_t ssq_fq_bwd_workspace_size(int64_t n, int64_t inner, int64_t nch);
int ssq_fq_bwd(const float* x, const float* gy, const float* delta, const float* zp,
               int64_t n, int64_t inner, int64_t nch, int qmin, int qmax,
               float* gx, float* gdelta, float* gzp, void* ws, size_t ws_bytes,
               ssq_stream_t stream);
/* Backward of q/dq with torch.round instead of round_ste: ChannelQuantAct 'none' mode
 * (quant/channelQuantAct.py:56-67; x / (delta*shiftedScale) rounded with no gradient).
 * Pass delta = the fp32 product delta*shiftedScale.  The gradient wrt x is zero (not
 * written); gdelta = sum gy*(q - zp) is the gradient wrt that product (the caller scales
 * it by shiftedScale, the product's backward); gzp as ssq_fq_bwd.  Workspace as
 * ssq_fq_bwd.                                                                          */
int ssq_fq_round_bwd(const float* x, const float* gy, const float* delta, const float* zp,
                     int64_t n, int64_t inner, int64_t nch, int qmin, int qmax, float* gdelta,
                     float* gzp, void* ws, size_t ws_bytes, ssq_stream_t stream);
/* Per-tensor ssq_fq_bwd for an x that is a ReLU output, with the ReLU backward folded in:
 * gx is written at the ReLU's input (x <= 0 -> 0, torch threshold_backward on the output),
 * bit-identical to ssq_fq_bwd followed by ssq_relu_bwd.  Workspace as ssq_fq_bwd with
 * nch = 1.  Replaces the act quantizer's backward (quant_layer.py:92-98) + the ReLU's
 * (quant_block.py:117, QuantModule activation quant_layer.py:270).                     */
int ssq_fq_relu_bwd(const float* x, const float* gy, const float* delta, const float* zp,
                    int64_t n, int qmin, int qmax, float* gx, float* gdelta, float* gzp,
                    void* ws, size_t ws_bytes, ssq_stream_t stream);
/* The same for x a ReLU6 output (MobileNetV2's QuantInvertedResidual, quant_block.py:
 * 205-239): gx = 0 where x <= 0 or x >= 6 (torch hardtanh_backward).                  */
int ssq_fq_relu6_bwd(const float* x, const float* gy, const float* delta, const float* zp,
                     int64_t n, int qmin, int qmax, float* gx, float* gdelta, float* gzp,
                     void* ws, size_t ws_bytes, ssq_stream_t stream);

/* ---------------------------------------------------------------- K3/K4 scale init
 * init_quantization_scale (quant_layer.py:100-166) for `rows` independent rows of
 * `inner` elements (rows = Co for channel-wise weights, 1 for a per-tensor activation).
 * method 0 = 'max' (fp64 finalize exactly as the host Python; scale_flag = 'scale' in
 * scale_method), 1 = 'mse' (80 shrink candidates, mean |x-q|^2.4, first strict min).
 * Outputs delta, zp, raw_zp: `rows` floats each.  `scores_or_null` receives the
 * rows x 80 candidate scores (mse only) for inspection.                                */
size_t ssq_scale_init_workspace_size(int64_t rows, int64_t inner, int method);
int ssq_scale_init(const float* x, int64_t rows, int64_t inner, int n_bits, int sym,
                   int method, int scale_flag, float* delta, float* zp, float* raw_zp,
                   double* scores_or_null, void* ws, size_t ws_bytes, ssq_stream_t stream);

/* ---------------------------------------------------------------- K5-K9 ChannelQuant
 * Shift-candidate floors are recomputed in-kernel from W:  F_i = floor(W / (delta*s_i)).
 * alpha layout: conv (Ci, S); Linear (Co, Ci, S)  (is_fc = 1).  S <= 8.
 * `shifts` (the shiftTarget list) is a HOST array of S floats; every other pointer is
 * device memory.                                                                      */

/* ChannelQuant.init_v_beta (channelQuant.py:279-294, mode 0) / init_v (:201-213, mode 1)
 * + init_alpha (:158-199) + get_delta (:221-237).  init_alpha's squared error compares W
 * with the integer floors F_i (mode 0, the reference's quirk) or with the dequantized
 * 'none'-mode candidates at delta*s_i (mode 1, uses zp/qmin/qmax).  Writes alpha (init
 * logits), beta (W-shaped, mode 0; may be NULL) and the per-(Ci,S) (conv) / per-element
 * (fc) squared-error table mse_out (may be NULL).                                      */
size_t ssq_shift_init_workspace_size(int64_t Co, int64_t Ci, int64_t K, int S, int is_fc);
int ssq_shift_init(const float* W, const float* delta, const float* zp, const float* shifts,
                   int S, int64_t Co, int64_t Ci, int64_t K, int is_fc, int mode, int qmin,
                   int qmax, float* alpha, float* beta, float* mse_out, void* ws,
                   size_t ws_bytes, ssq_stream_t stream);

/* ChannelQuant.init_beta (channelQuant.py:300-307) / AdaRoundQuantizer.init_alpha
 * (adaptive_rounding.py:66-74): beta = -log((zeta-gamma)/(rest-gamma) - 1).           */
int ssq_rect_init(const float* W, const float* delta, int delta_per_ci, int64_t Co,
                  int64_t Ci, int64_t K, float* beta, ssq_stream_t stream);

/* ChannelQuant.get_delta (channelQuant.py:221-237): out (Co, Ci) = delta * s[argmax p].*/
int ssq_get_delta(const float* delta, const float* alpha, const float* shifts, int S,
                  int64_t Co, int64_t Ci, int is_fc, float* out, ssq_stream_t stream);

/* ChannelQuant.forward 'adaShift' (channelQuant.py:51-64, shifted_x_quant :96-118):
 *   Xf = hard_targets ? F_{argmax p} : sum_i F_i * p_i   (separate fp32 roundings)
 *   Q  = clamp(Xf + (hard_round ? [beta>=0] : h(beta)) + zp, qmin, qmax)
 *   What = (Q - zp) * delta                                                           */
int ssq_adashift_fwd(const float* W, const float* alpha, const float* beta,
                     const float* delta, const float* zp, const float* shifts, int S,
                     int64_t Co, int64_t Ci, int64_t K, int is_fc, int hard_targets,
                     int hard_round, int qmin, int qmax, float* What, void* codes_or_null,
                     ssq_stream_t stream);

/* Backward of the soft-target adaShift forward wrt alpha (and beta if gbeta != NULL).
 * Conv alpha gradients are reduced over (Co, K) deterministically in two fixed-order
 * stages through `ws` (ssq_adashift_bwd_workspace_size bytes; 0 for Linear).
 * Fused shift regulariser (layer_recon_fused_shiftedScale.py:281-282), applied when
 * lambda != 0:  reg = lambda * sum(1 - |2p-1|^b);  its gradient is added to galpha and
 * per-alpha-row values are written to reg_vals (may be NULL).  (lambda, b) come from
 * reg_lambda/reg_b, or from the DEVICE pair reg_dev[0..1] when reg_dev != NULL (the
 * graph-capturable form: the schedule changes every iteration).
 * galpha is OVERWRITTEN (not accumulated).                                             */
size_t ssq_adashift_bwd_workspace_size(int64_t Co, int64_t Ci, int64_t K, int S, int is_fc);
int ssq_adashift_bwd(const float* gWhat, const float* W, const float* alpha,
                     const float* beta, const float* delta, const float* zp,
                     const float* shifts, int S, int64_t Co, int64_t Ci, int64_t K,
                     int is_fc, int hard_round, int qmin, int qmax, float reg_lambda,
                     float reg_b, const float* reg_dev, float* galpha, float* gbeta,
                     float* reg_vals, void* ws, size_t ws_bytes, ssq_stream_t stream);

/* Prepared adaShift (conv weights, S <= 4, K <= 256).  In the fused loop W, delta, the shifts
 * and beta are frozen (layer_recon_fused_shiftedScale.py:59-66) and the reference computes
 * its floor candidates x_q once (channelQuant.py:284-286).  ssq_adashift_prepare does that
 * once: fpack[e] = the S floors floor(W/(delta*s_i)) as int8 bytes (byte i) of one 32-bit
 * word, hterm[e] = h(beta) (hard_round: [beta >= 0]).  *overflow (device int, zeroed by the
 * caller) becomes nonzero if a floor does not fit int8 -- the caller then keeps
 * ssq_adashift_fwd/bwd.  The prepared forward / backward give the same What and alpha
 * gradients as ssq_adashift_fwd / ssq_adashift_bwd (beta frozen: no gbeta) while streaming
 * 12 B per weight each.  The _multi forms take nseg weights (e.g. every conv of a block,
 * same S) in ONE forward launch and TWO backward launches; arrays are indexed by segment.
 * The backward reduces over (Co, K) in two fixed-order stages through `ws`; galpha
 * OVERWRITTEN; regulariser as ssq_adashift_bwd (reg_vals may be NULL, or entries NULL). */
int ssq_adashift_prepare(const float* W, const float* beta, const float* delta,
                         const float* shifts, int S, int64_t Co, int64_t Ci, int64_t K,
                         int hard_round, uint32_t* fpack, float* hterm, int* overflow,
                         ssq_stream_t stream);
int ssq_adashift_fwd_prepared(const uint32_t* fpack, const float* hterm, const float* alpha,
                              const float* delta, const float* zp, int S, int64_t Co,
                              int64_t Ci, int64_t K, int hard_targets, int qmin, int qmax,
                              float* What, ssq_stream_t stream);
int ssq_adashift_fwd_prepared_multi(int nseg, const uint32_t* const* fpack,
                                    const float* const* hterm, const float* const* alpha,
                                    const float* const* delta, const float* const* zp,
                                    const int64_t* Co, const int64_t* Ci, const int64_t* K,
                                    const int* qmin, const int* qmax, int S, int hard_targets,
                                    float* const* What, ssq_stream_t stream);
size_t ssq_adashift_bwd_prepared_workspace_size(int64_t Co, int64_t Ci, int64_t K, int S);
int ssq_adashift_bwd_prepared(const float* gWhat, const uint32_t* fpack, const float* hterm,
                              const float* alpha, const float* delta, const float* zp, int S,
                              int64_t Co, int64_t Ci, int64_t K, int qmin, int qmax,
                              float reg_lambda, float reg_b, const float* reg_dev,
                              float* galpha, float* reg_vals, void* ws, size_t ws_bytes,
                              ssq_stream_t stream);
size_t ssq_adashift_bwd_prepared_multi_workspace_size(int nseg, const int64_t* Co,
                                                      const int64_t* Ci, const int64_t* K, int S);
int ssq_adashift_bwd_prepared_multi(int nseg, const float* const* gWhat,
                                    const uint32_t* const* fpack, const float* const* hterm,
                                    const float* const* alpha, const float* const* delta,
                                    const float* const* zp, const int64_t* Co, const int64_t* Ci,
                                    const int64_t* K, const int* qmin, const int* qmax, int S,
                                    float reg_lambda, float reg_b, const float* reg_dev,
                                    float* const* galpha, float* const* reg_vals, void* ws,
                                    size_t ws_bytes, ssq_stream_t stream);

/* Shift-regulariser alone (value + gradient wrt alpha), for iterations where the
 * reconstruction gradient is not wanted.  mode 0: lambda*sum(1-|2p-1|^b)
 * (fused loss); mode 1: entropy lambda*-sum(p log(p+1e-10))
 * (layer_recon_shiftedScale.py:393,467).  galpha is ACCUMULATED (+=) if not NULL.     */
int ssq_shift_reg(const float* alpha, int S, int64_t rows, int mode, float lambda, float b,
                  float* galpha, float* reg_vals, ssq_stream_t stream);

/* 'learned_hard_sigmoid' (channelQuant.py:81-82): What = sum_i Xq_i * p_i (or Xq_{argmax})
 * where Xq_i are the DEQUANTIZED candidates of init_v (channelQuant.py:201-213), i.e.
 * 'none'-mode q/dq of W at delta*s_i, recomputed in-kernel.  galpha OVERWRITTEN.      */
int ssq_lhs_fwd(const float* W, const float* alpha, const float* delta, const float* zp,
                const float* shifts, int S, int64_t Co, int64_t Ci, int64_t K, int is_fc,
                int hard_targets, int qmin, int qmax, float* What, ssq_stream_t stream);
int ssq_lhs_bwd(const float* gWhat, const float* W, const float* alpha, const float* delta,
                const float* zp, const float* shifts, int S, int64_t Co, int64_t Ci,
                int64_t K, int is_fc, int qmin, int qmax, float* galpha, void* ws,
                size_t ws_bytes, ssq_stream_t stream);

/* 'adaround' mode (channelQuant.py:65-78) and AdaRoundQuantizer 'learned_hard_sigmoid'
 * (adaptive_rounding.py:38-67):  Q = clamp(floor(W/d) + (hard ? [beta>=0] : h(beta)) + zp)
 * What = (Q - zp)*d, d = delta*scale.  Backward gives gbeta (W-shaped, OVERWRITTEN); with
 * reg_lambda != 0 (or reg_dev != NULL: (lambda, b) read from that DEVICE pair, the
 * graph-capturable form) the gradient of the rounding regulariser
 * lambda*sum(1-|2h(beta)-1|^b) (block_recon.py:171-174) is added in the same pass.      */
int ssq_adaround_fwd(const float* W, const float* beta, const float* delta, int delta_per_ci,
                     const float* zp, float scale, int64_t Co, int64_t Ci, int64_t K,
                     int hard_round, int qmin, int qmax, float* What, void* codes_or_null,
                     ssq_stream_t stream);
int ssq_adaround_bwd(const float* gWhat, const float* W, const float* beta,
                     const float* delta, int delta_per_ci, const float* zp, float scale,
                     int64_t Co, int64_t Ci, int64_t K, int qmin, int qmax, float reg_lambda,
                     float reg_b, const float* reg_dev, float* gbeta, ssq_stream_t stream);
/* Several AdaRound weights (a block's quantizers) in one launch each way (up to 8 per
 * launch, further launches beyond that): arrays of nseg per-weight arguments as in
 * ssq_adaround_fwd / _bwd (scale, qmin, qmax per weight); results bit-identical to one
 * call per weight. */
int ssq_adaround_fwd_multi(int nseg, const float* const* W, const float* const* beta,
                           const float* const* delta, const int* delta_per_ci,
                           const float* const* zp, const float* scale, const int64_t* Co,
                           const int64_t* Ci, const int64_t* K, int hard_round, const int* qmin,
                           const int* qmax, float* const* What, ssq_stream_t stream);
int ssq_adaround_bwd_multi(int nseg, const float* const* gWhat, const float* const* W,
                           const float* const* beta, const float* const* delta,
                           const int* delta_per_ci, const float* const* zp, const float* scale,
                           const int64_t* Co, const int64_t* Ci, const int64_t* K, const int* qmin,
                           const int* qmax, float reg_lambda, float reg_b, const float* reg_dev,
                           float* const* gbeta, ssq_stream_t stream);

/* Rounding regulariser lambda*sum(1-|2h(v)-1|^b) over h = rect_sigmoid(v)
 * (layer_recon_fused_shiftedScale.py:278-279, block_recon.py:171-174,
 * layer_recon_shiftedScale.py:386-387).  loss_out: one float (deterministic).
 * gv (may be NULL) is ACCUMULATED (+=).                                               */
size_t ssq_round_reg_workspace_size(int64_t n);
int ssq_round_reg(const float* v, int64_t n, float lambda, float b, float* loss_out,
                  float* gv, void* ws, size_t ws_bytes, ssq_stream_t stream);

/* ---------------------------------------------------------------- K10 ChannelQuantMSE
 * init_scale 'max' mode (channelQuantMSE.py:203-241): per column j of W viewed as
 * (Co, J) keep the LAST candidate c = k/level (k = level..1) whose normalized codes
 * ((W/c)/delta + zero)/(2^b-1), zero = rint(raw_zp/delta), lie in the open range
 * (-0.5*thr/(2^b-1), 1+0.5*thr/(2^b-1)) over all Co.  inp_scale: J floats.           */
int ssq_inpscale_search(const float* W, const float* delta, const float* raw_zp,
                        int64_t Co, int64_t J, int n_bits, int level, float threshold,
                        float* inp_scale, ssq_stream_t stream);
/* ChannelQuantMSE.forward (channelQuantMSE.py:267-276). */
int ssq_inpscale_fwd(const float* W, const float* inp_scale, const float* delta,
                     const float* raw_zp, int64_t Co, int64_t J, int n_bits, float* What,
                     ssq_stream_t stream);

/* ---------------------------------------------------------------- K11 reconstruction loss
 * lp_loss (quant_layer.py:25-32) value and its gradient wrt pred in one pass:
 *   loss = sum |pred-tgt|^p / M ;  grad = gscale * ((1/M) * (p*|d|^(p-1)) * sgn(d))
 * M = n / C for reduction 'none' (sum over dim 1, mean over the rest), n for 'all'.
 * loss_out / grad / gscale (a DEVICE scalar, the upstream gradient) may each be NULL.
 * relu_mask != 0: pred is the output of a ReLU and grad is written at the ReLU's input
 * (grad = 0 where pred <= 0, torch's threshold_backward) -- the block's final ReLU
 * backward folded into the loss pass.  The loss reduction is deterministic: workgroup
 * partials in ws, summed in index order by a finalize launch (or task, with deferral on). */
size_t ssq_lp_loss_workspace_size(int64_t n);
int ssq_lp_loss(const float* pred, const float* tgt, int64_t n, int64_t M, float p,
                float* loss_out, float* grad, const float* gscale, int relu_mask, void* ws,
                size_t ws_bytes, ssq_stream_t stream);

/* ssq_lp_loss with the target rows read straight from the cached outputs: target element
 * i is tgt_cache[idx[i / row] * row + i % row] (the loop's cached_outs[idx] batch,
 * layer_recon_fused_shiftedScale.py:95-97, without materialising it).  n % row == 0,
 * n < 2^31.  Same values as ssq_gather_rows2 + ssq_lp_loss.                             */
int ssq_lp_loss_rows(const float* pred, const float* tgt_cache, const int64_t* idx, int64_t row,
                     int64_t n, int64_t M, float p, float* loss_out, float* grad,
                     const float* gscale, int relu_mask, void* ws, size_t ws_bytes,
                     ssq_stream_t stream);

/* ---------------------------------------------------------------- K20 Fisher-weighted losses
 * BRECQ's opt_mode 'fisher_diag' / 'fisher_full' (block_recon.py:156-162, layer_recon.py:
 * 144-148): value and gradient wrt pred, with fis = the cached |dKL/d(output)| + 1 rows
 * (data_utils.py:40-71).  loss_out / grad / gscale / relu_mask / ws, the deterministic loss
 * reduction and the deferral rules are ssq_lp_loss's (the finalize is the same kind of task);
 * the _rows forms read BOTH the target and the Fisher rows in place from [N_cache, row]
 * caches through the same idx, as ssq_lp_loss_rows reads its target (n % row == 0, n < 2^31).
 *   fisher_diag: loss = sum (pred-tgt)^2 * fis^2 / M, M = n / C (2-D predictions included);
 *     grad = gscale * ((1/M * fis*fis) * (2*d)), d = pred - tgt: torch autograd's operations
 *     in its order, each rounded to fp32 -- bit-identical to the reference's backward.
 *     One pass, 16 B/elem.
 *   fisher_full: a = |pred-tgt|, s_k = sum over sample k of a*|fis| (N samples of n / N
 *     elements), loss = sum_k s_k * sum(a*|fis|) / (100*n),
 *     grad = gscale * (2*s_k/(100*n) * |fis| * sgn(d)), sgn(0) = 0.  Two launches: the
 *     per-(sample, chunk) partials of s_k in ws (doubles, fixed order), then the gradient and
 *     the loss partials.  ndim is the prediction's rank: anything but 4 is SSQ_E_ARG, as the
 *     reference's torch.sum(..., (1, 2, 3)) raises.  idx holds N entries.
 * ssq_fisher_loss_workspace_size(n, N): bytes either loss needs for n elements in N samples. */
size_t ssq_fisher_loss_workspace_size(int64_t n, int64_t N);
int ssq_fisher_diag_loss(const float* pred, const float* tgt, const float* fis, int64_t n,
                         int64_t M, float* loss_out, float* grad, const float* gscale,
                         int relu_mask, void* ws, size_t ws_bytes, ssq_stream_t stream);
int ssq_fisher_diag_loss_rows(const float* pred, const float* tgt_cache, const float* fis_cache,
                              const int64_t* idx, int64_t row, int64_t n, int64_t M,
                              float* loss_out, float* grad, const float* gscale, int relu_mask,
                              void* ws, size_t ws_bytes, ssq_stream_t stream);
int ssq_fisher_full_loss(const float* pred, const float* tgt, const float* fis, int64_t n,
                         int64_t N, int ndim, float* loss_out, float* grad, const float* gscale,
                         int relu_mask, void* ws, size_t ws_bytes, ssq_stream_t stream);
int ssq_fisher_full_loss_rows(const float* pred, const float* tgt_cache, const float* fis_cache,
                              const int64_t* idx, int64_t n, int64_t N, int ndim,
                              float* loss_out, float* grad, const float* gscale, int relu_mask,
                              void* ws, size_t ws_bytes, ssq_stream_t stream);

/* ---------------------------------------------------------------- K14 batch gather
 * dst_k[r] = src_k[idx[r]] for two sources at once (cached block input and output,
 * layer_recon_fused_shiftedScale.py:95-97). src1/dst1 may be NULL.                    */
int ssq_gather_rows2(const float* src0, float* dst0, int64_t row0, const float* src1,
                     float* dst1, int64_t row1, const int64_t* idx, int64_t nidx,
                     ssq_stream_t stream);
/* The same gather with the indices read from `slot` (one iteration's row of a device ring
 * the host filled for several iterations at once: nidx indices, then the iteration's other
 * words) and slot[0:stage_words] copied to stage_dst in the same launch -- the static words
 * the iteration's later launches read (the loss rows' indices, Adam's step constants).  A
 * loop captured as several iterations per graph replay starts each with this launch
 * (quant/block_recon.py).                                                              */
int ssq_gather_rows2_staged(const float* src0, float* dst0, int64_t row0, const float* src1,
                            float* dst1, int64_t row1, const int64_t* slot, int64_t nidx,
                            int64_t* stage_dst, int64_t stage_words, ssq_stream_t stream);

/* ---------------------------------------------------------------- K19 fused fc iteration
 * One BRECQ AdaRound iteration of a Linear layer (the network's last layer: layer_recon.py
 * :10-104 with its LossFunction :107-170, adaptive_rounding.py:38-67, lp_loss p = 2,
 * quant_layer.py:25-32) in two launches: y = x[idx] What^T + bias and the loss gradient
 * g = dL/dy; then dW = g^T x[idx], V's gradient (AdaRound backward + the rounding
 * regulariser), V's Adam step (exp_avg / exp_avg_sq; ssq_adam's ops), What = AdaRound(W, V)
 * of the updated V for the next call (per-row delta / zp, soft rounding, clamp to
 * [qmin, qmax]; ssq_adaround_fwd's ops -- which also provides the first call's What), and
 * the loss value into loss_out.  `slot` (device) holds the bs batch indices (rows of
 * x_cache [N, Ci] and tgt_cache [N, Co]) followed by the iteration's words as fp32 pairs:
 * (lambda, b) of the regulariser, then Adam's (-lr/bc1, sqrt(bc2)).  g ([bs, Co]) is
 * scratch (and readable); gv_out may receive V's gradient.  1 <= bs <= 64, Ci a multiple
 * of 64 up to 4096; x_cache and What 16-B aligned.  fp32 MFMA (v_mfma_f32_16x16x4_f32):
 * the forward as 16 x 16 output tiles with the K range split over 8 waves, the weight
 * gradient as one 16 x 16 tile per wave; fixed summation orders.                      */
size_t ssq_fc_recon_workspace_size(int64_t Co, int64_t Ci, int64_t bs);
int ssq_fc_recon_iter(const float* x_cache, const float* tgt_cache, const int64_t* slot,
                      int64_t bs, const float* W, float* V, float* What, const float* delta,
                      const float* zp, int qmin, int qmax, const float* bias, int64_t Co,
                      int64_t Ci, float one_minus_beta1, float beta2, float one_minus_beta2,
                      float eps, float* exp_avg, float* exp_avg_sq, float* g, float* gv_out,
                      float* loss_out, void* ws, size_t ws_bytes, ssq_stream_t stream);
/* The same iteration split where V's gradient exists, for data parallel: the reference
 * all-reduces the gradients between err.backward() and optimizer.step()
 * (block_recon.py:100-102).  ssq_fc_recon_grad runs the forward launch and then the
 * backward up to V's gradient, written to gv_out (required; 4-B aligned is enough, so it
 * may be a slice of a flat all-reduce bucket); V, What and Adam's moments are only read or
 * not touched.  Shapes, alignment, slot and workspace as ssq_fc_recon_iter.
 * ssq_fc_recon_apply is the rest, one elementwise launch: V's Adam step from `grad` (any
 * gradient of V's shape, e.g. the reduced one; 4-B aligned, read as float4 when 16-B
 * aligned) and What = AdaRound(W, V) of the updated V for the next ssq_fc_recon_grad; only
 * Adam's words of `slot` (after its bs indices and (lambda, b)) are read.  W, V, What and
 * the moments 16-B aligned.  The per-element operations of the pair are
 * ssq_fc_recon_iter's: fed its own gv_out, the pair gives that call's bits.           */
int ssq_fc_recon_grad(const float* x_cache, const float* tgt_cache, const int64_t* slot,
                      int64_t bs, const float* W, const float* V, const float* What,
                      const float* delta, const float* zp, int qmin, int qmax,
                      const float* bias, int64_t Co, int64_t Ci, float* g, float* gv_out,
                      float* loss_out, void* ws, size_t ws_bytes, ssq_stream_t stream);
int ssq_fc_recon_apply(const float* W, float* V, float* What, const float* delta,
                       const float* zp, int qmin, int qmax, int64_t Co, int64_t Ci,
                       const int64_t* slot, int64_t bs, const float* grad,
                       float one_minus_beta1, float beta2, float one_minus_beta2, float eps,
                       float* exp_avg, float* exp_avg_sq, ssq_stream_t stream);

/* ---------------------------------------------------------------- K13 fused epilogue
 * QuantModule conv bias add (quant_layer.py:250), the block's residual add and ReLU
 * (quant_block.py:99-117) in one pass, in the reference's op order:
 *   out = act((y + bias[c]) + res),  c = (i / hw) % C,
 * act by the `relu` code of every K13 entry point: 0 identity, 1 ReLU, 2 ReLU6 (torch
 * clamp semantics: -0.0 and NaN kept).  bias / res may be NULL.  ssq_relu_bwd: gin =
 * out <= 0 ? 0 : g (torch's ReLU backward on its output); ssq_relu6_bwd: gin = 0 where
 * out <= 0 or out >= 6 (hardtanh_backward).  n < 2^31.                                   */
int ssq_bias_act(const float* y, const float* bias, const float* res, float* out, int64_t n,
                 int64_t hw, int64_t C, int relu, ssq_stream_t stream);
int ssq_relu_bwd(const float* g, const float* out, float* gin, int64_t n, ssq_stream_t stream);
int ssq_relu6_bwd(const float* g, const float* out, float* gin, int64_t n, ssq_stream_t stream);
/* F.max_pool2d forward, NCHW fp32, square K x K window (K <= 7), stride, pad <= K/2, no
 * dilation, floor mode: torch's rule (a larger value or a NaN replaces the running max, ties
 * keep the first, window walked row-major), bit-identical to torch.  The ResNet stem's pool
 * (models/resnet.py's maxpool after the stem; validation common.py:153-221). */
int ssq_maxpool2d_fwd(const float* x, float* y, int64_t N, int64_t C, int64_t H, int64_t W,
                      int64_t K, int64_t stride, int64_t pad, ssq_stream_t stream);
/* ssq_bias_act with the following per-tensor activation fake-quant (quant_layer.py:92-98,
 * applied at quant_layer.py:272 / quant_block.py:118) in the same pass:
 *   yq = (clamp(rint(out/delta[0]) + zp[0], qmin, qmax) - zp[0]) * delta[0]
 * bit-identical to ssq_bias_act + ssq_fq_fwd.  out (the pre-quant activation, needed only
 * by the backward) may be NULL: then the pass reads y (+res) and writes yq alone.        */
int ssq_bias_act_fq(const float* y, const float* bias, const float* res, float* out, float* yq,
                    int64_t n, int64_t hw, int64_t C, int relu, const float* delta,
                    const float* zp, int qmin, int qmax, ssq_stream_t stream);

/* The general epilogue: out = act(((y + bias[c]) * gamma[c] + phi[c]) + res), the
 * QuantModule's gamma^z/phi^z affine (quant_layer.py:266-267, learned with --bias_cal)
 * included, optionally followed by the per-tensor act fake-quant (yq; then out may be
 * NULL).  gamma/phi (both or neither), bias, res, delta/zp may be NULL.  Bit-identical to
 * the reference's separate fp32 ops.                                                     */
int ssq_epilogue_fwd(const float* y, const float* bias, const float* gamma, const float* phi,
                     const float* res, float* out, float* yq, int64_t n, int64_t hw, int64_t C,
                     int relu, const float* delta, const float* zp, int qmin, int qmax,
                     ssq_stream_t stream);
/* Its backward from g = dL/d(output), recomputing the pre-activation from y (NCHW, N x C
 * planes of hw): gy = g_t * gamma[c] (or g_t), gres = g_t, ggamma[c] = sum g_t*(y+bias[c]),
 * gphi[c] = sum g_t, gdelta/gzp as ssq_fq_bwd, where g_t is the act quantizer's STE and the
 * ReLU mask applied to g.  Every output may be NULL (gy: dL/dy not wanted, only the
 * per-channel / quantizer sums are produced).  Per-(n, c) partials in ws
 * (ssq_epilogue_bwd_workspace_size(N*C)), reduced in a fixed order.                     */
size_t ssq_epilogue_bwd_workspace_size(int64_t rows);
/* The form the K13 forward runs for n elements in planes of hw (aligned: every tensor pointer
 * is 16-B aligned; rows: y or res is read through a row map): 0 scalar, 1 float4s with a
 * channel lookup per element, 2 float4s that never straddle a plane (hw % 4 == 0).        */
int ssq_epilogue_fwd_form(int64_t n, int64_t hw, int aligned, int rows);
/* The form the K13 backward (and its fused tail: loss) runs for rows of hw elements: returns
 * 16 (4 rows per wave, 16 lanes per row), 4 (4 rows per wave, a lane per element: the A/B
 * form) or 1 (a row per wave), and in *vec (may be NULL) whether the rows are read as
 * float4s.  quant: an act quantizer; res2: the residual's own epilogue is folded in.      */
int ssq_epilogue_bwd_form(int64_t hw, int aligned, int quant, int res2, int loss, int* vec);
int ssq_epilogue_bwd(const float* g, const float* y, const float* bias, const float* gamma,
                     const float* phi, const float* res, int64_t N, int64_t C, int64_t hw,
                     int relu, const float* delta, const float* zp, int qmin, int qmax, float* gy,
                     float* gres, float* ggamma, float* gphi, float* gdelta, float* gzp, void* ws,
                     size_t ws_bytes, ssq_stream_t stream);
/* The fused tail of a reconstruction iteration: the block's final epilogue forward, the
 * reconstruction loss (power p: 2 in the shifted-scale loops, 2.4 in BRECQ's act phase)
 * against the cached target rows and the epilogue backward, in one pass
 * (layer_recon_fused_shiftedScale.py's quant_out -> lp_loss -> backward; block_recon.py's
 * act branch).  The output is recomputed from y with the forward's ops and never stored;
 * dL/d(output) is ssq_lp_loss_rows's gradient at the same p (mean over M) bit for bit; the
 * loss value Sum|out - tgt|^p / M (row partials summed in row order) goes to loss_out.
 * tgt_cache is [*, C, hw], idx holds the N cached rows of this batch.  Outputs and
 * workspace as ssq_epilogue_bwd.  res_bias / res_gamma+res_phi (any may be NULL; ReLU or
 * identity only): res is the raw output of the block's downsample conv and its own epilogue
 * (bias add, gamma^z/phi^z, no activation: ssq_epilogue_fwd's ops) is applied in the pass;
 * gres is then dL/d(that raw output) and gres_gamma / gres_phi its gamma / phi gradients --
 * bit-identical to running that epilogue forward and backward as two more passes. */
int ssq_epilogue_loss_bwd(const float* tgt_cache, const int64_t* idx, int64_t M, float p,
                          float* loss_out, const float* y, const float* bias, const float* gamma,
                          const float* phi, const float* res, const float* res_bias,
                          const float* res_gamma, const float* res_phi, int64_t N, int64_t C,
                          int64_t hw, int relu, const float* delta, const float* zp, int qmin,
                          int qmax, float* gy, float* gres, float* ggamma, float* gphi,
                          float* gres_gamma, float* gres_phi, float* gdelta, float* gzp,
                          void* ws, size_t ws_bytes, ssq_stream_t stream);
/* The three above reading y and / or res in place from per-sample row caches: with a map,
 * y / res is a [*, C, hw] cache and sample n of the batch is its row y_rows[n] / res_rows[n]
 * (either map may be NULL: that operand is the batch itself).  BRECQ's act phase hands its
 * frozen convs' precomputed outputs and the cached block input to the epilogues this way
 * instead of gathering a batch copy of each (block_recon.py:62-73's cached[idx]); the values
 * and their order are those of the gathered batch, so the results are bit-identical.       */
/* stage_dst (may be NULL): workgroup 0 also copies stage_n int64 words (<= 4096) from
 * stage_src to stage_dst -- a loop replaying several iterations per graph hands each
 * iteration's device words (a ring row, from which this launch takes its row maps) to the
 * static slot its later launches read, without a copy launch of its own.                  */
int ssq_epilogue_fwd_rows(const float* y, const int64_t* y_rows, const float* bias,
                          const float* gamma, const float* phi, const float* res,
                          const int64_t* res_rows, float* out, float* yq, int64_t n, int64_t hw,
                          int64_t C, int relu, const float* delta, const float* zp, int qmin,
                          int qmax, const int64_t* stage_src, int64_t* stage_dst,
                          int64_t stage_n, ssq_stream_t stream);
int ssq_epilogue_bwd_rows(const float* g, const float* y, const int64_t* y_rows,
                          const float* bias, const float* gamma, const float* phi,
                          const float* res, const int64_t* res_rows, int64_t N, int64_t C,
                          int64_t hw, int relu, const float* delta, const float* zp, int qmin,
                          int qmax, float* gy, float* gres, float* ggamma, float* gphi,
                          float* gdelta, float* gzp, void* ws, size_t ws_bytes,
                          ssq_stream_t stream);
int ssq_epilogue_loss_bwd_rows(const float* tgt_cache, const int64_t* idx, int64_t M, float p,
                               float* loss_out, const float* y, const int64_t* y_rows,
                               const float* bias, const float* gamma, const float* phi,
                               const float* res, const int64_t* res_rows,
                               const float* res_bias, const float* res_gamma,
                               const float* res_phi, int64_t N, int64_t C, int64_t hw, int relu,
                               const float* delta, const float* zp, int qmin, int qmax,
                               float* gy, float* gres, float* ggamma, float* gphi,
                               float* gres_gamma, float* gres_phi, float* gdelta, float* gzp,
                               void* ws, size_t ws_bytes, ssq_stream_t stream);

/* ---------------------------------------------------------------- Adam
 * torch.optim.Adam's single-tensor step (the reference's optimizer; block_recon.py:57-60,
 * layer_recon_fused_shiftedScale.py:57/73) over nseg parameter tensors in one launch:
 *   m = m + (1-b1)*(g-m);  v = v*b2 + ((1-b2)*g)*g;  p = p + (nss*m)/(sqrt(v)/bc2s + eps)
 * with nss = -lr/(1-b1^t), bc2s = sqrt(1-b2^t) taken from the DEVICE pair `hyper` when it
 * is not NULL (graph-capturable), else from the scalar arguments.  Arrays are HOST arrays
 * of length nseg holding device pointers.                                               */
int ssq_adam(int nseg, float* const* p, const float* const* g, float* const* m,
             float* const* v, const int64_t* n, float one_minus_beta1, float beta2,
             float one_minus_beta2, float eps, const float* hyper, float neg_step_size,
             float bias_correction2_sqrt, ssq_stream_t stream);
/* The same step, armed instead of launched: ssq_adam_arm records the nseg parameters
 * (p, m, v, n; hyper is required) for `stream`; the next prepared alpha backward on that
 * stream applies the step where each gradient is finalised -- the alpha segments of that
 * launch in their finalisers, gamma^z / phi^z (parameters whose gradients the epilogue
 * backward entry points of that stream produce) in their finalize tasks -- when it can
 * cover EVERY armed parameter, and attaches nothing otherwise.  Same update, same fp32
 * operations as ssq_adam: bit-identical.  ssq_adam_take returns 1 when the armed step ran
 * inside a launch (nothing left to do) and 0 when it did not (the caller launches ssq_adam);
 * either way it disarms.  The gradients are still written.  Host state, not thread-safe. */
int ssq_adam_arm(int nseg, float* const* p, float* const* m, float* const* v, const int64_t* n,
                 float one_minus_beta1, float beta2, float one_minus_beta2, float eps,
                 const float* hyper, ssq_stream_t stream);
int ssq_adam_take(ssq_stream_t stream);

/* ---------------------------------------------------------------- deferred finalizes
 * With deferral on, ssq_lp_loss[_rows] (loss value) and ssq_epilogue_bwd (gamma/phi and act
 * delta/zp gradients) queue their small finalize reduction on the stream instead of
 * launching it; the next ssq_epilogue_bwd or prepared alpha backward on that stream runs
 * the queue in extra workgroups of its own launch (same code and order: bit-identical).
 * ssq_adam, the lp_loss entry points and ssq_flush_finalize launch what is still queued.
 * The caller must give each producer's workspace a slot no other launch writes before the
 * flush, and must flush before reading a queued output on the host or with other kernels
 * (the reconstruction loop: deferral on for its body, flush at its end).  Host state,
 * not thread-safe.  ssq_set_deferred_finalize returns the previous setting; it launches
 * nothing (it takes no stream), so flush every stream with queued tasks before turning
 * deferral off. */
int ssq_set_deferred_finalize(int on);
int ssq_flush_finalize(ssq_stream_t stream);

/* ---------------------------------------------------------------- deferred prepared forward
 * The fused loop's iteration start in one launch (csrc/prep_ride.h).  With this deferral on,
 * ssq_adashift_fwd_prepared_multi (<= 8 segments) does not launch: it queues its table on
 * its stream, and the next ssq_gather_rows2 on that stream runs it in extra workgroups of
 * the gather launch (same code: bit-identical What).  One table is queued at a time (a second
 * call launches the first); ssq_flush_prep_fwd launches a table still queued on `stream`.
 * The caller must not read the queued What before that gather or flush.  Host state, not
 * thread-safe; ssq_set_deferred_prep_fwd returns the previous setting; turning it off
 * launches a forward still queued (on its own stream).  Replaces nothing in the reference: the iteration start of
 * layer_recon_fused_shiftedScale.py:94-100 (batch draw, then the quantized forward). */
int ssq_set_deferred_prep_fwd(int on);
int ssq_flush_prep_fwd(ssq_stream_t stream);

/* ---------------------------------------------------------------- K17 conv weight gradient
 * Deterministic fp32 conv weight gradient (NCHW, dilation 1) on the fp32 matrix cores:
 *   dw[co, ci, r, s] = sum_{n,oh,ow} dy[n, co, oh, ow] * x[n, g*Cig + ci, oh*st + r - pad,
 *                                                          ow*st + s - pad]
 * (the autograd of the reconstruction loops' F.conv2d weight, quant_layer.py:250, under
 * the reference's cudnn.deterministic = True, common.py:77-85).  Split-K partials in ws,
 * summed in a fixed order: bit-identical run to run.  Tensors < 2^31 elements; H != W, R != S
 * and any stride >= 1 are taken (the band kernel: 3x3 / pad 1 / stride 1-2 only).  There is
 * no bound on OW as such: the 1x1, im2col-DMA and depthwise kernels take any width (depthwise:
 * a padded plane <= 128 KiB), and the input-row-tile kernel refuses a shape -- workspace size
 * 0, SSQ_E_ARG -- only when the (W + 2 pad)-wide input rows of one pixel chunk, for the input
 * channels of one column tile, do not fit its 160 KiB LDS tile (a 3x3 / 64-channel conv:
 * W about 150; 4 channels: about 1000). */
/* A/B knob (returns the previous value; out-of-range values only query): non-depthwise
 * weight-gradient form, 0 auto, 1 input-row-tile kernel (+ 1x1 GEMM), 2 im2col-DMA kernel,
 * 3 band kernel (3x3 / pad 1 / stride 1-2 / Cin, Cout multiples of 32; others as 1), 4 the
 * band kernel at 4 waves per workgroup instead of 8 (same bits). */
int ssq_conv_wgrad_set_form(int form);
/* The kernel ssq_conv_wgrad runs for a shape under the current form: 0 unsupported,
 * 1 input-row tile, 2 im2col-DMA, 3 band (16-byte staging), 4 1x1 GEMM, 5 depthwise
 * reduction, 6 band (4-byte staging: planes whose rows are not 16-B aligned). */
int ssq_conv_wgrad_kind(int64_t Nb, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t R,
                        int64_t S, int64_t stride, int64_t pad, int64_t groups);
size_t ssq_conv_wgrad_workspace_size(int64_t Nb, int64_t C, int64_t H, int64_t W, int64_t Co,
                                     int64_t R, int64_t S, int64_t stride, int64_t pad,
                                     int64_t groups);
int ssq_conv_wgrad(const float* x, const float* dy, int64_t Nb, int64_t C, int64_t H, int64_t W,
                   int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t groups,
                   float* dw, void* ws, size_t ws_bytes, ssq_stream_t stream);
/* The same weight gradient as one fp32 library GEMM (small output planes, where it beats
 * the band kernel): the two operands, written in one launch,
 *   dy2[co][n*P + p] = dy[n][co][p]                                  (Co x N*P)
 *   col[n*P + p][(ci*R + r)*S + s] = x[n][ci][oh*st+r-pad][ow*st+s-pad] (N*P x C*R*S, 0 outside)
 * with P = OH*OW; then dw = dy2 @ col (Co x C*R*S = dw's layout) by the caller's GEMM.
 * Either output may be NULL (with its input): the forward GEMM y2 = W @ col^T needs col
 * only, a backward with a saved col needs dy2 only.  Ungrouped convs; every operand
 * < 2^31 elements. */
int ssq_wgrad_gemm_operands(const float* x, const float* dy, int64_t Nb, int64_t C, int64_t H,
                            int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride,
                            int64_t pad, float* col, float* dy2, ssq_stream_t stream);
/* The im2col matrix col (N*OH*OW x C*R*S) of epilogue(y): y is the previous conv's raw
 * output and the epilogue the K13 one (ssq_epilogue_fwd's bias, gamma^z / phi^z, activation
 * and per-tensor act fake-quant, each optional: bias / gamma+phi / delta+zp may be NULL),
 * applied on the fly with the same fp32 ops -- col is bit for bit the im2col of the
 * materialised epilogue output, which is never written (ResNet BasicBlock conv1 -> conv2 on
 * the small planes: quant_layer.py:250-272 then conv2's F.conv2d, quant_block.py:99-117). */
int ssq_gemm_col_epilogue(const float* y, const float* bias, const float* gamma,
                          const float* phi, int relu, const float* delta, const float* zp,
                          int qmin, int qmax, int64_t Nb, int64_t C, int64_t H, int64_t W,
                          int64_t R, int64_t S, int64_t stride, int64_t pad, float* col,
                          ssq_stream_t stream);

/* ---------------------------------------------------------------- K18 depthwise conv
 * Depthwise (groups == C == Co) fp32 NCHW conv, dilation 1, R*S <= 25, zero padding:
 *   y[n,c,oh,ow] = sum_{r,s} w[c,r,s] * x[n,c,oh*st+r-pad, ow*st+s-pad]
 * and its input gradient dx (the same sum transposed).  The MobileNetV2 blocks' depthwise
 * F.conv2d of QuantModule.forward (quant_layer.py:250) and its autograd; one plane per
 * workgroup staged in LDS ((H+2pad)*(W+2pad)*4 <= 128 KiB).  Deterministic.           */
/* 1 when both the forward and the input-gradient plan of this depthwise shape fit the
 * 128 KiB LDS stage (weight rows + zero-padded / margined planes), else 0 -- the caller
 * then keeps MIOpen.                                                                    */
int ssq_dwconv_supported(int64_t Nb, int64_t C, int64_t H, int64_t W, int64_t R, int64_t S,
                         int64_t stride, int64_t pad);
int ssq_dwconv_fwd(const float* x, const float* w, float* y, int64_t Nb, int64_t C, int64_t H,
                   int64_t W, int64_t R, int64_t S, int64_t stride, int64_t pad,
                   ssq_stream_t stream);
int ssq_dwconv_bwd_data(const float* dy, const float* w, float* dx, int64_t Nb, int64_t C,
                        int64_t H, int64_t W, int64_t R, int64_t S, int64_t stride, int64_t pad,
                        ssq_stream_t stream);

/* ---------------------------------------------------------------- K15/K16 packed export
 * Low-bit weight export (replaces the fp32 state_dict + pickled shift
 * choice of main_cifar10.py:86 / myScaledMethods.py:204-205).  A hard weight quantizer's
 * output is W_hat = ((q - zp[co]) * d1) (* d2[j]) with d1 per co (d1_per_ci = 0) or per
 * (co, ci) (= 1) and the optional column scale d2 (ChannelQuantMSE's inp_scale, j in
 * [0, Ci*K)).  Codes are stored as q - qmin in ssq_pack_bits(n_bits) = 2 / 4 / 8 bits each,
 * little-endian, ssq_pack_bytes(n, n_bits) bytes for n codes.
 * ssq_pack_encode recovers q from W_hat and ADDS to *mismatch (device u32, caller-zeroed)
 * the number of elements whose decode is not bit-identical to W_hat (0 = exact export).
 * ssq_pack_decode writes W_hat back.  Co*Ci*K < 2^31.                                    */
int ssq_pack_bits(int n_bits);
size_t ssq_pack_bytes(int64_t n, int n_bits);
int ssq_pack_encode(const float* What, const float* zp, const float* d1, int d1_per_ci,
                    const float* d2, int64_t Co, int64_t Ci, int64_t K, int n_bits, int qmin,
                    int qmax, void* packed, uint32_t* mismatch, ssq_stream_t stream);
int ssq_pack_decode(const void* packed, const float* zp, const float* d1, int d1_per_ci,
                    const float* d2, int64_t Co, int64_t Ci, int64_t K, int n_bits, int qmin,
                    float* What, ssq_stream_t stream);

/* ---------------------------------------------------------------- K21-K23 integer inference
 * A layer whose input is an act quantizer's output x_hat = (q_a - z_a) * delta_a (scalar
 * delta_a, integer z_a) and whose weight is a packed export W_hat = (q_w - z_w[co]) * d1[co]
 * (d1 per co, no column scale) computes, with groups == 1, dilation 1, R, S <= 7 and
 * K = Ci*R*S <= 65536,
 *     y[n,co,oh,ow] = fp32(I) * scale[co],  I = sum_{r,s,ci} (q_a - z_a)(q_w - z_w[co]),
 * I exact (int8 MFMA, i32 accumulation, int64 epilogue), converted to fp32 once (round to
 * nearest even) and multiplied once by the caller's scale[co] = fp32(delta_a * d1[co]): no
 * bias, no FMA, reproducible bit for bit from a host integer reference.  A zero-padded tap
 * contributes (q_a - z_a) = 0.  A Linear is the 1x1 conv on a 1x1 plane.
 *
 * K21 act_encode: fp32 NCHW (or (N, C) with H = W = 1) -> int8 codes in NHWC order with C
 * padded to qinfer_cpad(C) = 16*ceil(C/16): q = clamp(rint(x/delta) + zp, qmin, qmax) stored as
 * q - (qmin + 128), padded channels 0.  ADDS to *bad (device u32, caller-zeroed) the number
 * of elements whose (q - zp) * delta is not bit-identical to x; NaN / +-inf are counted and
 * stored as qmin.  qmax - qmin <= 255, zp an integer in [qmin, qmin + 255] (a padded tap
 * stores zp - (qmin + 128) as an int8), N*H*W*Cpad < 2^31.
 *
 * K22 qweight_prepare (once per layer): packed codes (K15's layout: (co, ci, r, s) order,
 * stored as q - qmin) + zp[co] -> the conv kernel's operand, qweight_prepared_bytes(Co, Ci,
 * R, S) bytes: int8 q - (qmin + 128) as [64*ceil(Co/64)][64*ceil(R*S*Cpad/64)] with
 * k = (r*S + s)*Cpad + ci (zero outside the real taps), the 0/1 row of real k, and the two
 * per-channel int32 vectors of the epilogue (csrc/qinfer.hip).  qmin is 0 or -2^(n_bits-1).
 * ADDS to *bad the number of channels whose zp is not an integer in [qmin-256, qmin+511].
 *
 * K23 qconv_i8_fwd: codes (K21) x prepared (K22) -> y, fp32 NCHW (or (N, Co)).  The
 * activation quantizer's (zero point, qmin, qmax) are those given to K21.  Host-side checks
 * before the launch (SSQ_E_ARG): null pointer, groups != 1, K > 65536, R or S > 7, a
 * zero point that is not an integer in [qmin, qmin + 255].                                    */
int64_t ssq_qinfer_cpad(int64_t C);
size_t ssq_qweight_prepared_bytes(int64_t Co, int64_t Ci, int64_t R, int64_t S);
int ssq_act_encode(const float* x, int64_t Nb, int64_t C, int64_t H, int64_t W, float delta,
                   float zero_point, int qmin, int qmax, int8_t* codes, uint32_t* bad,
                   ssq_stream_t stream);
int ssq_qweight_prepare(const void* packed, const float* zp, int64_t Co, int64_t Ci, int64_t R,
                        int64_t S, int n_bits, int qmin, void* prepared, uint32_t* bad,
                        ssq_stream_t stream);
int ssq_qconv_i8_fwd(const int8_t* codes, const void* prepared, const float* scale, int64_t Nb,
                     int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S,
                     int64_t stride, int64_t pad, int64_t groups, float act_zero_point,
                     int act_qmin, int act_qmax, float* y, ssq_stream_t stream);

/* ---------------------------------------------------------------- K24-K26 grouped integer inference
 * The same contract for a conv with groups = G >= 2, Cig = C/G, Cog = Co/G: output channel co
 * belongs to group co / Cog and I runs over that group's K = Cig*R*S taps.  The activation
 * operand is K21's, unchanged (dense NHWC int8, C padded to qinfer_cpad(C) at the end only),
 * so one encode serves every consumer.
 *
 * qconv_grouped_kind(Co, Cig, groups): the kernel prepare and conv both take -- 1 the direct
 * depthwise kernel (Cig == 1 and Co == groups), 2 the grouped int8-MFMA kernel (every other
 * groups >= 2), 0 invalid (groups < 2, Co or Cig < 1, Co % groups != 0).
 *
 * K24 qweight_prepare_grouped (once per layer): the export's packed codes as stored, bit
 * offset ((co*Cig + ci)*R*S + tap)*bs, + zp[co] -> qweight_prepared_bytes_grouped(Co, Cig, R,
 * S, groups) bytes (0 on invalid geometry) in a layout private to the kind
 * (csrc/qinfer_grouped.hip).  ADDS to *bad the number of channels whose zp is not an integer in
 * [qmin-256, qmin+511], as K22 does.
 *
 * K25 / K26 qconv_i8_grouped_fwd: codes (K21, C channels) x prepared (K24) -> y, fp32 NCHW.
 * Host-side checks before the launch (SSQ_E_ARG): null pointer, groups < 2 (groups == 1 is
 * ssq_qconv_i8_fwd), C or Co not divisible by groups, R or S outside [1, 7], Cig*R*S > 65536,
 * a tensor of 2^31 elements or more, a zero point that is not an integer in [qmin, qmin+255]. */
int ssq_qconv_grouped_kind(int64_t Co, int64_t Cig, int64_t groups);
size_t ssq_qweight_prepared_bytes_grouped(int64_t Co, int64_t Cig, int64_t R, int64_t S,
                                          int64_t groups);
int ssq_qweight_prepare_grouped(const void* packed, const float* zp, int64_t Co, int64_t Cig,
                                int64_t R, int64_t S, int64_t groups, int n_bits, int qmin,
                                void* prepared, uint32_t* bad, ssq_stream_t stream);
int ssq_qconv_i8_grouped_fwd(const int8_t* codes, const void* prepared, const float* scale,
                             int64_t Nb, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t R,
                             int64_t S, int64_t stride, int64_t pad, int64_t groups,
                             float act_zero_point, int act_qmin, int act_qmax, float* y,
                             ssq_stream_t stream);

/* ---------------------------------------------------------------- carried codes (fused requantize)
 * The integer convs with the consumer's operand as their output: for the exact sum I of
 * channel co, in this fp32 operation order (csrc/qinfer_epi.h),
 *     y = fp32(I) * scale[co];  pre = y + bias[co] (bias != NULL);
 *     t = pre * gamma[co] + phi[co] (two roundings; gamma and phi both or neither);
 *     t = act(t), act 0 identity / 1 ReLU / 2 ReLU6;
 *     q = clamp(round_ste(t / out_delta) + out_zero_point, out_qmin, out_qmax)
 * and out_codes receives q - (out_qmin + 128) in K21's layout, NHWC int8 with Co padded to
 * qinfer_cpad(Co), padded channels 0: what ssq_act_encode derives from the K13 epilogue's
 * fp32 output whenever it counts nothing off-grid.  A NaN q (a NaN bias, an infinite
 * t / out_delta) is stored as out_qmin and ADDED to *bad (device u32), as K13 followed by K21
 * leaves it.  The first sixteen arguments and their checks are those of ssq_qconv_i8_fwd /
 * ssq_qconv_i8_grouped_fwd; the output quantizer is checked as ssq_act_encode checks its own
 * (delta positive and finite, zero point an integer in [qmin, qmin + 255], qmax - qmin <= 255).
 * No allocation, no sync, capturable.
 *
 * act_decode, K21's inverse: NHWC codes (C padded) -> fp32 NCHW (q - zero_point) * delta,
 * q = code + qmin + 128.                                                                      */
int ssq_qconv_i8_codes_fwd(const int8_t* codes, const void* prepared, const float* scale,
                           int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R,
                           int64_t S, int64_t stride, int64_t pad, int64_t groups,
                           float act_zero_point, int act_qmin, int act_qmax, const float* bias,
                           const float* gamma, const float* phi, int act, float out_delta,
                           float out_zero_point, int out_qmin, int out_qmax, int8_t* out_codes,
                           uint32_t* bad, ssq_stream_t stream);
int ssq_qconv_i8_grouped_codes_fwd(const int8_t* codes, const void* prepared, const float* scale,
                                   int64_t Nb, int64_t C, int64_t H, int64_t W, int64_t Co,
                                   int64_t R, int64_t S, int64_t stride, int64_t pad,
                                   int64_t groups, float act_zero_point, int act_qmin,
                                   int act_qmax, const float* bias, const float* gamma,
                                   const float* phi, int act, float out_delta,
                                   float out_zero_point, int out_qmin, int out_qmax,
                                   int8_t* out_codes, uint32_t* bad, ssq_stream_t stream);
int ssq_act_decode(const int8_t* codes, int64_t Nb, int64_t C, int64_t H, int64_t W, float delta,
                   float zero_point, int qmin, float* x, ssq_stream_t stream);

/* ---------------------------------------------------------------- carried block tails
 * ssq_qconv_i8_codes_fwd with K13's residual add: t = t + rv between the affine and the
 * activation, one more fp32 rounding, so out_codes is what ssq_act_encode derives from the
 * K13 epilogue run with that residual.  Exactly one residual pointer is non-null:
 *   res_f32    fp32 NCHW [Nb, Co, OH, OW] (a downsample branch's output, an fp32 block input);
 *              rv is the element itself, res_delta .. res_qmax are not read;
 *   res_codes  int8 NHWC [Nb*OH*OW][qinfer_cpad(Co)] in K21's stored form (a carried block
 *              input) with its own quantizer: rv = (q_r - res_zero_point) * res_delta,
 *              q_r = code + res_qmin + 128, the value ssq_act_decode writes.
 * groups must be 1 (the dense kernel K23).  The residual quantizer is checked as the output
 * one: res_delta positive and finite, res_zero_point an integer in [res_qmin, res_qmin + 255],
 * res_qmax - res_qmin <= 255.  A NaN q (now also from a NaN residual) is stored as out_qmin
 * and ADDED to *bad.  Every refusal is SSQ_E_ARG before any launch.  No allocation, no sync,
 * capturable.                                                                                 */
int ssq_qconv_i8_codes_res_fwd(const int8_t* codes, const void* prepared, const float* scale,
                               int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                               int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t groups,
                               float act_zero_point, int act_qmin, int act_qmax,
                               const float* bias, const float* gamma, const float* phi, int act,
                               float out_delta, float out_zero_point, int out_qmin, int out_qmax,
                               int8_t* out_codes, uint32_t* bad, const float* res_f32,
                               const int8_t* res_codes, float res_delta, float res_zero_point,
                               int res_qmin, int res_qmax, ssq_stream_t stream);

/* ---------------------------------------------------------------- carried stem (K27, K28)
 * ssq_epilogue_codes_fwd (K27): the K13 epilogue of an fp32 conv output y (NCHW [Nb, C, H, W])
 * leaving as K21's stored codes: the operation list above from `pre = y + bias[c]` on, the same
 * device function the integer kernels' code epilogue runs.  out_codes is NHWC int8
 * [Nb*H*W][qinfer_cpad(C)], padded channels 0, every byte written: what ssq_act_encode derives
 * from K13's fp32 output whenever it counts nothing off-grid; a NaN q is stored as out_qmin
 * and ADDED to *bad.  The output quantizer is checked as by ssq_qconv_i8_codes_fwd.
 *
 * ssq_maxpool_i8_fwd (K28): max-pool on stored codes, codes NHWC [Nb, H, W, qinfer_cpad(C)] ->
 * out [Nb, OH, OW, qinfer_cpad(C)], ssq_maxpool2d_fwd's geometry (square window K <= 7,
 * 2 * pad <= K, stride >= 1, floor mode, no dilation).  The per-channel signed byte maximum
 * over the in-bounds taps; since the stored form is the code shifted by one constant and
 * (q - z) * delta is non-decreasing in q, out is what ssq_act_encode derives from the fp32
 * max-pool of the decoded tensor.  Padded channels stay 0.
 *
 * Every refusal (null pointer, bad geometry or quantizer, an empty output, a tensor of 2^31
 * bytes or more) is SSQ_E_ARG before any launch.  No allocation, no sync, capturable.         */
int ssq_epilogue_codes_fwd(const float* y, const float* bias, const float* gamma, const float* phi,
                           int64_t Nb, int64_t C, int64_t H, int64_t W, int act, float out_delta,
                           float out_zero_point, int out_qmin, int out_qmax, int8_t* out_codes,
                           uint32_t* bad, ssq_stream_t stream);
int ssq_maxpool_i8_fwd(const int8_t* codes, int64_t Nb, int64_t C, int64_t H, int64_t W, int64_t K,
                       int64_t stride, int64_t pad, int8_t* out, ssq_stream_t stream);

/* ---------------------------------------------------------------- fused stem (K31)
 * The stem conv itself, on the fp32 MFMA, with a stated summation order.  For an fp32 NCHW image
 * x [Nb, Ci, H, W] and an fp32 OIHW weight w [Co, Ci, R, S], stride (stride_h, stride_w), padding
 * (pad_h, pad_w), dilation 1, groups 1, no bias,
 *     y[n, co, oh, ow] = acc_K,  acc_0 = +0.0f,  acc_{k+1} = fmaf(x_k, w[co, k], acc_k),
 * k over (ci, r, s) in the memory order of w[co], K = Ci*R*S, x_k the pixel under tap k or +0.0f
 * outside the image; one rounding per tap and no other, so a host fmaf loop gives the same bits.
 *
 * ssq_stem_weight_prepare (once per layer): w -> ssq_stem_weight_prepared_bytes(Co, Ci, R, S)
 * bytes in the conv's operand order (csrc/qinfer_layout.h, SLayout); 0 bytes for a geometry
 * outside 1 <= Ci <= 4, 1 <= R, S <= 7, Co >= 1.
 * ssq_stem_conv_fwd: y as fp32 NCHW [Nb, Co, OH, OW].
 * ssq_stem_conv_codes_fwd: qepi_code_y on each accumulator, i.e. ssq_epilogue_codes_fwd's
 * arguments, checks and bytes for that y (NHWC int8 [Nb*OH*OW][qinfer_cpad(Co)], padded channels
 * 0, every byte written, a NaN q stored as out_qmin and ADDED to *bad) without the fp32 tensor.
 *
 * Refused with SSQ_E_ARG before any launch: a null pointer, the geometry above, strides < 1,
 * pad_h >= R or pad_w >= S or negative, an empty output, prepared_bytes below the blob's size, a
 * tensor of 2^31 elements or more.  No allocation, no sync, no float atomics, capturable.      */
size_t ssq_stem_weight_prepared_bytes(int64_t Co, int64_t Ci, int64_t R, int64_t S);
int ssq_stem_weight_prepare(const float* w, int64_t Co, int64_t Ci, int64_t R, int64_t S,
                            void* prepared, ssq_stream_t stream);
int ssq_stem_conv_fwd(const float* x, const void* prepared, size_t prepared_bytes, int64_t Nb,
                      int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S,
                      int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, float* y,
                      ssq_stream_t stream);
int ssq_stem_conv_codes_fwd(const float* x, const void* prepared, size_t prepared_bytes,
                            int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R,
                            int64_t S, int64_t stride_h, int64_t stride_w, int64_t pad_h,
                            int64_t pad_w, const float* bias, const float* gamma, const float* phi,
                            int act, float out_delta, float out_zero_point, int out_qmin,
                            int out_qmax, int8_t* out_codes, uint32_t* bad, ssq_stream_t stream);

/* ---------------------------------------------------------------- uint8 stem (K32)
 * The stem conv of a uint8 image on the int8 MFMA.  The image is x = (u/255 - mean[c]) / std[c]
 * with u [Nb, Ci, H, W] uint8 NCHW, the weight W_hat = (q_w - z_w[co]) * d[co, c] (packed codes as
 * ssq_qweight_prepare takes them; d per co or per (co, ci)).  With the caller's two fp32 tables
 *     M[c] = fp32(255 * mean[c])        s[co, c] = fp32(fp32(1 / fp32(255 * std[c])) * d[co, c])
 * (s as [Co][Ci]) and, per (pixel, co, c) over the taps of the window inside the image, the exact
 * integers B_c = sum (q_w - z_w[co]) and A_c = sum (q_w - z_w[co]) * u (a padded tap is x = 0 and
 * enters neither; |A_c| <= 49 * 767 * 255 < 2^24),
 *     t_c = fp32(A_c) - M[c] * fp32(B_c)
 *     y   = t_0 * s[co, 0];  y = y + t_c * s[co, c],  c = 1 .. Ci - 1 ascending
 * every product, difference and sum rounded once, no FMA: a host float32 loop gives the same bits.
 *
 * ssq_stem_u8_weight_prepare (once per layer): packed codes + zp[co] -> the operand,
 * ssq_stem_u8_weight_prepared_bytes(Co, Ci, R, S) bytes (csrc/qinfer_layout.h, ULayout; 0 bytes
 * outside 1 <= Ci <= 4, 1 <= R, S <= 7, Co >= 1): int8 q_w - (qmin + 128) as [Ci][Cop][64], the
 * vector cwz[co] = qmin + 128 - z_w[co] and the full-window sums T[c][co].  ADDS to *bad the number
 * of channels whose zp is not an integer in [qmin-256, qmin+511] (taken as qmin), as K22 does.
 * ssq_stem_conv_u8_fwd: y as fp32 NCHW [Nb, Co, OH, OW].
 * ssq_stem_conv_u8_codes_fwd: qepi_code_y on each y, i.e. ssq_epilogue_codes_fwd's arguments,
 * checks and bytes for the fp32 form's y (NHWC int8 [Nb*OH*OW][qinfer_cpad(Co)], padded channels 0,
 * every byte written, a NaN q stored as out_qmin and ADDED to *bad) without the fp32 tensor.
 * A workgroup whose tile has every tap inside the image reads B_c from T and skips the validity
 * sums; every_tile_border != 0 makes every workgroup compute them (the same bits: an A/B and test
 * knob).  ssq_stem_u8_tiles: the workgroups of a launch of this geometry (codes: the code form's)
 * that take the interior and the border path.
 *
 * Strided views.  ssq_stem_conv_u8_strided_fwd / _strided_codes_fwd take u as any view of
 * [Nb, Ci, H, W] uint8 elements with four byte strides (sN, sC, sH, sW) >= 0: element (n, c, h, w)
 * is the byte u[n sN + c sC + h sH + w sW].  The two calls above are the strided ones at the dense
 * NCHW strides (Ci H W, H W, W, 1).  The output is the same bits whatever the strides; only how the
 * patch is staged differs, in three forms chosen on the host: planar (0; sW == 1: NCHW, planar
 * crops, batch-strided views), interleaved (1; sC == 1 and Ci <= sW <= 4: HWC pixels of 3 or 4
 * bytes, 3 channels in 4-byte pixels, crops of either, at any alignment of the base) and generic
 * (2; any other strides: correct, no speed claim).  No load touches a byte outside the view's
 * span, offsets lo = 0 .. hi = (Nb-1) sN + (Ci-1) sC + (H-1) sH + (W-1) sW from u: a padded tap
 * stands for x = 0, never for the byte next to the view, and a pixel's pad byte is not read.
 * ssq_stem_u8_view_span (host only): lo, hi and the form of a view, with the view's refusals.
 *
 * Refused with SSQ_E_ARG before any launch: a negative stride (no channel reversal), a view that
 * spans 2^31 bytes or more (hi, or a stride, >= 2^31), a null pointer, the geometry above,
 * strides < 1,
 * pad_h >= R or pad_w >= S or negative, an empty output, prepared_bytes below the blob's size, a
 * prepared pointer that is not 16-byte aligned (the kernel reads the weight rows as 16-byte
 * vectors), a tensor of 2^31 elements or more.  No allocation, no sync, no float atomics,
 * capturable.                                                                                  */
size_t ssq_stem_u8_weight_prepared_bytes(int64_t Co, int64_t Ci, int64_t R, int64_t S);
int ssq_stem_u8_weight_prepare(const void* packed, const float* zp, int64_t Co, int64_t Ci,
                               int64_t R, int64_t S, int n_bits, int qmin, void* prepared,
                               uint32_t* bad, ssq_stream_t stream);
int ssq_stem_u8_tiles(int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R,
                      int64_t S, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w,
                      int codes, int64_t* interior, int64_t* border);
int ssq_stem_conv_u8_fwd(const uint8_t* u, const void* prepared, size_t prepared_bytes,
                         const float* M, const float* s, int64_t Nb, int64_t Ci, int64_t H,
                         int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride_h,
                         int64_t stride_w, int64_t pad_h, int64_t pad_w, int every_tile_border,
                         float* y, ssq_stream_t stream);
int ssq_stem_conv_u8_codes_fwd(const uint8_t* u, const void* prepared, size_t prepared_bytes,
                               const float* M, const float* s, int64_t Nb, int64_t Ci, int64_t H,
                               int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride_h,
                               int64_t stride_w, int64_t pad_h, int64_t pad_w,
                               int every_tile_border, const float* bias, const float* gamma,
                               const float* phi, int act, float out_delta, float out_zero_point,
                               int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad,
                               ssq_stream_t stream);
int ssq_stem_u8_view_span(int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t sN, int64_t sC,
                          int64_t sH, int64_t sW, int64_t* lo, int64_t* hi, int* form);
int ssq_stem_conv_u8_strided_fwd(const uint8_t* u, const void* prepared, size_t prepared_bytes,
                                 const float* M, const float* s, int64_t Nb, int64_t Ci, int64_t H,
                                 int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride_h,
                                 int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t sN,
                                 int64_t sC, int64_t sH, int64_t sW, int every_tile_border,
                                 float* y, ssq_stream_t stream);
int ssq_stem_conv_u8_strided_codes_fwd(const uint8_t* u, const void* prepared,
                                       size_t prepared_bytes, const float* M, const float* s,
                                       int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                       int64_t R, int64_t S, int64_t stride_h, int64_t stride_w,
                                       int64_t pad_h, int64_t pad_w, int64_t sN, int64_t sC,
                                       int64_t sH, int64_t sW, int every_tile_border,
                                       const float* bias, const float* gamma, const float* phi,
                                       int act, float out_delta, float out_zero_point,
                                       int out_qmin, int out_qmax, int8_t* out_codes,
                                       uint32_t* bad, ssq_stream_t stream);

/* ---------------------------------------------------------------- column-scaled weights
 * A weight with a per-column input scale on a common integer grid,
 *     W_hat[co, j] = ((q_w - z_w[co]) * d1[co]) * c[j],  c[j] = fp32(kcol[j] / L),  j = (ci, r, s)
 * (ChannelQuantMSE; kcol[j] in 1..L, L <= 127 found by the caller), runs on the same kernels
 * with the centred integer m[co, j] = (q_w - z_w[co]) * kcol[j] as the int8 operand:
 *     I = sum_j (q_a - z_a) m[co, j] = D + az * T[co],  D = sum a_s m,  T[co] = sum_j m[co, j]
 * exact for K <= 65536 (|a_s| <= 128, |m| <= 127), and y = fp32(I) * scale[co] with the caller's
 * scale[co] = fp32(fp32(delta_a * d1[co]) / fp32(L)): one conversion, one multiply, as above.
 *
 * ssq_qweight_prepare_colscale / ssq_qweight_prepare_grouped_colscale: ssq_qweight_prepare /
 * ssq_qweight_prepare_grouped with kcol (device int32 [Ci*R*S], [Cig*R*S] shared by all groups):
 * the same byte count and layout, holding m, cwz = 0, T[co] = sum m and the 0/1 row(s) (the
 * depthwise int32 blob is the centred weight times kcol[tap]), so every reader of a prepared
 * blob (ssq_qconv_i8_*_fwd, ssq_qconv_i8_grouped_*_fwd, ssq_qlinear_pooled_fwd) runs it as it
 * stands.  *bad also receives the number of real elements with |m| > 127 (stored saturated) or
 * with kcol[j] outside [1, 127]: a blob prepared with *bad != 0 must not be used.
 *
 * ssq_qconv_i8_centred_fwd / _codes_fwd / _codes_res_fwd: ssq_qconv_i8_fwd / _codes_fwd /
 * _codes_res_fwd (same arguments, checks and results bit for bit) for a blob whose cwz is 0,
 * i.e. one of ssq_qweight_prepare_colscale: the 0/1 row and cwz are not read and the window-sum
 * MFMA is not issued (four per k step instead of five).  On any other blob the result is wrong. */
int ssq_qweight_prepare_colscale(const void* packed, const float* zp, const int32_t* kcol,
                                 int64_t Co, int64_t Ci, int64_t R, int64_t S, int n_bits,
                                 int qmin, void* prepared, uint32_t* bad, ssq_stream_t stream);
int ssq_qweight_prepare_grouped_colscale(const void* packed, const float* zp, const int32_t* kcol,
                                         int64_t Co, int64_t Cig, int64_t R, int64_t S,
                                         int64_t groups, int n_bits, int qmin, void* prepared,
                                         uint32_t* bad, ssq_stream_t stream);
int ssq_qconv_i8_centred_fwd(const int8_t* codes, const void* prepared, const float* scale,
                             int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R,
                             int64_t S, int64_t stride, int64_t pad, int64_t groups,
                             float act_zero_point, int act_qmin, int act_qmax, float* y,
                             ssq_stream_t stream);
int ssq_qconv_i8_centred_codes_fwd(const int8_t* codes, const void* prepared, const float* scale,
                                   int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                   int64_t R, int64_t S, int64_t stride, int64_t pad,
                                   int64_t groups, float act_zero_point, int act_qmin,
                                   int act_qmax, const float* bias, const float* gamma,
                                   const float* phi, int act, float out_delta,
                                   float out_zero_point, int out_qmin, int out_qmax,
                                   int8_t* out_codes, uint32_t* bad, ssq_stream_t stream);
int ssq_qconv_i8_centred_codes_res_fwd(const int8_t* codes, const void* prepared,
                                       const float* scale, int64_t Nb, int64_t Ci, int64_t H,
                                       int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride,
                                       int64_t pad, int64_t groups, float act_zero_point,
                                       int act_qmin, int act_qmax, const float* bias,
                                       const float* gamma, const float* phi, int act,
                                       float out_delta, float out_zero_point, int out_qmin,
                                       int out_qmax, int8_t* out_codes, uint32_t* bad,
                                       const float* res_f32, const int8_t* res_codes,
                                       float res_delta, float res_zero_point, int res_qmin,
                                       int res_qmax, ssq_stream_t stream);

/* ---------------------------------------------------------------- per-(co, ci) scales, the wide operand
 * A weight whose scale is per (co, ci) on a common grid (ChannelQuant's shifted scale),
 *     W_hat[co, ci, r, s] = (q_w - z_w[co]) * fp32(base[co] * fp32(kfac[co, ci] / L)),
 * runs like a column-scaled one with the centred integer m = (q_w - z_w[co]) * kfac[co, ci] as
 * the operand, T[co] = sum m and the caller's scale[co] = fp32(fp32(delta_a * base[co]) / fp32(L)).
 *
 * ssq_qweight_prepare_perci / ssq_qweight_prepare_grouped_perci: the *_colscale prepares with
 * kfac (device int32 [Co*Ci], [Co*Cig] grouped) in kcol's place: same blob, same *bad rules
 * (kfac outside [1, 127], |m| > 127).  A Linear's scale is per element (R = S = 1).  A depthwise
 * weight has no such form (SSQ_E_ARG).
 *
 * The wide blob holds a centred operand of up to |m| <= 16319 as two int8 digits,
 *     m = 128 h + l,  l = ((m + 64) mod 128) - 64 in [-64, 63],  h = (m - l) / 128 in [-127, 127]:
 * [Cop][Kp] int8 rows of h, [Cop][Kp] rows of l, the 0/1 row [Kp], cwz[Cop] = 0, T[Cop] = sum m
 * (ssq_qweight_prepared_bytes_wide bytes).  ssq_qweight_prepare_wide writes it from kfac, column
 * factors [Ci*R*S] (per_ci = 0) or per-(co, ci) factors [Co*Ci] (per_ci = 1), in [1, 16319];
 * *bad counts a factor outside that range, an |m| > 16319 and a zero point that is no code.
 *
 * ssq_qconv_i8_wide_fwd / _codes_fwd / _codes_res_fwd: the centred forms' arguments, checks and
 * epilogue on a wide blob: D_h = sum a_s h and D_l = sum a_s l are exact int32 sums (eight MFMAs per
 * k step), I = 128 D_h + D_l + az * T[co] in int64, then one conversion and one multiply (or the
 * code-emitting epilogue): a function of the codes alone, equal bit for bit to the centred form
 * wherever |m| <= 127.  Dense only, no split-K form; a blob of any other prepare gives wrong
 * results.  No allocation, no sync, capturable. */
int ssq_qweight_prepare_perci(const void* packed, const float* zp, const int32_t* kfac,
                              int64_t Co, int64_t Ci, int64_t R, int64_t S, int n_bits, int qmin,
                              void* prepared, uint32_t* bad, ssq_stream_t stream);
int ssq_qweight_prepare_grouped_perci(const void* packed, const float* zp, const int32_t* kfac,
                                      int64_t Co, int64_t Cig, int64_t R, int64_t S,
                                      int64_t groups, int n_bits, int qmin, void* prepared,
                                      uint32_t* bad, ssq_stream_t stream);
size_t ssq_qweight_prepared_bytes_wide(int64_t Co, int64_t Ci, int64_t R, int64_t S);
int ssq_qweight_prepare_wide(const void* packed, const float* zp, const int32_t* kfac, int per_ci,
                             int64_t Co, int64_t Ci, int64_t R, int64_t S, int n_bits, int qmin,
                             void* prepared, uint32_t* bad, ssq_stream_t stream);
int ssq_qconv_i8_wide_fwd(const int8_t* codes, const void* prepared, const float* scale,
                          int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R,
                          int64_t S, int64_t stride, int64_t pad, int64_t groups,
                          float act_zero_point, int act_qmin, int act_qmax, float* y,
                          ssq_stream_t stream);
int ssq_qconv_i8_wide_codes_fwd(const int8_t* codes, const void* prepared, const float* scale,
                                int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t groups,
                                float act_zero_point, int act_qmin, int act_qmax,
                                const float* bias, const float* gamma, const float* phi, int act,
                                float out_delta, float out_zero_point, int out_qmin, int out_qmax,
                                int8_t* out_codes, uint32_t* bad, ssq_stream_t stream);
int ssq_qconv_i8_wide_codes_res_fwd(const int8_t* codes, const void* prepared, const float* scale,
                                    int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                    int64_t R, int64_t S, int64_t stride, int64_t pad,
                                    int64_t groups, float act_zero_point, int act_qmin,
                                    int act_qmax, const float* bias, const float* gamma,
                                    const float* phi, int act, float out_delta,
                                    float out_zero_point, int out_qmin, int out_qmax,
                                    int8_t* out_codes, uint32_t* bad, const float* res_f32,
                                    const int8_t* res_codes, float res_delta,
                                    float res_zero_point, int res_qmin, int res_qmax,
                                    ssq_stream_t stream);

/* ---------------------------------------------------------------- K23 split along K
 * The six dense conv entry points with the k walk divided among `splits` = Z workgroups per
 * output tile, for planes whose (ceil(M/64), ceil(Co/64)) grid does not fill the device
 * (M = Nb*OH*OW).  Two kernels, no atomics: the partial kernel (grid z = Z) walks the k steps
 * [floor(z*nk/Z), floor((z+1)*nk/Z)) of the nk = Kp/64 and stores its raw int32 accumulators to
 * the caller's workspace, D[Z][Co][M] then (plain blobs only) SA[Z][M]; the finish kernel adds
 * the slices and runs the parent's epilogue functions.  The integer sum is exact and
 * associative, so every result equals the parent entry point's bit for bit, `*bad` included.
 * Every workspace element is written once by one thread before it is read: the workspace needs
 * no initialisation and holds nothing between calls.
 *
 * Each takes its parent's argument list plus (splits, ws, ws_bytes) before the stream.
 * SSQ_E_ARG before any launch: splits < 2, splits > 16, splits > nk, groups != 1, ws null or
 * ws_bytes below ssq_qconv_i8_splitk_workspace_size, and everything the parent refuses.
 * ssq_qconv_i8_splitk_workspace_size: bytes for the geometry (Cp = qinfer_cpad(Ci)); 0 when
 * the split would be refused.  No allocation, no sync, capturable. */
size_t ssq_qconv_i8_splitk_workspace_size(int64_t Nb, int64_t H, int64_t W, int64_t Co, int64_t R,
                                          int64_t S, int64_t stride, int64_t pad, int64_t Cp,
                                          int splits, int centred);
int ssq_qconv_i8_splitk_fwd(const int8_t* codes, const void* prepared, const float* scale,
                            int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co, int64_t R,
                            int64_t S, int64_t stride, int64_t pad, int64_t groups,
                            float act_zero_point, int act_qmin, int act_qmax, float* y, int splits,
                            void* ws, size_t ws_bytes, ssq_stream_t stream);
int ssq_qconv_i8_centred_splitk_fwd(const int8_t* codes, const void* prepared, const float* scale,
                                    int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                    int64_t R, int64_t S, int64_t stride, int64_t pad,
                                    int64_t groups, float act_zero_point, int act_qmin,
                                    int act_qmax, float* y, int splits, void* ws, size_t ws_bytes,
                                    ssq_stream_t stream);
int ssq_qconv_i8_splitk_codes_fwd(const int8_t* codes, const void* prepared, const float* scale,
                                  int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                  int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t groups,
                                  float act_zero_point, int act_qmin, int act_qmax,
                                  const float* bias, const float* gamma, const float* phi, int act,
                                  float out_delta, float out_zero_point, int out_qmin, int out_qmax,
                                  int8_t* out_codes, uint32_t* bad, int splits, void* ws,
                                  size_t ws_bytes, ssq_stream_t stream);
int ssq_qconv_i8_centred_splitk_codes_fwd(const int8_t* codes, const void* prepared,
                                          const float* scale, int64_t Nb, int64_t Ci, int64_t H,
                                          int64_t W, int64_t Co, int64_t R, int64_t S,
                                          int64_t stride, int64_t pad, int64_t groups,
                                          float act_zero_point, int act_qmin, int act_qmax,
                                          const float* bias, const float* gamma, const float* phi,
                                          int act, float out_delta, float out_zero_point,
                                          int out_qmin, int out_qmax, int8_t* out_codes,
                                          uint32_t* bad, int splits, void* ws, size_t ws_bytes,
                                          ssq_stream_t stream);
int ssq_qconv_i8_splitk_codes_res_fwd(const int8_t* codes, const void* prepared, const float* scale,
                                      int64_t Nb, int64_t Ci, int64_t H, int64_t W, int64_t Co,
                                      int64_t R, int64_t S, int64_t stride, int64_t pad,
                                      int64_t groups, float act_zero_point, int act_qmin,
                                      int act_qmax, const float* bias, const float* gamma,
                                      const float* phi, int act, float out_delta,
                                      float out_zero_point, int out_qmin, int out_qmax,
                                      int8_t* out_codes, uint32_t* bad, const float* res_f32,
                                      const int8_t* res_codes, float res_delta,
                                      float res_zero_point, int res_qmin, int res_qmax, int splits,
                                      void* ws, size_t ws_bytes, ssq_stream_t stream);
int ssq_qconv_i8_centred_splitk_codes_res_fwd(
    const int8_t* codes, const void* prepared, const float* scale, int64_t Nb, int64_t Ci,
    int64_t H, int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
    int64_t groups, float act_zero_point, int act_qmin, int act_qmax, const float* bias,
    const float* gamma, const float* phi, int act, float out_delta, float out_zero_point,
    int out_qmin, int out_qmax, int8_t* out_codes, uint32_t* bad, const float* res_f32,
    const int8_t* res_codes, float res_delta, float res_zero_point, int res_qmin, int res_qmax,
    int splits, void* ws, size_t ws_bytes, ssq_stream_t stream);

/* ---------------------------------------------------------------- pooling head on codes (K29, K30)
 * The global average pool and the fc behind it on stored codes, with a numerics contract of
 * their own (the fc has no input quantizer, so the pooled value is never re-quantized):
 *     P[n,c]  = sum_hw (q_a - z_a)                     exact integer
 *     I[n,co] = sum_c P[n,c] (q_w[co,c] - z_w[co])     exact integer (int64)
 *     y[n,co] = fp32(I) * scale_h[co]                  one conversion (RNE), one multiply
 * scale_h[co] = fp32(fp32(delta_a * d1[co]) / fp32(HW)) is the caller's.  No bias, no FMA.  y is a
 * function of the codes alone and reproducible bit for bit from a host int64 restatement; it is
 * NOT bit-equal to an fp32 mean followed by an fp32 GEMM.
 *
 * ssq_avgpool_i8_digits_fwd (K29): codes NHWC [Nb, H, W, qinfer_cpad(C)] (ssq_act_encode's
 * stored form a_s) -> the plane sums P_s[n,c] = sum_hw a_s as two int8 digits
 * hi = (P_s + 64) >> 7, lo = P_s - 128 * hi in [-64, 63], each [Nb][qinfer_cpad(C)] with padded
 * channels 0, and sp[n] = sum_c P_s[n,c] (int32).  H * W <= 126 (|hi| <= 126), C <= 65536.
 *
 * ssq_qlinear_pooled_fwd (K30): y [Nb, Co] fp32 from K29's hi, lo, sp and the fc's prepared
 * weight (ssq_qweight_prepare's blob for (Co, Ci, 1, 1), unchanged): D = 128 * D_hi + D_lo on
 * v_mfma_i32_16x16x64_i8, I = D + cwz[co] * sp[n] + HW * az * T[co] in int64.  HW is the pooled
 * plane's H * W (1..126), (act_zero_point, act_qmin, act_qmax) the pooled codes' quantizer.
 *
 * Every refusal (null pointer, bad geometry or quantizer, H * W > 126, C > 65536, a tensor of
 * 2^31 bytes or more) is SSQ_E_ARG before any launch.  No allocation, no sync, capturable.
 * ssq_qlinear_pooled_set_tile: measurement plumbing only, K30's image tile (16, the default, or
 * 64); returns the previous value, any other argument only queries.                           */
int ssq_avgpool_i8_digits_fwd(const int8_t* codes, int64_t Nb, int64_t C, int64_t H, int64_t W,
                              int8_t* hi, int8_t* lo, int32_t* sp, ssq_stream_t stream);
int ssq_qlinear_pooled_fwd(const int8_t* hi, const int8_t* lo, const int32_t* sp,
                           const void* prepared, const float* scale_h, int64_t Nb, int64_t Ci,
                           int64_t Co, int64_t HW, float act_zero_point, int act_qmin,
                           int act_qmax, float* y, ssq_stream_t stream);
int ssq_qlinear_pooled_set_tile(int tile);

/* ---------------------------------------------------------------- the wide operand on grouped convs and the pooled fc
 * The wide operand (m = 128 h + l, |m| <= 16319, factors in [1, 16319]; see above) for the
 * kernels that read one int8 digit otherwise: K26, K25 and K30.
 *
 * ssq_qweight_prepare_grouped_wide writes ssq_qweight_prepared_bytes_grouped_wide bytes from
 * kfac, column factors [Cig*R*S] (per_ci = 0) or per-(co, ci) factors [Co*Cig] (per_ci = 1):
 *   grouped (ssq_qconv_grouped_kind 2): the grouped blob with two digit planes, h rows
 *     [G*Cogp][Kp], then l rows G*Cogp*Kp bytes behind, the 0/1 rows [G][Kp] (written, not
 *     read), cwz[Co] = 0, T[Co] = sum m;
 *   depthwise (kind 1): the int32 blob [R*S][Cp] holding m itself; per_ci = 0 only (a depthwise
 *     row has no per-(co, ci) form: SSQ_E_ARG).
 * *bad counts a factor outside [1, 16319], an |m| > 16319 and a zero point that is no code.
 *
 * ssq_qconv_i8_grouped_wide_fwd / _codes_fwd: ssq_qconv_i8_grouped_fwd / _codes_fwd's arguments,
 * checks and epilogues on that blob.  Grouped: D_h = sum a_s h and D_l = sum a_s l are exact
 * int32 sums (2 MFMAs per 16-row fragment and k step, no 0/1 row, no SA product),
 * I = 128 D_h + D_l + az * T[co] in int64, K = Cig*R*S <= 65536; equal bit for bit to the grouped
 * form on the centred int8 blob wherever |m| <= 127.  Depthwise: the int32 accumulator is exact
 * (|I| <= 49 * 255 * 16319 < 2^31), but |I| may pass 2^24, so the one int -> fp32 conversion rounds
 * to nearest even there, as K23's.
 *
 * ssq_qlinear_pooled_wide_fwd: ssq_qlinear_pooled_fwd's arguments and checks with `prepared` a
 * blob of ssq_qweight_prepare_wide for (Co, Ci, 1, 1):
 *     I = 128^2 D_hh + 128 (D_hl + D_lh) + D_ll + HW * az * T[co]   (activation digit first)
 * in int64, four int8-MFMA products per fragment; sp is not read (cwz = 0) but must be valid.  The
 * caller's scale_h[co] = fp32(fp32(delta_a * base[co]) / fp32(L * HW)); L * HW <= 129 024 is
 * exact in fp32.  A scaled fc whose m fits int8 needs none of this: its centred blob
 * (ssq_qweight_prepare_colscale / _perci) runs through ssq_qlinear_pooled_fwd as it stands.
 *
 * A blob of any other prepare gives wrong results.  Every refusal is SSQ_E_ARG before any
 * launch.  No allocation, no sync, capturable. */
size_t ssq_qweight_prepared_bytes_grouped_wide(int64_t Co, int64_t Cig, int64_t R, int64_t S,
                                               int64_t groups);
int ssq_qweight_prepare_grouped_wide(const void* packed, const float* zp, const int32_t* kfac,
                                     int per_ci, int64_t Co, int64_t Cig, int64_t R, int64_t S,
                                     int64_t groups, int n_bits, int qmin, void* prepared,
                                     uint32_t* bad, ssq_stream_t stream);
int ssq_qconv_i8_grouped_wide_fwd(const int8_t* codes, const void* prepared, const float* scale,
                                  int64_t Nb, int64_t C, int64_t H, int64_t W, int64_t Co,
                                  int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t groups,
                                  float act_zero_point, int act_qmin, int act_qmax, float* y,
                                  ssq_stream_t stream);
int ssq_qconv_i8_grouped_wide_codes_fwd(const int8_t* codes, const void* prepared,
                                        const float* scale, int64_t Nb, int64_t C, int64_t H,
                                        int64_t W, int64_t Co, int64_t R, int64_t S, int64_t stride,
                                        int64_t pad, int64_t groups, float act_zero_point,
                                        int act_qmin, int act_qmax, const float* bias,
                                        const float* gamma, const float* phi, int act,
                                        float out_delta, float out_zero_point, int out_qmin,
                                        int out_qmax, int8_t* out_codes, uint32_t* bad,
                                        ssq_stream_t stream);
int ssq_qlinear_pooled_wide_fwd(const int8_t* hi, const int8_t* lo, const int32_t* sp,
                                const void* prepared, const float* scale_h, int64_t Nb, int64_t Ci,
                                int64_t Co, int64_t HW, float act_zero_point, int act_qmin,
                                int act_qmax, float* y, ssq_stream_t stream);

/* ---------------------------------------------------------------- K33 shifted-scale activations
 * ChannelQuantAct 'shiftFeature' (the evident intent of channelQuantAct.py:69-134, whose
 * own code never ran; contract in DESIGN.md section 6).  x is (N, C, HW) in NCHW order
 * ((N, C): HW = 1); delta / zp are the replaced per-tensor quantizer's device scalars;
 * shifts is a HOST array of S <= 4 scale multipliers; p / dp / mse are (C, S).
 * Candidate i is the 'none'-mode q/dq at d_i = fp32(delta * shifts[i]), the arithmetic of
 * ssq_fq_round_fwd with qmin = 0:
 *   v_i = rint(x / d_i) + zp;  Q_i = (clamp(v_i, 0, qmax) - zp) * d_i;  in_i = [0 <= v_i <= qmax]
 * fwd   soft: y = Q_0*p[c,0]; y = y + Q_i*p[c,i], i = 1..S-1 (each product and each sum
 *             rounded in fp32, no fma);   hard: y = Q_k, k = first argmax of p[c,:]
 * bwd   soft: dx = g * m, m = +0 + p[c,0]*in_0 + ... in i order (separate fp32 products
 *             and sums); dp[c,i] = sum over (n, hw) of g*Q_i
 *       hard: dx = g * in_k; dp = 0 (dp may be NULL: the zeros are then not written)
 * init  mse[c,i] = sum over (n, hw) of (x - Q_i)^2  (ChannelQuant.init_alpha's errors)
 * The channel sums are exact products accumulated in double in a fixed order (per-plane
 * partials in `ws`, then summed over n ascending): no atomics, the same bits on every run.
 * Refused with SSQ_E_ARG before any launch: S outside 1..4, a null pointer, N*C*HW >= 2^31,
 * qmax < 1; SSQ_E_WS for a workspace smaller than its *_workspace_size (8-B aligned; the
 * forward needs none).  No allocation, no sync, capturable. */
size_t ssq_actshift_fwd_workspace_size(int64_t N, int64_t C, int64_t HW, int S);
int ssq_actshift_fwd(const float* x, const float* p, const float* delta, const float* zp,
                     const float* shifts, int S, int64_t N, int64_t C, int64_t HW, int qmax,
                     int hard, float* y, void* ws, size_t ws_bytes, ssq_stream_t stream);
size_t ssq_actshift_bwd_workspace_size(int64_t N, int64_t C, int64_t HW, int S);
int ssq_actshift_bwd(const float* x, const float* g, const float* p, const float* delta,
                     const float* zp, const float* shifts, int S, int64_t N, int64_t C,
                     int64_t HW, int qmax, int hard, float* dx, float* dp, void* ws,
                     size_t ws_bytes, ssq_stream_t stream);
size_t ssq_actshift_init_workspace_size(int64_t N, int64_t C, int64_t HW, int S);
int ssq_actshift_init(const float* x, const float* delta, const float* zp, const float* shifts,
                      int S, int64_t N, int64_t C, int64_t HW, int qmax, float* mse, void* ws,
                      size_t ws_bytes, ssq_stream_t stream);

/* ---------------------------------------------------------------- bandwidth probe
 * float4 device copy, used by bench.py to report the measured stream bandwidth.      */
int ssq_stream_copy(const float* src, float* dst, int64_t n, ssq_stream_t stream);
/* HBM read-only (kind 1: nt loads of src, dst receives nothing) / write-only (kind 2: nt
 * stores into dst) probe over n floats, K1's geometry.  Bench context only. */
int ssq_stream_probe(const float* src, float* dst, int64_t n, int kind, ssq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SSQ_H_ */
