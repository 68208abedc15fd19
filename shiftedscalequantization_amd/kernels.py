"""Tensor-level wrappers and autograd Functions over libssq.so.

Each function states the reference op sequence it replaces.  All of them require fp32
tensors on the HIP device; nothing here falls back to eager PyTorch arithmetic.
Weight geometry: W is (Co, Ci, kh, kw) -> (Co, Ci, K=kh*kw), Linear (Co, Ci) -> K = 1.
"""
import collections
import ctypes as C
import functools
import os

import torch

from . import _capi as A
from ._capi import call, fptr, query, stream_of, workspace
from .nets import GlobalMeanPool


def qrange(n_bits, sym):
    n = 2 ** n_bits
    return (-(n // 2), n // 2 - 1) if sym else (0, n - 1)


def geometry(w):
    if w.dim() == 4:
        return int(w.shape[0]), int(w.shape[1]), int(w.shape[2] * w.shape[3]), 0
    if w.dim() == 2:
        return int(w.shape[0]), int(w.shape[1]), 1, 1
    raise ValueError(f"weight must be 2-D (Linear) or 4-D (Conv2d), got {tuple(w.shape)}")


def _codes_buf(x, want):
    return torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want else None


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ K1/K2
def _channel_layout(x, delta):
    """(inner, nch) for ssq_fq_fwd: delta broadcasts over x as x.shape[:k] + (1,)*rest,
    channel c of element i = (i // inner) % nch."""
    nd = delta.numel()
    if nd == 1:
        return 1, 1
    ds = tuple(delta.shape) + (1,) * (x.dim() - delta.dim())
    for k in range(1, x.dim() + 1):
        if ds[:k] == tuple(x.shape[:k]) and all(d == 1 for d in ds[k:]):
            return x.numel() // nd, nd
    raise ValueError(f"unsupported delta shape {tuple(delta.shape)} for x {tuple(x.shape)}")


def _zp_like(zp, delta):
    """Expand a per-row zero point to delta's per-(row, in-channel) layout if needed."""
    if zp.numel() == delta.numel() or zp.numel() == 1 and delta.numel() == 1:
        return zp
    return zp.expand(delta.shape).contiguous() if zp.dim() == delta.dim() else \
        zp.reshape(zp.shape + (1,) * (delta.dim() - zp.dim())).expand(delta.shape).contiguous()


def fake_quant_fwd(x, delta, zp, n_bits, sym=False, scale=1.0, codes=False, out=None,
                   ste=True):
    """UniformAffineQuantizer.forward (quant_layer.py:92-98). Returns (y, codes|None);
    `out` (same shape, fp32, on the device) receives y when given.  ste=True rounds as the
    reference's round_ste ((round(t) - t) + t: NaN at t = +-inf), ste=False as plain
    torch.round (ChannelQuant / ChannelQuantAct 'none', AdaRound 'nearest')."""
    x, xp = fptr(x, "x")
    delta, dp = fptr(delta.detach(), "delta")
    zp, zpp = fptr(_zp_like(zp.detach(), delta), "zero_point")
    inner, nch = _channel_layout(x, delta)
    lo, hi = qrange(n_bits, sym)
    if out is not None:
        y, _ = fptr(out, "out")
        if y.shape != x.shape or y is not out:
            raise A.SSQError("fake_quant_fwd: out must be a contiguous tensor shaped like x")
    else:
        y = torch.empty_like(x)
    cb = _codes_buf(x, codes)
    call("ssq_fq_fwd" if ste else "ssq_fq_round_fwd", xp, _vp(y), _vp(cb), dp, zpp, x.numel(),
         inner, nch, float(scale), lo, hi, stream_of(x))
    return y, cb


class FakeQuantFn(torch.autograd.Function):
    """round_ste fake-quant with the reference's autograd: STE for x, exact chain for
    delta / zero_point (used by the act-delta LSQ recon, block_recon.py:62-73)."""

    @staticmethod
    def forward(ctx, x, delta, zp, n_bits, sym):
        y, _ = fake_quant_fwd(x, delta, zp, n_bits, sym)
        ctx.save_for_backward(x, delta, zp)
        ctx.q = (n_bits, sym)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, delta, zp = ctx.saved_tensors
        n_bits, sym = ctx.q
        x = x.contiguous()
        gy = gy.contiguous()
        d, z = delta.detach().contiguous(), zp.detach().contiguous()
        inner, nch = _channel_layout(x, d)
        lo, hi = qrange(n_bits, sym)
        need_x, need_d, need_z = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gx = torch.empty_like(x) if need_x else None
        gd = torch.empty(d.numel(), dtype=torch.float32, device=x.device) if need_d else None
        gz = torch.empty(z.numel(), dtype=torch.float32, device=x.device) if need_z else None
        wsb = query("ssq_fq_bwd_workspace_size", x.numel(), inner, nch)
        ws, wsn = workspace(wsb, x.device)
        call("ssq_fq_bwd", _vp(x), _vp(gy), _vp(d), _vp(z), x.numel(), inner, nch, lo, hi,
             _vp(gx), _vp(gd), _vp(gz), ws, wsn, stream_of(x))
        return (gx, None if gd is None else gd.view(delta.shape),
                None if gz is None else gz.view(zp.shape), None, None)


def fake_quant(x, delta, zp, n_bits, sym=False):
    return FakeQuantFn.apply(x, delta, zp, n_bits, sym)


class RoundQuantFn(torch.autograd.Function):
    """q/dq with torch.round (NO straight-through estimator) at delta*scale, clamp
    [lo, hi]: ChannelQuantAct 'none' mode (channelQuantAct.py:56-67).  The reference's
    autograd gives d/dx = 0 (round has a zero gradient), d/ddelta = scale * sum g*(q-zp)
    (through the product delta*shiftedScale), d/dzp = -sum_{clamped} g*delta*scale."""

    @staticmethod
    def forward(ctx, x, delta, zp, n_bits, sym, scale):
        y, _ = fake_quant_fwd(x, delta, zp, n_bits, sym, scale=scale, ste=False)
        ctx.save_for_backward(x, delta, zp)
        ctx.q = (n_bits, sym, scale)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, delta, zp = ctx.saved_tensors
        n_bits, sym, scale = ctx.q
        need_x, need_d, need_z = ctx.needs_input_grad[:3]
        gx = torch.zeros_like(x) if need_x else None
        if not (need_d or need_z):
            return gx, None, None, None, None, None
        x, gy = x.contiguous(), gy.contiguous()
        # the product delta*shiftedScale as the reference forms it (tensor * python float)
        t = (delta.detach() * scale).contiguous()
        z = _zp_like(zp.detach(), t).contiguous()
        inner, nch = _channel_layout(x, t)
        lo, hi = qrange(n_bits, sym)
        gt = torch.empty(t.numel(), dtype=torch.float32, device=x.device)
        gz = torch.empty(z.numel(), dtype=torch.float32, device=x.device) if need_z else None
        wsb = query("ssq_fq_bwd_workspace_size", x.numel(), inner, nch)
        ws, wsn = workspace(wsb, x.device)
        call("ssq_fq_round_bwd", _vp(x), _vp(gy), _vp(t), _vp(z), x.numel(), inner, nch, lo, hi,
             _vp(gt), _vp(gz), ws, wsn, stream_of(x))
        gd = (gt * scale).view(delta.shape) if need_d else None
        return (gx, gd, None if gz is None else gz.view(zp.shape), None, None, None)


def round_quant(x, delta, zp, n_bits, sym=False, scale=1.0):
    return RoundQuantFn.apply(x, delta, zp, n_bits, sym, float(scale))


class FqMultiPlan:
    """fake_quant_multi's arguments checked and packed once: calling the plan launches the
    same table again (one ctypes call), e.g. a fixed model's weights quantised every step.
    The plan holds its tensors and reads their current values at each launch, so in-place
    updates of x / delta / zero_point are seen; it therefore refuses non-contiguous inputs
    (a contiguous copy would freeze their values at plan time).  A tensor replaced by a new
    one needs a new plan.  fake_quant_multi (one launch) copies non-contiguous inputs."""

    def __init__(self, xs, deltas, zps, n_bits, sym=False, out=None, _once=False):
        n = len(xs)
        if not _once:
            for k, (x, d, z) in enumerate(zip(xs, deltas, zps)):
                for t, what in ((x, "x"), (d, "delta"), (z, "zero_point")):
                    if not t.is_contiguous():
                        raise ValueError(f"FqMultiPlan: {what}[{k}] is not contiguous (a copy "
                                         "would not see later in-place updates)")
        if out is None:
            ys = [torch.empty_like(x) for x in xs]
        else:
            if len(out) != n:
                raise ValueError(f"fake_quant_multi: {len(out)} outputs for {n} inputs")
            for k, (x, y) in enumerate(zip(xs, out)):
                A.check(y, f"out[{k}]")
                if y.shape != x.shape or not y.is_contiguous():
                    raise ValueError(f"fake_quant_multi: out[{k}] must be contiguous, shape "
                                     f"{tuple(x.shape)}")
            ys = list(out)
        keep = []
        P = C.c_void_p * n
        xa, ya, da, za = P(), P(), P(), P()
        na, ia, ca = (C.c_int64 * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
        lo_a, hi_a = (C.c_int * n)(), (C.c_int * n)()
        nb = n_bits if isinstance(n_bits, (list, tuple)) else [n_bits] * n
        for k, (x, d, z, y) in enumerate(zip(xs, deltas, zps, ys)):
            x, xp = fptr(x)
            d, dp = fptr(d.detach())
            z, zpp = fptr(z.detach())
            keep += [x, d, z]
            inner, nch = _channel_layout(x, d)
            xa[k], ya[k], da[k], za[k] = xp.value, y.data_ptr(), dp.value, zpp.value
            na[k], ia[k], ca[k] = x.numel(), inner, nch
            lo_a[k], hi_a[k] = qrange(nb[k], sym)
        self.ys, self.keep = ys, keep
        self.args = (n, xa, ya, da, za, na, ia, ca, lo_a, hi_a)
        self.device = xs[0].device

    def __call__(self):
        call("ssq_fq_fwd_multi", *self.args, stream_of(self.ys[0]))
        if _DEFERRED_FQ_KEEP is not None:
            # the table may launch later (riding on the next per-tensor launch): keep any
            # contiguous copies made for it alive until then
            _DEFERRED_FQ_KEEP.append(self)
        return self.ys


def fake_quant_multi(xs, deltas, zps, n_bits, sym=False, out=None):
    """Every tensor of a list in one launch (per-channel params staged in LDS); out: a
    list of contiguous fp32 outputs, one per input and of its shape (else allocated).
    FqMultiPlan packs the same arguments once for repeated launches."""
    return FqMultiPlan(xs, deltas, zps, n_bits, sym, out, _once=True)()


_DEFERRED_FQ_KEEP = None


def maxpool2d(x, k, stride, padding):
    """F.max_pool2d forward (no dilation, floor mode) on ssq_maxpool2d_fwd: bit-identical to
    torch's, NCHW fp32 on the device, K <= 7, padding <= K // 2."""
    x, xp = fptr(x, "x")
    N, C_, H, W = (int(v) for v in x.shape)
    OH, OW = (H + 2 * padding - k) // stride + 1, (W + 2 * padding - k) // stride + 1
    y = torch.empty((N, C_, OH, OW), dtype=torch.float32, device=x.device)
    call("ssq_maxpool2d_fwd", xp, _vp(y), N, C_, H, W, int(k), int(stride), int(padding),
         stream_of(x))
    return y


# QuantModel swaps nn.MaxPool2d for SsqMaxPool2d (A/B knob: SSQ_MAXPOOL=0 keeps torch's)
MAXPOOL_HIP = os.environ.get("SSQ_MAXPOOL", "1") != "0"


class SsqMaxPool2d(torch.nn.MaxPool2d):
    """nn.MaxPool2d whose forward runs on ssq_maxpool2d_fwd where it applies (a square
    window of <= 7, padding <= K // 2, no dilation / ceil mode / indices, a 4-D fp32 device
    input that needs no gradient); torch's pooling otherwise.  Same results either way.
    A carried int8 code tensor (`carried`) is pooled as codes (ssq_maxpool_i8_fwd) while the
    integer plan's edge marks this pool and is live, and decoded to the fp32 tensor it stands for
    otherwise."""

    @staticmethod
    def wrap(m):
        s = SsqMaxPool2d(m.kernel_size, m.stride, m.padding, m.dilation, m.return_indices,
                         m.ceil_mode)
        return s

    def _plan(self):
        def one(v):
            if isinstance(v, int):
                return v
            return v[0] if len(set(v)) == 1 else None
        k, st, pad, dil = (one(v) for v in (self.kernel_size, self.stride, self.padding,
                                            self.dilation))
        if None in (k, st, pad, dil) or dil != 1 or self.ceil_mode or self.return_indices:
            return None
        if k > 7 or 2 * pad > k:
            return None
        return k, st, pad

    _int_stem = None    # the StemEdge that marks a planned pool (quant/integer.py, carry_stem)

    def forward(self, x):
        plan = self._plan()
        cc = getattr(x, "_ssq_codes", None)
        if cc is not None:
            # a carried code tensor: pooled as codes (K28) by a planned pool, decoded otherwise
            stem = self._int_stem
            if stem is not None and plan is not None and stem.live():
                out = maxpool_codes(x, *plan)
                stem.pooled[self] += 1
                N, OH, OW, _ = (int(v) for v in out.shape)
                return carried(out, (N, cc.shape[1], OH, OW), *cc.quantizer())
            x = materialize_epi(x)
        if (plan is not None and x.dim() == 4 and x.is_cuda and x.dtype == torch.float32
                and not (torch.is_grad_enabled() and x.requires_grad)):
            return maxpool2d(x, *plan)
        return super().forward(x)


class SsqGlobalAvgPool(torch.nn.AdaptiveAvgPool2d):
    """The global average pool in front of the fc -- nn.AdaptiveAvgPool2d with output size 1
    ((N, C, 1, 1)), or with `flat` a GlobalMeanPool ((N, C)) -- whose forward is the wrapped
    module's on any untagged input.  A carried int8 code tensor (`carried`) is pooled as codes
    (ssq_avgpool_i8_digits_fwd, leaving as `pooled` digits for the planned fc) while the
    integer plan's edge marks this pool and is live, and decoded to the fp32 tensor it stands
    for otherwise."""

    @staticmethod
    def wraps(m):
        if isinstance(m, GlobalMeanPool):
            return True
        return type(m) is torch.nn.AdaptiveAvgPool2d and m.output_size in (1, (1, 1))

    @staticmethod
    def wrap(m):
        s = SsqGlobalAvgPool(1)
        s.flat = isinstance(m, GlobalMeanPool)
        return s

    flat = False
    _int_head = None    # the HeadEdge that marks a planned pool (quant/integer.py, carry_head)

    def forward(self, x):
        cc = getattr(x, "_ssq_codes", None)
        if cc is not None:
            head = self._int_head
            if (head is not None and x.dim() == 4 and x.shape[1] * x.shape[2] <= HEAD_MAX_HW
                    and head.live()):
                hi, lo, sp = avgpool_codes(x)
                head.pooled[self] += 1
                return pooled(hi, lo, sp, (cc.shape[0], cc.shape[1]),
                              int(x.shape[1] * x.shape[2]), *cc.quantizer())
            x = materialize_epi(x)
        return x.mean([2, 3]) if self.flat else super().forward(x)


class deferred_fq_multi:
    """Context: a fake_quant_multi inside it rides on the next per-tensor fake_quant_fwd of
    its stream -- one launch for both (include/ssq.h ssq_set_deferred_fq_multi); a table
    still queued at exit is launched then."""

    def __init__(self, on=True, device=None):
        self.on, self.device = on, device

    def __enter__(self):
        global _DEFERRED_FQ_KEEP
        self.prev = bool(query("ssq_set_deferred_fq_multi", 1)) if self.on else None
        if self.on:
            self.prev_keep, _DEFERRED_FQ_KEEP = _DEFERRED_FQ_KEEP, []
        return self

    def __exit__(self, *exc):
        global _DEFERRED_FQ_KEEP
        if self.on:
            dev_ = torch.device("cuda", torch.cuda.current_device()) if self.device is None \
                else self.device
            try:
                call("ssq_flush_fq_multi", C.c_void_p(torch.cuda.current_stream(dev_).cuda_stream))
            finally:
                query("ssq_set_deferred_fq_multi", int(self.prev))
                # every queued table has launched: its inputs may be freed (stream order)
                _DEFERRED_FQ_KEEP = self.prev_keep


# ------------------------------------------------------------------ K3/K4
class ScaleInitError(A.SSQError, ValueError):
    """A row the reference's init_quantization_scale cannot initialise."""


def scale_init(x, n_bits, sym=False, channel_wise=False, method="max", return_scores=False,
               check=True):
    """init_quantization_scale (quant_layer.py:100-166) on the device.
    Returns (delta, zero_point, raw_zero_point) shaped like the reference's:
    (Co,1,1,1)/(Co,1) for channel_wise, 0-dim otherwise.

    A row holding NaN (or, for 'max', -inf; for 'mse', any infinity or a constant row) has no
    init in the reference: 'max' raises ValueError at round(nan) (:140), 'mse' never assigns
    delta (:147-162) and fails where it is used.  ssq_scale_init marks such rows NaN and this
    raises ScaleInitError (an SSQError and a ValueError) naming them -- one host sync, as the
    reference's own .item() calls; check=False skips it (the caller inspects the NaN rows)."""
    x, xp = fptr(x.detach(), "x")
    if "max" in method:
        m, sflag = 0, int("scale" in method)
    elif method == "mse":
        m, sflag = 1, 0
    else:
        raise NotImplementedError(method)
    rows = x.shape[0] if channel_wise else 1
    inner = x.numel() // rows
    d = torch.empty(rows, dtype=torch.float32, device=x.device)
    z = torch.empty_like(d)
    r = torch.empty_like(d)
    sc = torch.empty(rows, 80, dtype=torch.float64, device=x.device) if (return_scores and m == 1) else None
    wsb = query("ssq_scale_init_workspace_size", rows, inner, m)
    ws, wsn = workspace(wsb, x.device)
    call("ssq_scale_init", xp, rows, inner, n_bits, int(sym), m, sflag, _vp(d), _vp(z), _vp(r),
         _vp(sc), ws, wsn, stream_of(x))
    if check:
        bad = torch.isnan(d) | torch.isnan(z)
        if bool(bad.any()):
            rows_bad = bad.nonzero().flatten()[:8].tolist()
            raise ScaleInitError(f"ssq_scale_init ({method}): {int(bad.sum())} of {rows} rows have "
                                 f"no quantization scale (NaN / infinite input; rows {rows_bad}...), "
                                 f"as the reference's init_quantization_scale raises there")
    if channel_wise:
        shape = (-1,) + (1,) * (x.dim() - 1)
        out = d.view(shape), z.view(shape), r.view(shape)
    else:
        out = d.view(()), z.view(()), r.view(())
    return out + (sc,) if return_scores else out


# ------------------------------------------------------------------ K9 inits
def shift_init(w, delta, shifts, zp=None, n_bits=None, sym=False, mode=0):
    """ChannelQuant.init_v_beta (mode 0, channelQuant.py:279-294) -> (alpha, beta, mse) or
    init_v's alpha (mode 1, channelQuant.py:201-213; beta is None)."""
    w, wp = fptr(w.detach(), "weight")
    delta, dp = fptr(delta.detach(), "delta")
    z, zpp = fptr(zp.detach(), "zero_point") if zp is not None else (None, None)
    Co, Ci, K, is_fc = geometry(w)
    S = len(shifts)
    lo, hi = qrange(n_bits, sym) if mode == 1 else (0, 1)
    alpha = torch.empty((Co, Ci, S) if is_fc else (Ci, S), dtype=torch.float32, device=w.device)
    mse = torch.empty_like(alpha)
    beta = torch.empty_like(w) if mode == 0 else None
    wsb = query("ssq_shift_init_workspace_size", Co, Ci, K, S, is_fc)
    ws, wsn = workspace(wsb, w.device)
    call("ssq_shift_init", wp, dp, zpp, A.shifts_arg(shifts), S, Co, Ci, K, is_fc, int(mode), lo, hi,
         _vp(alpha), _vp(beta), _vp(mse), ws, wsn, stream_of(w))
    return alpha, beta, mse


def rect_init(w, delta):
    """beta = -log((zeta-gamma)/(rest-gamma) - 1) (channelQuant.py:300-307,
    adaptive_rounding.py:72-78); delta per output row or per (row, in-channel)."""
    w, wp = fptr(w.detach(), "weight")
    delta, dp = fptr(delta.detach(), "delta")
    Co, Ci, K, _ = geometry(w)
    per_ci = _delta_per_ci(delta, Co, Ci)
    beta = torch.empty_like(w)
    call("ssq_rect_init", wp, dp, per_ci, Co, Ci, K, _vp(beta), stream_of(w))
    return beta


def _delta_per_ci(delta, Co, Ci):
    if delta.numel() == Co:
        return 0
    if delta.numel() == Co * Ci:
        return 1
    raise ValueError(f"delta with {delta.numel()} entries for ({Co},{Ci}) weight")


def get_delta(delta, alpha, shifts, w_shape):
    """ChannelQuant.get_delta (channelQuant.py:221-237) -> (Co,Ci,1,1) conv / (Co,Ci) fc."""
    delta, dp = fptr(delta.detach(), "delta")
    alpha, ap = fptr(alpha.detach(), "alpha")
    Co, Ci = int(w_shape[0]), int(w_shape[1])
    is_fc = int(len(w_shape) == 2)
    out = torch.empty(Co, Ci, dtype=torch.float32, device=delta.device)
    call("ssq_get_delta", dp, ap, A.shifts_arg(shifts), len(shifts), Co, Ci, is_fc, _vp(out),
         stream_of(delta))
    return out if is_fc else out.view(Co, Ci, 1, 1)


# ------------------------------------------------------------------ K5/K6 adaShift
class AdaShiftFn(torch.autograd.Function):
    """ChannelQuant.forward 'adaShift' (channelQuant.py:51-64).  Gradients flow to alpha
    (soft targets only) and beta (soft rounding only), as in the reference's autograd.
    `reg` = (lambda, b, reg_vals, reg_dev) optionally fuses the shift regulariser: its
    gradient is added to alpha's inside the same backward kernel, (lambda, b) taken from
    the device pair reg_dev when given (graph-capturable)."""

    @staticmethod
    def forward(ctx, alpha, beta, w, delta, zp, shifts, n_bits, sym, hard_t, hard_r, reg):
        w, wp = fptr(w.detach(), "weight")
        a, ap = fptr(alpha.detach(), "alpha")
        b, bp = fptr(beta.detach(), "beta")
        d, dp = fptr(delta.detach(), "delta")
        z, zpp = fptr(zp.detach(), "zero_point")
        Co, Ci, K, is_fc = geometry(w)
        lo, hi = qrange(n_bits, sym)
        out = torch.empty_like(w)
        call("ssq_adashift_fwd", wp, ap, bp, dp, zpp, A.shifts_arg(shifts), len(shifts), Co, Ci, K,
             is_fc, int(hard_t), int(hard_r), lo, hi, _vp(out), None, stream_of(w))
        ctx.save_for_backward(a, b, w, d, z)
        ctx.cfg = (tuple(shifts), n_bits, sym, hard_t, hard_r, reg)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, w, d, z = ctx.saved_tensors
        shifts, n_bits, sym, hard_t, hard_r, reg = ctx.cfg
        need_a = ctx.needs_input_grad[0] and not hard_t
        need_b = ctx.needs_input_grad[1] and not hard_r
        if not (need_a or need_b):
            return (None,) * 11
        g = g.contiguous()
        Co, Ci, K, is_fc = geometry(w)
        lo, hi = qrange(n_bits, sym)
        ga = torch.empty_like(a)
        gb = torch.empty_like(w) if need_b else None
        lam, bb, reg_vals, reg_dev = (0.0, 0.0, None, None) if reg is None else reg
        S = len(shifts)
        wsb = query("ssq_adashift_bwd_workspace_size", Co, Ci, K, S, is_fc)
        ws, wsn = workspace(wsb, w.device)
        call("ssq_adashift_bwd", _vp(g), _vp(w), _vp(a), _vp(b), _vp(d), _vp(z),
             A.shifts_arg(shifts), S, Co, Ci, K, is_fc, int(hard_r), lo, hi, float(lam), float(bb),
             _vp(reg_dev), _vp(ga), _vp(gb), _vp(reg_vals), ws, wsn, stream_of(w))
        return (ga if need_a else None, gb, None, None, None, None, None, None, None, None, None)


def adashift(alpha, beta, w, delta, zp, shifts, n_bits, sym, hard_t, hard_r, reg=None):
    return AdaShiftFn.apply(alpha, beta, w, delta, zp, tuple(shifts), n_bits, sym, bool(hard_t),
                            bool(hard_r), reg)


class AdaShiftPrep:
    """Loop-invariant state of a conv ChannelQuant in 'adaShift' mode (W, delta, shifts,
    beta frozen, as in the fused loop): the packed int8 floors and h(beta) of
    ssq_adashift_prepare.  `ok` is False when a floor does not fit int8 or the kernel
    window exceeds 256 taps (the caller keeps the recomputing kernels)."""

    def __init__(self, w, beta, delta, shifts, hard_r):
        w, wp = fptr(w.detach(), "weight")
        b, bp = fptr(beta.detach(), "beta")
        d, dp = fptr(delta.detach(), "delta")
        Co, Ci, K, is_fc = geometry(w)
        if is_fc:
            raise A.SSQError("AdaShiftPrep: conv weights only")
        self.geo = (Co, Ci, K)
        self.S = len(shifts)
        self.fpack = torch.empty(w.shape, dtype=torch.int32, device=w.device)
        self.hterm = torch.empty_like(w)
        flag = torch.zeros(1, dtype=torch.int32, device=w.device)
        call("ssq_adashift_prepare", wp, bp, dp, A.shifts_arg(shifts), self.S, Co, Ci, K,
             int(hard_r), _vp(self.fpack), _vp(self.hterm), _vp(flag), stream_of(w))
        self.ok = int(flag.item()) == 0 and K <= 256   # one sync, at preparation time only


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


# Gradient destinations of leaf parameters (data_ptr -> contiguous tensor of the parameter's
# size), set by the data-parallel loop to the slices of its all-reduce bucket (grads_into):
# the backward kernels below then write a parameter's gradient straight into its slice and
# hand autograd None for it -- no AccumulateGrad add, and a deferred finalize (fin_tasks.h)
# may still be pending when backward returns: nothing reads the slice before the collective,
# which runs after the iteration's queued finalizes are flushed.  Each such parameter must
# get its gradient from exactly one kernel per iteration (alpha: its adaShift backward;
# gamma^z / phi^z: their module's epilogue).
GRAD_INTO = {}
INTO_WRITES = [0]       # gradients written straight into a GRAD_INTO slice (test counter)
_INTO_SEEN = set()      # the parameters already written into inside the current context


class grads_into:
    """Context: GRAD_INTO = mapping (param.data_ptr() -> destination) inside.  One context
    spans one iteration's backward: a second kernel producing the same parameter's gradient
    inside it would overwrite the first's contribution instead of adding to it, so it
    raises SSQError instead."""

    def __init__(self, mapping):
        self.mapping = mapping or {}

    def __enter__(self):
        self.prev = dict(GRAD_INTO), set(_INTO_SEEN)
        GRAD_INTO.clear()
        GRAD_INTO.update(self.mapping)
        _INTO_SEEN.clear()
        return self

    def __exit__(self, *exc):
        GRAD_INTO.clear()
        GRAD_INTO.update(self.prev[0])
        _INTO_SEEN.clear()
        _INTO_SEEN.update(self.prev[1])


def _grad_dest(param, numel, device, need=True):
    """(destination tensor, written_into) for a parameter's gradient: its GRAD_INTO slice,
    or a fresh buffer (None when the gradient is not needed)."""
    if param is None or not need:
        return None, False
    d = GRAD_INTO.get(param.data_ptr()) if GRAD_INTO else None
    if d is not None:
        if d.numel() != numel or not d.is_contiguous():
            raise A.SSQError("grads_into: destination does not match the parameter")
        if param.data_ptr() in _INTO_SEEN:
            raise A.SSQError("grads_into: a second kernel produces the gradient of the same "
                             "parameter in one iteration (it would overwrite, not add)")
        _INTO_SEEN.add(param.data_ptr())
        INTO_WRITES[0] += 1
        return d.view(-1), True
    return torch.empty(numel, device=device), False


class AdaShiftPrepFn(torch.autograd.Function):
    """ChannelQuant 'adaShift' forward of SEVERAL prepared weights (e.g. every conv of a
    block, same S and regulariser) in one launch (K5p), and their alpha backward in two
    (K6p, shift regulariser folded in as in AdaShiftFn).  cfg = (hard_t, reg, entries),
    entries[i] = (prep, delta, zp, n_bits, sym); inputs = the alphas; outputs = the Whats."""

    @staticmethod
    def forward(ctx, cfg, *alphas):
        hard_t, reg, entries = cfg
        keep, al, dl, zl = [], [], [], []
        for a, (prep, d, z, n_bits, sym) in zip(alphas, entries):
            a, _ = fptr(a.detach(), "alpha")
            d, _ = fptr(d.detach(), "delta")
            z, _ = fptr(z.detach(), "zero_point")
            al.append(a)
            dl.append(d)
            zl.append(z)
        n = len(entries)
        preps = [e[0] for e in entries]
        outs = [torch.empty_like(p.hterm) for p in preps]
        Co = (C.c_int64 * n)(*[p.geo[0] for p in preps])
        Ci = (C.c_int64 * n)(*[p.geo[1] for p in preps])
        Kk = (C.c_int64 * n)(*[p.geo[2] for p in preps])
        qr = [qrange(e[3], e[4]) for e in entries]
        lo = (C.c_int * n)(*[q[0] for q in qr])
        hi = (C.c_int * n)(*[q[1] for q in qr])
        call("ssq_adashift_fwd_prepared_multi", n, _ptrs([p.fpack for p in preps]),
             _ptrs([p.hterm for p in preps]), _ptrs(al), _ptrs(dl), _ptrs(zl), Co, Ci, Kk, lo, hi,
             preps[0].S, int(hard_t), _ptrs(outs), stream_of(outs[0]))
        ctx.save_for_backward(*al, *dl, *zl)
        ctx.cfg = (hard_t, reg, preps, (Co, Ci, Kk, lo, hi))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        hard_t, reg, preps, (Co, Ci, Kk, lo, hi) = ctx.cfg
        n = len(preps)
        if hard_t or not any(ctx.needs_input_grad[1:]):
            return (None,) * (n + 1)
        saved = ctx.saved_tensors
        al, dl, zl = saved[:n], saved[n:2 * n], saved[2 * n:]
        gs = [torch.zeros_like(p.hterm) if g is None else g.contiguous() for g, p in zip(gs, preps)]
        dst = [_grad_dest(a, a.numel(), a.device) for a in al]
        gas = [d.view(a.shape) for (d, _), a in zip(dst, al)]
        lam, bb, reg_vals, reg_dev = (0.0, 0.0, None, None) if reg is None else reg
        rv = reg_vals if isinstance(reg_vals, (list, tuple)) else [reg_vals] * n
        S = preps[0].S
        wsb = query("ssq_adashift_bwd_prepared_multi_workspace_size", n, Co, Ci, Kk, S)
        ws, wsn = workspace(wsb, gs[0].device)
        call("ssq_adashift_bwd_prepared_multi", n, _ptrs(gs), _ptrs([p.fpack for p in preps]),
             _ptrs([p.hterm for p in preps]), _ptrs(al), _ptrs(dl), _ptrs(zl), Co, Ci, Kk, lo, hi, S,
             float(lam), float(bb), _vp(reg_dev), _ptrs(gas),
             _ptrs(rv) if any(v is not None for v in rv) else None, ws, wsn, stream_of(gs[0]))
        return (None,) + tuple(ga if (need and not into) else None
                               for ga, (_, into), need in zip(gas, dst, ctx.needs_input_grad[1:]))


def adashift_prepared(alpha, prep, delta, zp, n_bits, sym, hard_t, reg=None):
    """One prepared weight (ChannelQuant.forward in 'adaShift' mode)."""
    return AdaShiftPrepFn.apply((bool(hard_t), reg, ((prep, delta, zp, n_bits, sym),)), alpha)[0]


def adashift_prepared_multi(alphas, entries, hard_t, reg=None):
    """Several prepared weights (same S, same regulariser schedule) in one launch."""
    return AdaShiftPrepFn.apply((bool(hard_t), reg, tuple(entries)), *alphas)


def adashift_codes(alpha, beta, w, delta, zp, shifts, n_bits, sym):
    """Hard/hard adaShift: dequantized weight and the integer codes (uint8/int8)."""
    w, wp = fptr(w.detach())
    a, ap = fptr(alpha.detach())
    b, bp = fptr(beta.detach())
    d, dp = fptr(delta.detach())
    z, zpp = fptr(zp.detach())
    Co, Ci, K, is_fc = geometry(w)
    lo, hi = qrange(n_bits, sym)
    out = torch.empty_like(w)
    codes = torch.empty(w.shape, dtype=torch.uint8, device=w.device)
    call("ssq_adashift_fwd", wp, ap, bp, dp, zpp, A.shifts_arg(shifts), len(shifts), Co, Ci, K,
         is_fc, 1, 1, lo, hi, _vp(out), _vp(codes), stream_of(w))
    return out, (codes.view(torch.int8) if sym else codes)


# ------------------------------------------------------------------ K7 learned_hard_sigmoid
class LhsFn(torch.autograd.Function):
    """ChannelQuant 'learned_hard_sigmoid' (channelQuant.py:81-82, :96-118) with the
    dequantized candidates of init_v (channelQuant.py:201-213) recomputed in-kernel."""

    @staticmethod
    def forward(ctx, alpha, w, delta, zp, shifts, n_bits, sym, hard_t):
        w, wp = fptr(w.detach())
        a, ap = fptr(alpha.detach())
        d, dp = fptr(delta.detach())
        z, zpp = fptr(zp.detach())
        Co, Ci, K, is_fc = geometry(w)
        lo, hi = qrange(n_bits, sym)
        out = torch.empty_like(w)
        call("ssq_lhs_fwd", wp, ap, dp, zpp, A.shifts_arg(shifts), len(shifts), Co, Ci, K, is_fc,
             int(hard_t), lo, hi, _vp(out), stream_of(w))
        ctx.save_for_backward(a, w, d, z)
        ctx.cfg = (tuple(shifts), n_bits, sym, hard_t)
        return out

    @staticmethod
    def backward(ctx, g):
        a, w, d, z = ctx.saved_tensors
        shifts, n_bits, sym, hard_t = ctx.cfg
        if hard_t or not ctx.needs_input_grad[0]:
            return (None,) * 8
        g = g.contiguous()
        Co, Ci, K, is_fc = geometry(w)
        lo, hi = qrange(n_bits, sym)
        ga = torch.empty_like(a)
        S = len(shifts)
        wsb = query("ssq_adashift_bwd_workspace_size", Co, Ci, K, S, is_fc)
        ws, wsn = workspace(wsb, w.device)
        call("ssq_lhs_bwd", _vp(g), _vp(w), _vp(a), _vp(d), _vp(z), A.shifts_arg(shifts), S, Co, Ci,
             K, is_fc, lo, hi, _vp(ga), ws, wsn, stream_of(w))
        return (ga, None, None, None, None, None, None, None)


def lhs(alpha, w, delta, zp, shifts, n_bits, sym, hard_t):
    return LhsFn.apply(alpha, w, delta, zp, tuple(shifts), n_bits, sym, bool(hard_t))


# ------------------------------------------------------------------ K8 adaround
class AdaRoundFn(torch.autograd.Function):
    """floor(W/d) + h(beta) (soft) or [beta>=0] (hard), clamp, dequant
    (channelQuant.py:65-78, adaptive_rounding.py:55-67)."""

    @staticmethod
    def forward(ctx, beta, w, delta, zp, n_bits, sym, hard_r, scale, reg=None):
        w, wp = fptr(w.detach())
        b, bp = fptr(beta.detach())
        d, dp = fptr(delta.detach())
        z, zpp = fptr(zp.detach())
        Co, Ci, K, _ = geometry(w)
        per_ci = _delta_per_ci(d, Co, Ci)
        lo, hi = qrange(n_bits, sym)
        out = torch.empty_like(w)
        call("ssq_adaround_fwd", wp, bp, dp, per_ci, zpp, float(scale), Co, Ci, K, int(hard_r), lo,
             hi, _vp(out), None, stream_of(w))
        ctx.save_for_backward(b, w, d, z)
        ctx.cfg = (n_bits, sym, hard_r, scale, per_ci, reg)
        return out

    @staticmethod
    def backward(ctx, g):
        b, w, d, z = ctx.saved_tensors
        n_bits, sym, hard_r, scale, per_ci, reg = ctx.cfg
        if hard_r or not ctx.needs_input_grad[0]:
            return (None,) * 9
        g = g.contiguous()
        Co, Ci, K, _ = geometry(w)
        lo, hi = qrange(n_bits, sym)
        gb = torch.empty_like(w)
        lam, bb, reg_dev = (0.0, 0.0, None) if reg is None else reg
        call("ssq_adaround_bwd", _vp(g), _vp(w), _vp(b), _vp(d), per_ci, _vp(z), float(scale), Co,
             Ci, K, lo, hi, float(lam), float(bb), _vp(reg_dev), _vp(gb), stream_of(w))
        return (gb, None, None, None, None, None, None, None, None)


class AdaRoundMultiFn(torch.autograd.Function):
    """AdaRoundFn for several weights (a block's AdaRound quantizers) in one launch each way
    (ssq_adaround_fwd_multi / _bwd_multi; bit-identical to one launch per weight).
    cfg = (hard_r, reg, entries), entries[i] = (w, delta, zp, n_bits, sym, scale); inputs =
    the betas; outputs = the Whats."""

    @staticmethod
    def forward(ctx, cfg, *betas):
        hard_r, reg, entries = cfg
        n = len(entries)
        ws, bs, ds, zs, outs, geo, pc, sc, lo_, hi_ = [], [], [], [], [], [], [], [], [], []
        for b, (w, d, z, n_bits, sym, scale) in zip(betas, entries):
            w, _ = fptr(w.detach(), "weight")
            b, _ = fptr(b.detach(), "beta")
            d, _ = fptr(d.detach(), "delta")
            z, _ = fptr(z.detach(), "zero_point")
            Co, Ci, K, _ = geometry(w)
            ws.append(w)
            bs.append(b)
            ds.append(d)
            zs.append(z)
            outs.append(torch.empty_like(w))
            geo.append((Co, Ci, K))
            pc.append(_delta_per_ci(d, Co, Ci))
            sc.append(float(scale))
            lo, hi = qrange(n_bits, sym)
            lo_.append(lo)
            hi_.append(hi)
        arr = (C.c_int64 * n)
        args = (arr(*[g[0] for g in geo]), arr(*[g[1] for g in geo]), arr(*[g[2] for g in geo]))
        ints = ((C.c_int * n)(*pc), (C.c_float * n)(*sc), (C.c_int * n)(*lo_), (C.c_int * n)(*hi_))
        call("ssq_adaround_fwd_multi", n, _ptrs(ws), _ptrs(bs), _ptrs(ds), ints[0], _ptrs(zs),
             ints[1], *args, int(hard_r), ints[2], ints[3], _ptrs(outs), stream_of(ws[0]))
        ctx.save_for_backward(*bs, *ws, *ds, *zs)
        ctx.cfg = (hard_r, reg, n, args, ints)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        hard_r, reg, n, args, ints = ctx.cfg
        if hard_r or not any(ctx.needs_input_grad[1:]):
            return (None,) * (n + 1)
        saved = ctx.saved_tensors
        bs, ws, ds, zs = saved[:n], saved[n:2 * n], saved[2 * n:3 * n], saved[3 * n:]
        gs = [torch.zeros_like(w) if g is None else g.contiguous() for g, w in zip(gs, ws)]
        gb = [torch.empty_like(w) for w in ws]
        lam, bb, reg_dev = (0.0, 0.0, None) if reg is None else reg
        call("ssq_adaround_bwd_multi", n, _ptrs(gs), _ptrs(ws), _ptrs(bs), _ptrs(ds), ints[0],
             _ptrs(zs), ints[1], *args, ints[2], ints[3], float(lam), float(bb), _vp(reg_dev),
             _ptrs(gb), stream_of(ws[0]))
        return (None,) + tuple(g if need else None for g, need in zip(gb, ctx.needs_input_grad[1:]))


def adaround_multi(betas, entries, hard_r, reg=None):
    """Several AdaRound weights in one launch (AdaRoundMultiFn)."""
    return AdaRoundMultiFn.apply((bool(hard_r), reg, tuple(entries)), *betas)


def adaround(beta, w, delta, zp, n_bits, sym, hard_r, scale=1.0, reg=None):
    """reg = (lambda, b, reg_dev) folds the rounding regulariser's gradient into the
    backward ((lambda, b) from the device pair reg_dev when given)."""
    return AdaRoundFn.apply(beta, w, delta, zp, n_bits, sym, bool(hard_r), float(scale), reg)


# ------------------------------------------------------------------ K12 regularisers
class ShiftRegFn(torch.autograd.Function):
    """lambda*sum(1-|2p-1|^b) (mode 0) or lambda*-sum p log(p+1e-10) (mode 1) of
    p = get_sig_soft_targets(alpha) (layer_recon_fused_shiftedScale.py:281-282,
    layer_recon_shiftedScale.py:393)."""

    @staticmethod
    def forward(ctx, alpha, lam, b, mode):
        a, ap = fptr(alpha.detach())
        S = a.shape[-1]
        rows = a.numel() // S
        vals = torch.empty(rows, dtype=torch.float32, device=a.device)
        call("ssq_shift_reg", ap, S, rows, int(mode), float(lam), float(b), None, _vp(vals),
             stream_of(a))
        ctx.save_for_backward(a)
        ctx.cfg = (lam, b, mode)
        return vals.sum()

    @staticmethod
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        lam, b, mode = ctx.cfg
        S = a.shape[-1]
        ga = torch.zeros_like(a)
        call("ssq_shift_reg", _vp(a), S, a.numel() // S, int(mode), float(lam), float(b), _vp(ga),
             None, stream_of(a))
        return ga * g, None, None, None


def shift_reg(alpha, lam, b, mode=0):
    return ShiftRegFn.apply(alpha, lam, b, mode)


class RoundRegFn(torch.autograd.Function):
    """lambda*sum(1-|2h(v)-1|^b) with h the rectified sigmoid (block_recon.py:171-174,
    layer_recon_fused_shiftedScale.py:278-279)."""

    @staticmethod
    def forward(ctx, v, lam, b):
        v, vp = fptr(v.detach())
        loss = torch.empty(1, dtype=torch.float32, device=v.device)
        ws, wsn = workspace(query("ssq_round_reg_workspace_size", v.numel()), v.device)
        call("ssq_round_reg", vp, v.numel(), float(lam), float(b), _vp(loss), None, ws, wsn,
             stream_of(v))
        ctx.save_for_backward(v)
        ctx.cfg = (lam, b)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        lam, b = ctx.cfg
        gv = torch.zeros_like(v)
        tmp = torch.empty(1, dtype=torch.float32, device=v.device)
        ws, wsn = workspace(query("ssq_round_reg_workspace_size", v.numel()), v.device)
        call("ssq_round_reg", _vp(v), v.numel(), float(lam), float(b), _vp(tmp), _vp(gv), ws, wsn,
             stream_of(v))
        return gv * g, None, None


def round_reg(v, lam, b):
    return RoundRegFn.apply(v, lam, b)


def round_reg_value(v, lam, b, out=None):
    """Value only (no autograd), written to a 1-element device tensor."""
    v, vp = fptr(v.detach())
    out = torch.empty(1, dtype=torch.float32, device=v.device) if out is None else out
    ws, wsn = workspace(query("ssq_round_reg_workspace_size", v.numel()), v.device)
    call("ssq_round_reg", vp, v.numel(), float(lam), float(b), _vp(out), None, ws, wsn, stream_of(v))
    return out


# ------------------------------------------------------------------ K10
def inpscale_search(w, delta, raw_zp, n_bits, level, threshold):
    """ChannelQuantMSE.init_scale 'max' (channelQuantMSE.py:203-241) -> inp_scale
    shaped (1, Ci, kh, kw) / (1, Ci)."""
    w, wp = fptr(w.detach())
    d, dp = fptr(delta.detach())
    r, rp = fptr(raw_zp.detach())
    Co = w.shape[0]
    J = w.numel() // Co
    inp = torch.empty((1,) + tuple(w.shape[1:]), dtype=torch.float32, device=w.device)
    call("ssq_inpscale_search", wp, dp, rp, Co, J, n_bits, int(level), float(threshold), _vp(inp),
         stream_of(w))
    return inp


def inpscale_fwd(w, inp, delta, raw_zp, n_bits):
    """ChannelQuantMSE.forward (channelQuantMSE.py:267-276)."""
    w, wp = fptr(w.detach())
    i, ip = fptr(inp.detach())
    d, dp = fptr(delta.detach())
    r, rp = fptr(raw_zp.detach())
    Co = w.shape[0]
    out = torch.empty_like(w)
    call("ssq_inpscale_fwd", wp, ip, dp, rp, Co, w.numel() // Co, n_bits, _vp(out), stream_of(w))
    return out


# ------------------------------------------------------------------ K11 / K14
def _lp_M(pred, reduction):
    if reduction == "none":
        return pred.numel() // pred.shape[1]
    return pred.numel()


class Rows:
    """cache[idx] as a lazy target: the loss pass reads the rows in place
    (ssq_lp_loss_rows) instead of a gathered copy."""

    def __init__(self, cache, idx):
        self.cache, self.idx = cache, idx

    def materialize(self):
        return gather_rows2(self.cache, self.idx)[0]


# ------------------------------------------------------------------ in-place row views
# BRECQ's act phase reads its frozen convs' precomputed outputs and the cached block input
# by the batch indices (quant/block_recon.py ROWS_IN_PLACE).  Instead of gathering each into
# a batch buffer, the buffer is registered as a view of cache[idx] (rows_view) and the K13
# epilogue kernels read the rows in place (ssq_epilogue_*_rows, bit-identical to reading the
# gathered batch).  Any other kernel call reaching the buffer through fptr gathers it first
# (_capi.fptr), as does materialize(); the registry lives for one loop (row_views).
def rows_view(buf, cache, idx):
    """Register buf (a contiguous batch buffer, never read by torch ops while registered) as
    cache[idx]; returns buf."""
    if tuple(buf.shape) != (idx.numel(),) + tuple(cache.shape[1:]) or not buf.is_contiguous() \
            or idx.dtype != torch.int64 or not cache.is_contiguous():
        raise A.SSQError("rows_view: buffer, cache and indices do not match")
    A.ROW_VIEWS[buf.data_ptr()] = (buf, cache, idx)
    return buf


def rows_of(t):
    """(cache, idx) when t is a registered row view, else None."""
    if t is None or not A.ROW_VIEWS:
        return None
    e = A.ROW_VIEWS.get(t.data_ptr())
    return None if e is None or e[0].numel() != t.numel() else (e[1], e[2])


class row_views:
    """Context of a loop that registers row views: the registry and any stage still pending
    (a capture that raised between rows_lazy and the kernel that takes it) are emptied on
    exit, so no later call performs an old loop's copy."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        A.ROW_VIEWS.clear()
        A.ROW_STAGE.clear()


def lp_loss_and_grad(pred, tgt, p=2.0, reduction="none", want_grad=True, loss_out=None,
                     relu_mask=False):
    """lp_loss value (1-element device tensor) and d/d pred in one fused pass.  With
    relu_mask, pred is a ReLU output and the gradient is returned at the ReLU's input.
    tgt may be a Rows(cache, idx) target."""
    pred, pp = fptr(pred.detach(), "pred")
    loss = torch.empty(1, dtype=torch.float32, device=pred.device) if loss_out is None else loss_out
    grad = torch.empty_like(pred) if want_grad else None
    ws, wsn = workspace(query("ssq_lp_loss_workspace_size", pred.numel()), pred.device, "loss")
    M = _lp_M(pred, reduction)
    if isinstance(tgt, Rows):
        cache, cp = fptr(tgt.cache.detach(), "tgt cache")
        idx = tgt.idx
        row = cache[0].numel()
        if idx.dtype != torch.int64 or idx.device != pred.device or \
                idx.numel() * row != pred.numel() or tuple(cache.shape[1:]) != tuple(pred.shape[1:]):
            raise A.SSQError("lp_loss: Rows target does not match pred")
        call("ssq_lp_loss_rows", pp, cp, _vp(idx), row, pred.numel(), M, float(p), _vp(loss),
             _vp(grad), None, int(bool(relu_mask)), ws, wsn, stream_of(pred))
        return loss, grad
    tgt, tp = fptr(tgt.detach(), "tgt")
    call("ssq_lp_loss", pp, tp, pred.numel(), M, float(p), _vp(loss),
         _vp(grad), None, int(bool(relu_mask)), ws, wsn, stream_of(pred))
    return loss, grad


class LpLossFn(torch.autograd.Function):
    """lp_loss (quant_layer.py:25-32): forward = value only; backward = one pass that
    writes (1/M)*(p|d|^(p-1))*sgn(d) scaled by the upstream gradient (device scalar)."""

    @staticmethod
    def forward(ctx, pred, tgt, p, reduction):
        loss, _ = lp_loss_and_grad(pred, tgt, p, reduction, want_grad=False)
        ctx.save_for_backward(pred, tgt)
        ctx.cfg = (p, reduction)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        pred, tgt = ctx.saved_tensors
        p, reduction = ctx.cfg
        pred, tgt = pred.contiguous(), tgt.contiguous()
        grad = torch.empty_like(pred)
        gs = g.detach().reshape(1).to(torch.float32).contiguous()
        call("ssq_lp_loss", _vp(pred), _vp(tgt), pred.numel(), _lp_M(pred, reduction), float(p),
             None, _vp(grad), _vp(gs), 0, None, 0, stream_of(pred))
        return grad, None, None, None


def lp_loss(pred, tgt, p=2.0, reduction="none"):
    return LpLossFn.apply(pred, tgt, float(p), reduction)


# ------------------------------------------------------------------ K20 Fisher losses
FISHER_MODES = ("fisher_diag", "fisher_full")


def fisher_loss_and_grad(pred, tgt, fis, mode, relu_mask=False, want_grad=True, loss_out=None,
                         gscale=None, want_loss=True):
    """BRECQ's Fisher-weighted reconstruction loss (block_recon.py:156-162) and d/d pred in
    one entry-point call: mode 'fisher_diag' (one pass; the gradient bit-identical to
    autograd's) or 'fisher_full' (two launches; 4-D pred only).  tgt and fis are batches
    shaped like pred, or both Rows views with the same idx (read in place).  relu_mask as
    lp_loss_and_grad's.  Returns (loss [1] or None, grad or None)."""
    if mode not in FISHER_MODES:
        raise ValueError('Not supported reconstruction loss function: {}'.format(mode))
    pred, pp = fptr(pred.detach(), "pred")
    n, N = pred.numel(), int(pred.shape[0])
    loss = None
    if want_loss:
        loss = torch.empty(1, dtype=torch.float32, device=pred.device) if loss_out is None \
            else loss_out
    grad = torch.empty_like(pred) if want_grad else None
    ws, wsn = workspace(query("ssq_fisher_loss_workspace_size", n, N), pred.device, "fisher")
    tail = (_vp(loss), _vp(grad), _vp(gscale), int(bool(relu_mask)), ws, wsn, stream_of(pred))
    rows = isinstance(tgt, Rows)
    if rows != isinstance(fis, Rows):
        raise A.SSQError("fisher_loss: tgt and fis are both batches or both Rows")
    if rows:
        tc, tp = fptr(tgt.cache.detach(), "tgt cache")
        fc, fp = fptr(fis.cache.detach(), "fis cache")
        idx = tgt.idx
        row = tc[0].numel()
        if fis.idx is not idx and fis.idx.data_ptr() != idx.data_ptr():
            raise A.SSQError("fisher_loss: the target and Fisher rows share one idx")
        if idx.dtype != torch.int64 or idx.device != pred.device or not idx.is_contiguous() or \
                idx.numel() != N or N * row != n or \
                tuple(tc.shape[1:]) != tuple(pred.shape[1:]) or \
                tuple(fc.shape[1:]) != tuple(pred.shape[1:]):
            raise A.SSQError("fisher_loss: Rows target / Fisher rows do not match pred")
        if mode == "fisher_diag":
            call("ssq_fisher_diag_loss_rows", pp, tp, fp, _vp(idx), row, n, _lp_M(pred, "none"),
                 *tail)
        else:
            call("ssq_fisher_full_loss_rows", pp, tp, fp, _vp(idx), n, N, pred.dim(), *tail)
        return loss, grad
    if tuple(tgt.shape) != tuple(pred.shape) or tuple(fis.shape) != tuple(pred.shape):
        raise A.SSQError("fisher_loss: tgt and fis must be shaped like pred")
    tgt, tp = fptr(tgt.detach(), "tgt")
    fis, fp = fptr(fis.detach(), "fis")
    if mode == "fisher_diag":
        call("ssq_fisher_diag_loss", pp, tp, fp, n, _lp_M(pred, "none"), *tail)
    else:
        call("ssq_fisher_full_loss", pp, tp, fp, n, N, pred.dim(), *tail)
    return loss, grad


class FisherLossFn(torch.autograd.Function):
    """The Fisher losses for callers outside the device loop (LossFunction.__call__):
    forward = value only; backward = the gradient pass scaled by the upstream gradient
    (device scalar).  tgt and fis get no gradient (cached data)."""

    @staticmethod
    def forward(ctx, pred, tgt, fis, mode):
        loss, _ = fisher_loss_and_grad(pred, tgt, fis, mode, want_grad=False)
        ctx.save_for_backward(pred, tgt, fis)
        ctx.mode = mode
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        pred, tgt, fis = ctx.saved_tensors
        gs = g.detach().reshape(1).to(torch.float32).contiguous()
        _, grad = fisher_loss_and_grad(pred, tgt, fis, ctx.mode, want_loss=False, gscale=gs)
        return grad, None, None, None


def fisher_loss(pred, tgt, fis, mode):
    return FisherLossFn.apply(pred, tgt, fis, mode)


def gather_rows2(src0, idx, src1=None, out0=None, out1=None):
    """src[idx] for one or two row-major sources (the cached block input / output)."""
    s0, p0 = fptr(src0, "src0")
    idx = idx.to(device=s0.device, dtype=torch.int64).contiguous()
    n = idx.numel()
    row0 = s0[0].numel()
    d0 = torch.empty((n,) + tuple(s0.shape[1:]), dtype=s0.dtype, device=s0.device) if out0 is None else out0
    if src1 is not None:
        s1, p1 = fptr(src1, "src1")
        row1 = s1[0].numel()
        d1 = torch.empty((n,) + tuple(s1.shape[1:]), dtype=s1.dtype, device=s1.device) if out1 is None else out1
    else:
        s1, p1, row1, d1 = None, None, 0, None
    call("ssq_gather_rows2", p0, _vp(d0), row0, p1, _vp(d1), row1, _vp(idx), n, stream_of(s0))
    return d0, d1


def gather_rows2_staged(src0, slot, n, stage_dst, src1=None, out0=None, out1=None):
    """gather_rows2 with the indices slot[:n] of a device ring row, which the same launch
    also copies whole into stage_dst (ssq_gather_rows2_staged)."""
    s0, p0 = fptr(src0, "src0")
    if slot.dtype != torch.int64 or not slot.is_contiguous() or stage_dst.dtype != torch.int64 \
            or stage_dst.numel() != slot.numel() or slot.device != s0.device:
        raise A.SSQError("gather_rows2_staged: int64 contiguous slot and stage_dst of one size")
    row0 = s0[0].numel()
    d0 = torch.empty((n,) + tuple(s0.shape[1:]), dtype=s0.dtype, device=s0.device) if out0 is None else out0
    if src1 is not None:
        s1, p1 = fptr(src1, "src1")
        row1 = s1[0].numel()
        d1 = torch.empty((n,) + tuple(s1.shape[1:]), dtype=s1.dtype, device=s1.device) if out1 is None else out1
    else:
        s1, p1, row1, d1 = None, None, 0, None
    call("ssq_gather_rows2_staged", p0, _vp(d0), row0, p1, _vp(d1), row1, _vp(slot), n,
         _vp(stage_dst), slot.numel(), stream_of(s0))
    return d0, d1


# ------------------------------------------------------------------ K13 fused epilogue
class BiasActFn(torch.autograd.Function):
    """act((y + bias[c]) + res) in one kernel (conv bias add quant_layer.py:250, residual
    add + ReLU quant_block.py:99-117).  The bias is taken as a constant (no
    reconstruction optimises it); gradients flow to y and res."""

    @staticmethod
    def forward(ctx, y, bias, res, relu):
        _, out, _, _ = _k13_forward("bias_act", y, bias, None, None, res, relu)
        ctx.relu = int(relu)
        if relu:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.relu:
            (out,) = ctx.saved_tensors
            g, gp = fptr(g.contiguous(), "grad")
            gin = torch.empty_like(g)
            call("ssq_relu6_bwd" if ctx.relu == 2 else "ssq_relu_bwd", gp, _vp(out), _vp(gin),
                 g.numel(), stream_of(g))
        else:
            gin = g
        return gin, None, (gin if ctx.needs_input_grad[2] else None), None


def k13(y, bias, gamma, phi, res, relu, q, nonaffine_q, lazy):
    """act(((y + bias) * gamma + phi) + res) [-> q], the K13 epilogue: the one place that picks
    the wrapper that runs it.  q is a fusable act quantizer (quant_layer.fusable_act_quantizer)
    or None -- one that is on but not fusable runs as a module after this, at the caller.

        gamma   q     nonaffine_q   bias / relu / res    runs
        set     any   any           any                  epilogue
        None    set   on            any                  epilogue (gamma = phi = None)
        None    set   off           any                  bias_act_quant
        None    None  any           one of them set      bias_act
        None    None  any           none                 materialize(y): y as it is, a row
                                                         view gathered into the batch

    lazy (the block tail the recon loop fuses, TAIL_LAZY) goes to epilogue / bias_act, which
    hand back the placeholder (_lazy_tail) where the fused tail takes the case and run
    otherwise; bias_act_quant has no lazy form, so a lazy caller passes nonaffine_q=True.

    Forward: one kernel body (csrc/recon.hip bias_act) whichever wrapper runs, so bias_act =
    epilogue(gamma = q = None) and bias_act_quant = epilogue(gamma = None, q) bit for bit.
    Backward: a kernel per wrapper.  The first pair is element-wise on both sides
    (ssq_relu_bwd masks with the saved output, ssq_epilogue_bwd with the recomputed one).  The
    second pair sums the act delta / zero-point gradient in different orders -- bias_act_quant
    over the whole tensor, finalised in a launch of its own (ssq_fq_relu_bwd); epilogue per
    (n, c) row, finalised in the next launch's task list, as the fused tail does -- so there
    the two agree to rounding only, and the fused tail is bit-identical to the epilogue form
    and no other.  Hence nonaffine_q: quant_layer.EPI_NONAFFINE_Q at a QuantModule (an A/B
    knob), always on at a block tail."""
    if gamma is not None or (q is not None and nonaffine_q):
        return epilogue(y, bias, gamma, phi, res, relu, q, lazy=lazy)
    if q is not None:
        return bias_act_quant(y, bias, res, relu, q.delta, q.zero_point, q.n_bits, q.sym)
    if bias is not None or relu or res is not None:
        return bias_act(y, bias, res, relu, lazy=lazy)
    return materialize(y)


class LazyK13(collections.namedtuple("LazyK13", "y bias gamma phi res relu q",
                                     defaults=(None, None, None, None, 0, None))):
    """A K13 epilogue whose inputs exist but which has not run (the conv's raw output y and
    k13's inputs): the lazy block tail (out._ssq_tail, _lazy_tail), which the recon loop runs
    fused with the loss and its own backward (epilogue_loss_bwd); a downsample branch deferred
    into that tail (LazyRes(y, bias, gamma, phi)), which the tail's pass applies itself
    (ssq_epilogue_loss_bwd's res_* arguments), returning dL/dy; conv1's epilogue folded into
    conv2's im2col GEMM (x._ssq_epi, lazy_epilogue).  Anywhere else materialize() runs exactly
    the ops the eager site would have."""
    __slots__ = ()

    def materialize(self):
        return k13(*self, nonaffine_q=True, lazy=False)

    def grad_inputs(self):
        """The tensors (or None) of which one must require a gradient for the pass to have any
        to return -- whether a loop iteration steps."""
        q, res = self.q, self.res
        return ([self.y, self.gamma, self.phi] + ([q.delta, q.zero_point] if q is not None else [])
                + (res.grad_inputs() if isinstance(res, LazyK13) else [res]))


LazyRes = LazyEpi = LazyK13


def materialize(res):
    """A residual as a tensor with its values: a LazyRes materialised, a row view gathered."""
    if isinstance(res, LazyRes):
        return res.materialize()
    if res is not None and A.ROW_VIEWS:
        A.materialize_rows(res)
    return res


def _unlazy(res):
    """A LazyRes materialised for an epilogue kernel; a row view stays one (the K13 kernels
    read it in place)."""
    return res.materialize() if isinstance(res, LazyRes) else res


# A/B knob: the downsample branch's epilogue deferred into the block's fused tail (LazyRes;
# bit-identical either way)
FOLD_RESIDUAL = os.environ.get("SSQ_FOLD_RESIDUAL", "1") != "0"


# The fused tail also on planes whose rows are not float4 rows (ResNet-18 layer4's 7x7), in
# the kernel's scalar-row form: layer4.1 2114 it/s against 2085 with the three separate
# passes, layer4.0 unchanged (profiles/r3_ab_knobs.txt).  A/B knob: SSQ_TAIL_SCALAR=0.
TAIL_SCALAR = os.environ.get("SSQ_TAIL_SCALAR", "1") != "0"


def _tail_ok(y, res):
    """The fused tail (epilogue_loss_bwd) takes contiguous NCHW float4 rows (hw % 4 == 0,
    16-B aligned), and scalar rows when TAIL_SCALAR is set."""
    if isinstance(res, LazyRes):
        res = res.y
    if not (y.dim() == 4 and y.is_contiguous() and (res is None or res.is_contiguous())):
        return False
    if TAIL_SCALAR:
        return True
    return ((y.shape[2] * y.shape[3]) % 4 == 0 and y.data_ptr() % 16 == 0
            and (res is None or res.data_ptr() % 16 == 0))


def _lazy_tail(y, bias, gamma, phi, res, relu, q):
    """The lazy tail's placeholder (TAIL_LAZY): an uninitialised tensor like y carrying the
    epilogue's inputs as _ssq_tail; None where the fused tail does not take the case."""
    if int(relu) not in (0, 1) or not _tail_ok(y, res):
        return None
    out = torch.empty_like(y)
    out._ssq_tail = LazyK13(y, bias, gamma, phi, res, int(relu), q)
    return out


def bias_act(y, bias=None, res=None, relu=True, lazy=False):
    """relu: activation code (False/0 identity, True/1 ReLU, 2 ReLU6).  lazy: see
    TAIL_LAZY (the block's final epilogue, fused with the loss and its backward)."""
    out = _lazy_tail(y, bias, None, None, res, relu, None) if lazy else None
    if out is not None:
        return out
    res = _unlazy(res)
    out = BiasActFn.apply(y, bias, res, int(relu))
    if int(relu) == 1:
        # lets a loss that folds the ReLU backward into its own pass (lp_loss relu_mask)
        # back-propagate from the ReLU's inputs directly
        out._ssq_relu_inputs = tuple(t for t in (y, res) if t is not None and t.requires_grad)
    return out


def _chan(t, C_, what):
    """(tensor, pointer) of a per-channel operand, flattened; (None, None) without one."""
    if t is None:
        return None, None
    t, p = fptr(t.detach().reshape(-1), what)
    if t.numel() != C_:
        raise A.SSQError(f"K13 epilogue: {what} must have one value per channel")
    return t, p


_K13Layout = collections.namedtuple("_K13Layout", "y yp yi bp rp ri C hw stage hold")


def _epilogue_layout(y, bias, res, stage=False):
    """A K13 launch's operands: y as launched, the pointers of y / bias / res, (C, hw), and
    hold (what the pointers point into).  y / res may be row views: their pointers (yp / rp)
    are then their caches' and yi / ri their row maps' (None for an operand that is the batch
    itself).  stage (the K13 forward): a pending stage of the iteration's device words
    (_capi.ROW_STAGE) is taken over by the caller's launch -- the maps then point into the
    ring row it copies from -- and `stage` is (src, dst, n) for ssq_epilogue_fwd_rows, or
    (None, None, 0); without a row map the stage is performed here as a copy."""
    st = None
    if stage:
        st = A.take_row_stage()
    elif A.ROW_STAGE:
        A.flush_row_stage()
    yr, rr = rows_of(y), rows_of(res)
    if yr is not None:
        A.check(y, "conv output")
        yp = _vp(yr[0])
    else:
        y, yp = fptr(y.detach(), "conv output")
    C = y.shape[1] if y.dim() > 1 else 1
    hw = y[0, 0].numel() if y.dim() > 2 else 1
    bias, bp = _chan(bias, C, "bias")
    rp = None
    if res is not None:
        if rr is not None:
            A.check(res, "residual")
            rp = _vp(rr[0])
        else:
            res, rp = fptr(res.detach(), "residual")
        if res.shape != y.shape:
            raise A.SSQError("bias_act: residual shape mismatch")

    def rmap(t):
        # the static slot's indices are read from the ring row this launch copies
        if st is not None and t.data_ptr() == st[1].data_ptr():
            return _vp(st[0])
        return _vp(t)
    yi, ri = None if yr is None else rmap(yr[1]), None if rr is None else rmap(rr[1])
    if st is not None and yi is None and ri is None:
        st[1].copy_(st[0])
        st = None
    stg = (None, None, 0) if st is None else (_vp(st[0]), _vp(st[1]), st[0].numel())
    return _K13Layout(y, yp, yi, bp, rp, ri, C, hw, stg, (bias, res))


def _k13_forward(what, y, bias, gamma, phi, res, relu, delta=None, zp=None, n_bits=8, sym=False,
                 keep=True):
    """The K13 forward launch of BiasActFn, BiasActQuantFn and EpilogueFn: layout, quantizer
    operands, ssq_epilogue_fwd_rows (null row maps for an operand that is the batch itself, a
    null stage when none is pending).  keep: the activation before the quantizer is written
    too.  Returns (layout, that activation or None, the quantized output or None, (lo, hi))."""
    L = _epilogue_layout(y, bias, res, stage=True)
    gm, gmp = _chan(gamma, L.C, "gamma")
    ph, php = _chan(phi, L.C, "phi")
    quant = delta is not None
    if quant and (delta.numel() != 1 or zp.numel() != 1):
        raise A.SSQError(f"{what}: per-tensor activation quantizer only")
    d, dp = fptr(delta.detach().reshape(-1), "delta") if quant else (None, None)
    z, zpp = fptr(zp.detach().reshape(-1), "zero_point") if quant else (None, None)
    lo, hi = qrange(n_bits, sym) if quant else (0, 1)
    out = torch.empty_like(L.y) if (keep or not quant) else None
    yq = torch.empty_like(L.y) if quant else None
    call("ssq_epilogue_fwd_rows", L.yp, L.yi, L.bp, gmp, php, L.rp, L.ri, _vp(out), _vp(yq),
         L.y.numel(), L.hw, L.C, int(relu), dp, zpp, lo, hi, *L.stage, stream_of(L.y))
    return L, out, yq, (lo, hi)


class BiasActQuantFn(torch.autograd.Function):
    """K13 epilogue followed by the per-tensor activation fake-quant, one pass:
    fq(act((y + bias[c]) + res)) (quant_layer.py:250,270-272; quant_block.py:99-118).
    The pre-quant activation is written only when a backward will need it.  Backward:
    the STE / delta / zero-point gradients of FakeQuantFn with the ReLU backward folded
    into the same pass (ssq_fq_relu_bwd)."""

    @staticmethod
    def forward(ctx, y, bias, res, delta, zp, relu, n_bits, sym, keep):
        _, out, yq, ctx.q = _k13_forward("bias_act_fq", y, bias, None, None, res, relu, delta, zp,
                                         n_bits, sym, keep)
        ctx.relu = int(relu)
        if keep:
            ctx.save_for_backward(out, delta, zp)
        return yq

    @staticmethod
    def backward(ctx, g):
        out, delta, zp = ctx.saved_tensors
        lo, hi = ctx.q
        g, gp = fptr(g.contiguous(), "grad")
        d, z = delta.detach().contiguous(), zp.detach().contiguous()
        need_in = ctx.needs_input_grad[0] or ctx.needs_input_grad[2]
        gin = torch.empty_like(g) if need_in else None
        gd = torch.empty(1, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[3] else None
        gz = torch.empty(1, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[4] else None
        n = g.numel()
        ws, wsn = workspace(query("ssq_fq_bwd_workspace_size", n, n, 1), g.device)
        if ctx.relu:
            call("ssq_fq_relu6_bwd" if ctx.relu == 2 else "ssq_fq_relu_bwd", _vp(out), gp, _vp(d), _vp(z), n, lo, hi, _vp(gin), _vp(gd),
                 _vp(gz), ws, wsn, stream_of(g))
        else:
            call("ssq_fq_bwd", _vp(out), gp, _vp(d), _vp(z), n, n, 1, lo, hi, _vp(gin), _vp(gd),
                 _vp(gz), ws, wsn, stream_of(g))
        return (gin if ctx.needs_input_grad[0] else None, None,
                gin if ctx.needs_input_grad[2] else None,
                None if gd is None else gd.view(delta.shape),
                None if gz is None else gz.view(zp.shape), None, None, None, None)


def bias_act_quant(y, bias, res, relu, delta, zp, n_bits, sym=False):
    """bias_act followed by fake_quant(delta, zp) in one pass (per-tensor quantizer)."""
    res = _unlazy(res)
    keep = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (y, res, delta, zp))
    return BiasActQuantFn.apply(y, bias, res, delta, zp, int(relu), n_bits, sym, keep)


class EpilogueFn(torch.autograd.Function):
    """act(((y + bias[c]) * gamma[c] + phi[c]) (+ res)) [-> per-tensor act fake-quant] in one
    pass (quant_layer.py:250,266-272; quant_block.py:99-118) -- the general K13 epilogue,
    with the --bias_cal affine gamma^z/phi^z.  Backward (ssq_epilogue_bwd) recomputes the
    pre-activation from the conv output y and returns the y / res / gamma / phi / delta /
    zero_point gradients of the reference's op sequence."""

    @staticmethod
    def forward(ctx, y, bias, gamma, phi, res, delta, zp, relu, n_bits, sym):
        quant = delta is not None
        L, out, yq, (lo, hi) = _k13_forward("epilogue", y, bias, gamma, phi, res, relu, delta, zp,
                                            n_bits, sym, keep=False)
        ctx.cfg = (int(relu), lo, hi, quant, L.C, L.hw)
        ctx.save_for_backward(L.y, bias, gamma, phi, res, delta, zp)
        return yq if quant else out

    @staticmethod
    def backward(ctx, g):
        y, bias, gamma, phi, res, delta, zp = ctx.saved_tensors
        relu, lo, hi, quant, C_, hw = ctx.cfg
        return _epilogue_backward(g, y, bias, gamma, phi, res, delta, zp, relu, lo, hi, quant,
                                  C_, hw, ctx.needs_input_grad)


def _k13_bwd_operands(gamma, phi, delta, zp, need, N, C_, dev_):
    """What the K13 backward and the fused tail hand their kernel besides y / res: gamma / phi /
    delta / zero point flattened; their gradients' destinations where need asks for one
    (_grad_dest; the flags: written into a GRAD_INTO slice, not handed back); the workspace for
    N * C rows, in two alternating slots (a queued finalize of the previous call reads its own)."""
    flat = (lambda t: None if t is None else t.detach().reshape(-1).contiguous())
    ggm, gm_into = _grad_dest(gamma, C_, dev_, need[0])
    gph, ph_into = _grad_dest(phi, C_, dev_, need[1])
    gd = torch.empty(1, device=dev_) if need[2] else None
    gz = torch.empty(1, device=dev_) if need[3] else None
    ws = workspace(query("ssq_epilogue_bwd_workspace_size", N * C_), dev_, _epi_slot())
    return ((flat(gamma), flat(phi), flat(delta), flat(zp)), (ggm, gph, gd, gz),
            (gm_into, ph_into), ws)


def _epilogue_backward(g, y, bias, gamma, phi, res, delta, zp, relu, lo, hi, quant, C_, hw, need):
    """ssq_epilogue_bwd_rows for EpilogueFn (need = its needs_input_grad) and EpiConvGemmFn:
    EpilogueFn.backward's return tuple."""
    g, gp = fptr(g.contiguous(), "grad")
    b = None if bias is None else bias.detach().reshape(-1).contiguous()
    yr, rr = rows_of(y), rows_of(res)
    # (a residual that is the batch itself: contiguous, and alive until the launch)
    r = None if res is None else (res.contiguous() if rr is None else rr[0])
    gy = torch.empty_like(g) if need[0] else None
    gres = torch.empty_like(g) if (res is not None and need[4]) else None
    N = g.numel() // (C_ * hw)
    (gm, ph, d, z), (ggm, gph, gd, gz), (gm_into, ph_into), ws = _k13_bwd_operands(
        gamma, phi, delta, zp, (need[2], need[3], quant and need[5], quant and need[6]), N, C_,
        g.device)
    call("ssq_epilogue_bwd_rows", gp, _vp(y if yr is None else yr[0]),
         None if yr is None else _vp(yr[1]), _vp(b), _vp(gm), _vp(ph), _vp(r),
         None if rr is None else _vp(rr[1]), N, C_, hw, int(relu), _vp(d), _vp(z), lo, hi,
         _vp(gy), _vp(gres), _vp(ggm), _vp(gph), _vp(gd), _vp(gz), *ws, stream_of(g))
    shape = (lambda t, o: None if o is None else o.view(t.shape))
    return (gy if need[0] else None, None, None if gm_into else shape(gamma, ggm),
            None if ph_into else shape(phi, gph), gres, shape(delta, gd), shape(zp, gz), None,
            None, None)


_EPI_SLOT = [0]


def _epi_slot():
    _EPI_SLOT[0] ^= 1
    return _epi_slot_name()


def _epi_slot_name():
    """The workspace slot of the last epilogue backward (tests read its row records)."""
    return "epi%d" % _EPI_SLOT[0]


def set_deferred_finalize(on):
    """Queue the loss / epilogue-backward finalizes onto the next host launch (include/ssq.h,
    csrc/fin_tasks.h); returns the previous setting."""
    return bool(query("ssq_set_deferred_finalize", int(bool(on))))


def flush_finalize(device=None):
    """Launch the finalizes still queued on the current stream."""
    dev_ = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    call("ssq_flush_finalize", C.c_void_p(torch.cuda.current_stream(dev_).cuda_stream))


class deferred_finalize:
    """Context: deferral on inside, flushed and restored on exit (the recon loop body)."""

    def __init__(self, on=True, device=None):
        self.on, self.device = on, device

    def __enter__(self):
        self.prev = set_deferred_finalize(self.on) if self.on else None
        return self

    def __exit__(self, *exc):
        if self.on:
            try:
                flush_finalize(self.device)
            finally:
                set_deferred_finalize(self.prev)


class deferred_prep_fwd:
    """Context (the fused loop's iteration start): the prepared adaShift forward launched
    inside it rides on the next batch gather of its stream (include/ssq.h,
    csrc/prep_ride.h); a forward still queued at exit is launched then."""

    def __init__(self, on=True, device=None):
        self.on, self.device = on, device

    def __enter__(self):
        self.prev = bool(query("ssq_set_deferred_prep_fwd", 1)) if self.on else None
        return self

    def __exit__(self, *exc):
        if self.on:
            dev_ = torch.device("cuda", torch.cuda.current_device()) if self.device is None \
                else self.device
            try:
                call("ssq_flush_prep_fwd", C.c_void_p(torch.cuda.current_stream(dev_).cuda_stream))
            finally:
                query("ssq_set_deferred_prep_fwd", int(self.prev))


# Set by the fused recon loop around its block forward to the block it reconstructs: that
# block's final epilogue is not run; its output is returned as a placeholder carrying the
# epilogue's inputs (_ssq_tail), and the loop runs forward + loss + backward of that
# epilogue in one pass (epilogue_loss_bwd).  Only consumed by BaseQuantBlock._tail, and
# only by the block identical to TAIL_LAZY[0] (nested blocks and hooked blocks run eagerly).
TAIL_LAZY = [None]


# ------------------------------------------------------------------ K13 epilogue into an im2col GEMM
# A ResNet BasicBlock's conv1 epilogue feeds only conv2.  Where conv2's forward and weight
# gradient run as GEMMs over one im2col matrix (ResNet-18 layer3 / layer4: _use_fwd_gemm),
# the block marks conv2 as the consumer (EPI_CONSUMER) while conv1 runs; conv1 then returns
# a placeholder carrying its raw output and its epilogue's inputs (LazyEpi), and conv2 builds
# its im2col matrix from them with the epilogue applied on the fly (ssq_gemm_col_epilogue):
# the epilogue's forward launch and its activation-sized output are gone, the bits are the
# same (col is the im2col of the same values; the backward runs the same ssq_epilogue_bwd on
# the same input gradient).  Any other consumer materialises the placeholder with exactly
# the ops QuantModule.forward runs.  Off by default (SSQ_EPI_GEMM=1 turns it on): the im2col
# build evaluates the epilogue once per column entry, R*S = 9 times per activation, and that
# costs more than the launch it saves -- bench.py's recon loops, ABAB on one box (r5j,
# profiles/r5_epi_gemm_ab.txt): layer3.0 1980 vs 2001 it/s, layer3.1 2012 vs 2029, layer4.0
# 2341 vs 2344, layer4.1 2196 vs 2215 with the fold on vs off.
EPI_INTO_GEMM = os.environ.get("SSQ_EPI_GEMM", "0") == "1"
EPI_CONSUMER = [None]


def lazy_epilogue(y, bias, gamma, phi, relu, q):
    """conv1's raw output y and its K13 epilogue's inputs (QuantModule.forward's fused branch:
    bias, gamma^z / phi^z, activation code, per-tensor act quantizer -- the last only together
    with gamma^z / phi^z) as a placeholder for the consumer conv (x._ssq_epi)."""
    out = torch.empty_like(y)
    out._ssq_epi = LazyEpi(y, bias, gamma, phi, None, int(relu), q)
    return out


def materialize_epi(x):
    epi = getattr(x, "_ssq_epi", None)
    if epi is None:
        if getattr(x, "_ssq_pooled", None) is not None:
            # digits of plane sums (`pooled`) stand for no fp32 tensor another route computes
            raise A.SSQError("pooled code digits reached a consumer that is not the planned fc")
        cc = getattr(x, "_ssq_codes", None)
        return x if cc is None else cc.decode(x)
    return epi.materialize()


class EpiConvGemmFn(torch.autograd.Function):
    """conv2d(epilogue(y), W) (no bias, ungrouped, dilation 1) as ONE im2col build with the
    epilogue folded in (ssq_gemm_col_epilogue) + the strided-batched GEMM of conv_fwd_gemm.
    Backward: the input gradient on MIOpen (the input's values are not read), the weight
    gradient as conv_wgrad_gemm over the saved im2col matrix, then the epilogue's backward
    (ssq_epilogue_bwd) on that input gradient -- the unfused path's kernels and operands."""

    @staticmethod
    def forward(ctx, y, bias, gamma, phi, delta, zp, weight, cfg):
        relu, n_bits, sym, stride, padding = cfg
        Nb, C_, H, W, Co, _, R, S, st, pad, _, _, OH, OW, _ = conv_geometry(
            y.shape, weight.shape, stride, padding)
        y, yp = fptr(y.detach(), "conv output")
        (b, bp), (gm, gmp), (ph, php) = (_chan(bias, C_, "bias"), _chan(gamma, C_, "gamma"),
                                         _chan(phi, C_, "phi"))
        quant = delta is not None
        d, dp = fptr(delta.detach().reshape(-1), "delta") if quant else (None, None)
        z, zpp = fptr(zp.detach().reshape(-1), "zero_point") if quant else (None, None)
        lo, hi = qrange(n_bits, sym) if quant else (0, 1)
        NP, CRS = Nb * OH * OW, C_ * R * S
        col = torch.empty(NP, CRS, dtype=torch.float32, device=y.device)
        call("ssq_gemm_col_epilogue", yp, bp, gmp, php, int(relu), dp, zpp, lo, hi, Nb, C_, H, W,
             R, S, st, pad, _vp(col), stream_of(y))
        out = torch.matmul(weight.detach().reshape(Co, CRS), col.view(Nb, OH * OW, CRS).transpose(1, 2))
        ctx.save_for_backward(y, bias, gamma, phi, delta, zp, weight, col)
        ctx.cfg = (int(relu), lo, hi, quant, C_, H * W, stride, padding)
        return out.view(Nb, Co, OH, OW)

    @staticmethod
    def backward(ctx, g):
        y, bias, gamma, phi, delta, zp, weight, col = ctx.saved_tensors
        relu, lo, hi, quant, C_, hw, stride, padding = ctx.cfg
        need = ctx.needs_input_grad
        g = g.contiguous()
        # the conv's input: only its shape matters to the input gradient and the dy operand
        x_like = torch.empty(y.shape, dtype=y.dtype, device=y.device)
        gw = None
        if need[6]:
            _, dy2 = gemm_operands(x_like, g, weight.shape, stride, padding, want_col=False,
                                   want_dy2=True)
            gw = torch.matmul(dy2, col).view(tuple(weight.shape))
        if not any(need[:6]):
            return None, None, None, None, None, None, gw, None
        gx = torch.ops.aten.convolution_backward(
            g, x_like, weight, None, _pair(stride), _pair(padding), [1, 1], False, [0, 0], 1,
            (True, False, False))[0]
        gy, _, ggm, gph, _, gd, gz, _, _, _ = _epilogue_backward(
            gx, y, bias, gamma, phi, None, delta, zp, relu, lo, hi, quant, C_, hw,
            (need[0], False, need[2], need[3], False, need[4], need[5]))
        return gy, None, ggm, gph, gd, gz, gw, None


def epi_conv_gemm(x, weight, stride, padding):
    """conv2d of a LazyEpi placeholder x through EpiConvGemmFn."""
    e = x._ssq_epi
    delta, zp, n_bits, sym = _q_operands(e.q)
    return EpiConvGemmFn.apply(e.y, e.bias, e.gamma, e.phi, delta, zp, weight,
                               (e.relu, n_bits, sym, stride, padding))


def _q_operands(q):
    """(delta, zero point, n_bits, sym) of a fusable act quantizer, or of none."""
    return (None, None, 8, False) if q is None else (q.delta, q.zero_point, q.n_bits, q.sym)


def epilogue(y, bias, gamma, phi, res, relu, q=None, lazy=False):
    """EpilogueFn with q an (initialised, per-tensor) act quantizer or None.  lazy: see
    TAIL_LAZY (the placeholder must only reach epilogue_loss_bwd)."""
    out = _lazy_tail(y, bias, gamma, phi, res, relu, q) if lazy else None
    if out is not None:
        return out
    delta, zp, n_bits, sym = _q_operands(q)
    return EpilogueFn.apply(y, bias, gamma, phi, _unlazy(res), delta, zp, int(relu), n_bits, sym)


def epilogue_fwd_form(n, hw, aligned=True, rows=False):
    """The K13 forward's form for n elements in planes of hw (ssq_epilogue_fwd_form): 0 scalar,
    1 float4s with a channel lookup per element, 2 float4s inside one plane."""
    return int(query("ssq_epilogue_fwd_form", int(n), int(hw), int(bool(aligned)), int(bool(rows))))


def epilogue_bwd_form(hw, aligned=True, quant=False, res2=False, loss=False):
    """The K13 backward's form for rows of hw elements (ssq_epilogue_bwd_form): (rows per wave
    -- 16: 4 rows of 16 lanes, 4: the A/B register form, 1: a row per wave --, float4 rows)."""
    vec = C.c_int(0)
    rpw = query("ssq_epilogue_bwd_form", int(hw), int(bool(aligned)), int(bool(quant)),
                int(bool(res2)), int(bool(loss)), C.byref(vec))
    return int(rpw), bool(vec.value)


def epilogue_loss_bwd(tail, tgt, M, p=2.0):
    """The fused tail (ssq_epilogue_loss_bwd): for a lazy epilogue placeholder's inputs and a
    Rows target, the lp_loss value at power p (1-element device tensor, mean over M) and the
    gradients the epilogue's backward returns -- (loss, gy, gres, ggamma, gphi, gdelta, gzp,
    gres_gamma, gres_phi), None where the input needs none -- bit-identical to epilogue ->
    lp_loss_and_grad -> backward.  A LazyRes residual (the downsample's deferred epilogue) is
    applied in the same pass: gres is then dL/d(its raw conv output) and gres_gamma /
    gres_phi its gamma^z / phi^z gradients."""
    if not isinstance(tail, LazyK13):
        tail = LazyK13(*tail)           # (the seven fields in order)
    if not isinstance(tgt, Rows):
        raise A.SSQError("epilogue_loss_bwd: the target must be a Rows view of the cache")
    gamma, phi, q = tail.gamma, tail.phi, tail.q
    lres = tail.res if isinstance(tail.res, LazyRes) else None
    res = tail.res if lres is None else lres.y
    L = _epilogue_layout(tail.y, tail.bias, res)
    y, C_, N = L.y, L.C, L.y.shape[0]
    dev_ = y.device
    cache, cp = fptr(tgt.cache.detach(), "tgt cache")
    idx = tgt.idx
    if idx.dtype != torch.int64 or idx.numel() != N or tuple(cache.shape[1:]) != tuple(y.shape[1:]):
        raise A.SSQError("epilogue_loss_bwd: Rows target does not match the output")
    delta, zp, n_bits, sym = _q_operands(q)
    lo, hi = qrange(n_bits, sym) if q is not None else (0, 1)
    loss = torch.empty(1, dtype=torch.float32, device=dev_)
    gy = torch.empty_like(y)
    gres = torch.empty_like(y) if (res is not None and res.requires_grad) else None
    wants = (lambda t: t is not None and t.requires_grad)
    (gm, ph, d, z), (ggm, gph, gd, gz), (gm_into, ph_into), ws = _k13_bwd_operands(
        gamma, phi, delta, zp, (wants(gamma), wants(phi), wants(delta), wants(zp)), N, C_, dev_)
    # the residual's own epilogue (none: null operands, no gradient slots)
    rbias, rgamma, rphi = (None,) * 3 if lres is None else (lres.bias, lres.gamma, lres.phi)
    (rb, rbp), (rg, rgp), (rph_, rphp) = (_chan(rbias, C_, "residual bias"),
                                          _chan(rgamma, C_, "residual gamma"),
                                          _chan(rphi, C_, "residual phi"))
    grg, rg_into = _grad_dest(rgamma, C_, dev_, wants(rgamma))
    grph, rph_into = _grad_dest(rphi, C_, dev_, wants(rphi))
    call("ssq_epilogue_loss_bwd_rows", cp, _vp(idx), int(M), float(p), _vp(loss), L.yp, L.yi,
         L.bp, _vp(gm), _vp(ph), L.rp, L.ri, rbp, rgp, rphp, N, C_, L.hw, int(tail.relu), _vp(d),
         _vp(z), lo, hi, _vp(gy), _vp(gres), _vp(ggm), _vp(gph), _vp(grg), _vp(grph), _vp(gd),
         _vp(gz), *ws, stream_of(y))
    # a gradient written into its GRAD_INTO slice is not handed back (already in place)
    return (loss, gy, gres, None if gm_into else ggm, None if ph_into else gph, gd, gz,
            None if rg_into else grg, None if rph_into else grph)


def adam_step(params, grads, exp_avgs, exp_avg_sqs, beta1, beta2, eps, hyper=None,
              neg_step_size=0.0, bc2_sqrt=1.0):
    """One torch.optim.Adam (single-tensor form) step for every tensor, one launch.
    hyper: device [neg_step_size, bias_correction2_sqrt] (graph-capturable) or None."""
    n = len(params)
    P = C.c_void_p * n
    pa, ga, ma, va = P(), P(), P(), P()
    na = (C.c_int64 * n)()
    for k, (p_, g_, m_, v_) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        for t, nm in ((p_, "param"), (g_, "grad"), (m_, "exp_avg"), (v_, "exp_avg_sq")):
            A.check(t, nm)
            if not t.is_contiguous():
                raise A.SSQError(f"adam_step: {nm} must be contiguous")
        pa[k], ga[k], ma[k], va[k] = p_.data_ptr(), g_.data_ptr(), m_.data_ptr(), v_.data_ptr()
        na[k] = p_.numel()
    call("ssq_adam", n, pa, ga, ma, va, na, float(1 - beta1), float(beta2), float(1 - beta2),
         float(eps), _vp(hyper), float(neg_step_size), float(bc2_sqrt), stream_of(params[0]))


def fc_recon_iter(x_cache, tgt_cache, slot, bs, w, v, what, delta, zp, n_bits, bias, exp_avg,
                  exp_avg_sq, beta1, beta2, eps, g=None, gv_out=None, loss_out=None):
    """One fused BRECQ AdaRound iteration of a Linear layer (ssq_fc_recon_iter, K19): the
    forward on what = AdaRound(w, v) (the first call's from adaround(), every later one's
    written by the previous call), the p = 2 loss and its gradient, then dW, V's gradient
    with the rounding regulariser, V's Adam step and the next what, in two launches.  slot:
    int64 device words (bs indices, then (lambda, b, -lr/bc1, sqrt(bc2)) as fp32).
    Returns (loss, g)."""
    xc, xp = fptr(x_cache, "x cache")
    tc, tp = fptr(tgt_cache, "target cache")
    Co, Ci = int(w.shape[0]), int(w.shape[1])
    if xc.shape[1:].numel() != Ci or tc.shape[1:].numel() != Co or slot.dtype != torch.int64 \
            or not slot.is_contiguous() or slot.numel() < bs + 2:
        raise A.SSQError("fc_recon_iter: shapes / slot")
    for t, nm in ((w, "weight"), (v, "V"), (what, "W^"), (exp_avg, "exp_avg"),
                  (exp_avg_sq, "exp_avg_sq")):
        A.check(t, nm)
        if not t.is_contiguous() or t.numel() != Co * Ci:
            raise A.SSQError(f"fc_recon_iter: {nm} must be contiguous [Co, Ci]")
    d, dp = fptr(delta.detach().reshape(-1), "delta")
    z, zpp = fptr(zp.detach().reshape(-1), "zero_point")
    bt, bp = fptr(bias.detach().reshape(-1), "bias") if bias is not None else (None, None)
    dev_ = w.device
    g = torch.empty(bs, Co, device=dev_) if g is None else g
    loss = torch.empty(1, device=dev_) if loss_out is None else loss_out
    ws, wsn = workspace(query("ssq_fc_recon_workspace_size", Co, Ci, bs), dev_, "fc")
    call("ssq_fc_recon_iter", xp, tp, _vp(slot), bs, _vp(w), _vp(v), _vp(what), dp, zpp, 0,
         2 ** n_bits - 1, bp, Co, Ci, float(1 - beta1), float(beta2), float(1 - beta2),
         float(eps), _vp(exp_avg), _vp(exp_avg_sq), _vp(g), _vp(gv_out), _vp(loss), ws, wsn,
         stream_of(w))
    return loss, g


def _fc_state(name, w, tensors):
    """[Co, Ci] of the fc weight after checking the contiguous fp32 [Co, Ci] arrays."""
    Co, Ci = int(w.shape[0]), int(w.shape[1])
    for t, nm in tensors:
        A.check(t, nm)
        if not t.is_contiguous() or t.numel() != Co * Ci:
            raise A.SSQError(f"{name}: {nm} must be contiguous [Co, Ci]")
    return Co, Ci


def fc_recon_grad(x_cache, tgt_cache, slot, bs, w, v, what, delta, zp, n_bits, bias, gv_out,
                  g=None, loss_out=None):
    """fc_recon_iter up to V's gradient (ssq_fc_recon_grad): the forward on what, the p = 2
    loss and its gradient, dW and V's gradient with the rounding regulariser into gv_out --
    a contiguous tensor of V's size, which may be a slice of a flat all-reduce bucket (4-B
    aligned).  v, what and Adam's state are not written; fc_recon_apply does the rest once
    the gradient is reduced.  Returns (loss, g)."""
    xc, xp = fptr(x_cache, "x cache")
    tc, tp = fptr(tgt_cache, "target cache")
    Co, Ci = _fc_state("fc_recon_grad", w, ((w, "weight"), (v, "V"), (what, "W^"),
                                            (gv_out, "V gradient")))
    if xc.shape[1:].numel() != Ci or tc.shape[1:].numel() != Co or slot.dtype != torch.int64 \
            or not slot.is_contiguous() or slot.numel() < bs + 2:
        raise A.SSQError("fc_recon_grad: shapes / slot")
    d, dp = fptr(delta.detach().reshape(-1), "delta")
    z, zpp = fptr(zp.detach().reshape(-1), "zero_point")
    bt, bp = fptr(bias.detach().reshape(-1), "bias") if bias is not None else (None, None)
    dev_ = w.device
    g = torch.empty(bs, Co, device=dev_) if g is None else g
    loss = torch.empty(1, device=dev_) if loss_out is None else loss_out
    ws, wsn = workspace(query("ssq_fc_recon_workspace_size", Co, Ci, bs), dev_, "fc")
    call("ssq_fc_recon_grad", xp, tp, _vp(slot), bs, _vp(w), _vp(v), _vp(what), dp, zpp, 0,
         2 ** n_bits - 1, bp, Co, Ci, _vp(g), _vp(gv_out), _vp(loss), ws, wsn, stream_of(w))
    return loss, g


def fc_recon_apply(w, v, what, delta, zp, n_bits, slot, bs, grad, exp_avg, exp_avg_sq, beta1,
                   beta2, eps):
    """The rest of fc_recon_iter after fc_recon_grad (ssq_fc_recon_apply): V's Adam step from
    `grad` (the reduced gradient; contiguous, V's size, 4-B aligned) with the step constants
    of `slot`, and what = AdaRound(w, v) of the updated V for the next fc_recon_grad."""
    Co, Ci = _fc_state("fc_recon_apply", w, ((w, "weight"), (v, "V"), (what, "W^"),
                                             (grad, "V gradient"), (exp_avg, "exp_avg"),
                                             (exp_avg_sq, "exp_avg_sq")))
    if slot.dtype != torch.int64 or not slot.is_contiguous() or slot.numel() < bs + 2:
        raise A.SSQError("fc_recon_apply: slot")
    d, dp = fptr(delta.detach().reshape(-1), "delta")
    z, zpp = fptr(zp.detach().reshape(-1), "zero_point")
    call("ssq_fc_recon_apply", _vp(w), _vp(v), _vp(what), dp, zpp, 0, 2 ** n_bits - 1, Co, Ci,
         _vp(slot), bs, _vp(grad), float(1 - beta1), float(beta2), float(1 - beta2), float(eps),
         _vp(exp_avg), _vp(exp_avg_sq), stream_of(w))


def adam_arm(params, exp_avgs, exp_avg_sqs, beta1, beta2, eps, hyper):
    """Arm one Adam step of `params` (include/ssq.h ssq_adam_arm): the next prepared alpha
    backward on the current stream applies it where the gradients are finalised, when it
    can take all of it.  adam_take() then says whether it did."""
    n = len(params)
    P = C.c_void_p * n
    pa, ma, va = P(), P(), P()
    na = (C.c_int64 * n)()
    for k, (p_, m_, v_) in enumerate(zip(params, exp_avgs, exp_avg_sqs)):
        for t, nm in ((p_, "param"), (m_, "exp_avg"), (v_, "exp_avg_sq")):
            A.check(t, nm)
            if not t.is_contiguous():
                raise A.SSQError(f"adam_arm: {nm} must be contiguous")
        pa[k], ma[k], va[k] = p_.data_ptr(), m_.data_ptr(), v_.data_ptr()
        na[k] = p_.numel()
    call("ssq_adam_arm", n, pa, ma, va, na, float(1 - beta1), float(beta2), float(1 - beta2),
         float(eps), _vp(hyper), stream_of(params[0]))


def adam_take(device=None):
    """True when the armed Adam step ran inside a launch; disarms either way."""
    dev_ = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return bool(query("ssq_adam_take", C.c_void_p(torch.cuda.current_stream(dev_).cuda_stream)))


def stream_copy(src, dst):
    call("ssq_stream_copy", _vp(src), _vp(dst), src.numel(), stream_of(src))


def stream_read(src, sink):
    """HBM read-only probe over src (K1 geometry); sink is never written in practice."""
    call("ssq_stream_probe", _vp(src), _vp(sink), src.numel(), 1, stream_of(src))


def stream_write(dst):
    """HBM write-only probe over dst (K1 geometry)."""
    call("ssq_stream_probe", None, _vp(dst), dst.numel(), 2, stream_of(dst))


def set_variant(v):
    return query("ssq_set_variant", int(v))


# ------------------------------------------------------------------ K33 shifted-scale activations
ACTSHIFT_MAX_S = 4


def _actshift_geometry(x):
    """(N, C, HW) of an activation: (N, C, H, W), or (N, C) read as H = W = 1."""
    if x.dim() < 2:
        raise ValueError(f"actshift: activation must be (N, C, ...), got {tuple(x.shape)}")
    N, C_ = int(x.shape[0]), int(x.shape[1])
    hw = 1
    for d in x.shape[2:]:
        hw *= int(d)
    return N, C_, hw


def _actshift_table(t, C_, S, what):
    if tuple(t.shape) != (C_, S):
        raise A.SSQError(f"actshift: {what} must be (C, S) = ({C_}, {S}), got {tuple(t.shape)}")
    return fptr(t.detach(), what)


def _actshift_scalars(delta, zp):
    if delta.numel() != 1 or zp.numel() != 1:
        raise A.SSQError("actshift: delta and zero_point are the per-tensor quantizer's scalars")
    return fptr(delta.detach(), "delta"), fptr(zp.detach(), "zero_point")


def actshift_fwd(x, p, delta, zp, shifts, n_bits, hard=False):
    """ChannelQuantAct 'shiftFeature' forward (ssq_actshift_fwd): the soft mix sum_i Q_i(x) *
    p[c, i] of the per-channel candidates, or the hard choice Q_k(x), k = argmax_i p[c, i]."""
    x, xp = fptr(x.detach(), "x")
    N, C_, hw = _actshift_geometry(x)
    S = len(shifts)
    p, pp = _actshift_table(p, C_, S, "p")
    (delta, dp_), (zp, zpp) = _actshift_scalars(delta, zp)
    y = torch.empty_like(x)
    wsb = query("ssq_actshift_fwd_workspace_size", N, C_, hw, S)
    ws, wsn = workspace(wsb, x.device)
    call("ssq_actshift_fwd", xp, pp, dp_, zpp, A.shifts_arg(shifts), S, N, C_, hw,
         2 ** n_bits - 1, int(bool(hard)), _vp(y), ws, wsn, stream_of(x))
    return y


def actshift_bwd(x, g, p, delta, zp, shifts, n_bits, hard=False, want_dp=True):
    """(dx, dp) of actshift_fwd (ssq_actshift_bwd): dx = g * sum_i p[c, i] * in_i(x) (hard:
    g * in_k(x)), dp[c, i] = sum_{n,h,w} g * Q_i(x) (hard: zeros), deterministic.
    want_dp=False (hard only): dp is None and the launch that writes its zeros is saved."""
    x, xp = fptr(x.detach(), "x")
    g, gp = fptr(g.detach(), "g")
    if g.shape != x.shape:
        raise A.SSQError("actshift_bwd: g must be shaped like x")
    N, C_, hw = _actshift_geometry(x)
    S = len(shifts)
    p, pp = _actshift_table(p, C_, S, "p")
    (delta, dp_), (zp, zpp) = _actshift_scalars(delta, zp)
    dx = torch.empty_like(x)
    if not want_dp and not hard:
        raise A.SSQError("actshift_bwd: the soft backward always computes dp")
    dpt = torch.empty((C_, S), dtype=torch.float32, device=x.device) if want_dp else None
    wsb = query("ssq_actshift_bwd_workspace_size", N, C_, hw, S)
    ws, wsn = workspace(wsb, x.device)
    call("ssq_actshift_bwd", xp, gp, pp, dp_, zpp, A.shifts_arg(shifts), S, N, C_, hw,
         2 ** n_bits - 1, int(bool(hard)), _vp(dx), _vp(dpt), ws, wsn, stream_of(x))
    return dx, dpt


def actshift_init(x, delta, zp, shifts, n_bits):
    """mse[c, i] = sum_{n,h,w} (x - Q_i(x))^2 in one pass over x (ssq_actshift_init): the
    errors ChannelQuantAct.init_v picks each channel's starting shift from."""
    x, xp = fptr(x.detach(), "x")
    N, C_, hw = _actshift_geometry(x)
    S = len(shifts)
    (delta, dp_), (zp, zpp) = _actshift_scalars(delta, zp)
    mse = torch.empty((C_, S), dtype=torch.float32, device=x.device)
    wsb = query("ssq_actshift_init_workspace_size", N, C_, hw, S)
    ws, wsn = workspace(wsb, x.device)
    call("ssq_actshift_init", xp, dp_, zpp, A.shifts_arg(shifts), S, N, C_, hw, 2 ** n_bits - 1,
         _vp(mse), ws, wsn, stream_of(x))
    return mse


class ActShiftFn(torch.autograd.Function):
    """ChannelQuantAct 'shiftFeature': the kernels take the probabilities p (C, S) and return
    dp; the softmax, the (zeta - gamma) stretch and the clamp that make p from alpha stay in
    autograd.  x gets the clamp-masked straight-through gradient of each candidate mixed by
    p -- the 'none' mode's zero gradient would leave every quantizer of a block but its last
    without a signal."""

    @staticmethod
    def forward(ctx, x, p, delta, zp, shifts, n_bits, hard):
        y = actshift_fwd(x, p, delta, zp, shifts, n_bits, hard)
        ctx.save_for_backward(x, p, delta, zp)
        ctx.cfg = (shifts, n_bits, hard)
        return y

    @staticmethod
    def backward(ctx, g):
        x, p, delta, zp = ctx.saved_tensors
        shifts, n_bits, hard = ctx.cfg
        dx, dp = actshift_bwd(x, g, p, delta, zp, shifts, n_bits, hard, want_dp=not hard)
        return (dx if ctx.needs_input_grad[0] else None,
                dp if ctx.needs_input_grad[1] and not hard else None, None, None, None, None, None)


def actshift(x, p, delta, zp, shifts, n_bits, hard=False):
    return ActShiftFn.apply(x, p, delta, zp, tuple(float(s) for s in shifts), int(n_bits),
                            bool(hard))


# ------------------------------------------------------------------ K15/K16 packed export
def pack_encode(what, zp, d1, per_ci, d2, n_bits, qmin, qmax):
    """Hard W_hat -> (packed codes as a uint8 tensor, number of elements whose decode is not
    bit-identical; 0 = exact).  W_hat = ((q - zp[co]) * d1) (* d2[j])."""
    w, wp = fptr(what.detach(), "W_hat")
    Co, Ci, Kk, _ = geometry(w)
    z, zpp = fptr(zp.detach().reshape(-1), "zero_point")
    a, ap = fptr(d1.detach().reshape(-1), "scale")
    b, bp = fptr(d2.detach().reshape(-1), "col_scale") if d2 is not None else (None, None)
    if z.numel() != Co or a.numel() != (Co * Ci if per_ci else Co) or \
            (b is not None and b.numel() != Ci * Kk):
        raise A.SSQError("pack_encode: zp / scale / col_scale sizes do not match the weight")
    nbytes = query("ssq_pack_bytes", w.numel(), n_bits)
    packed = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=w.device)[:nbytes]
    bad = torch.zeros(1, dtype=torch.int32, device=w.device)
    call("ssq_pack_encode", wp, zpp, ap, int(per_ci), bp, Co, Ci, Kk, n_bits, qmin, qmax,
         _vp(packed), _vp(bad), stream_of(w))
    return packed, int(bad.item())


def pack_decode(packed, shape, zp, d1, per_ci, d2, n_bits, qmin):
    """Packed codes -> W_hat (fp32, `shape`)."""
    if packed.device.type != "cuda" or packed.dtype != torch.uint8:
        raise A.SSQError("pack_decode: packed codes must be a uint8 tensor on the HIP device")
    out = torch.empty(shape, dtype=torch.float32, device=packed.device)
    Co, Ci, Kk, _ = geometry(out)
    if packed.numel() < query("ssq_pack_bytes", out.numel(), n_bits):
        raise A.SSQError("pack_decode: packed buffer too small for the shape")
    packed = packed.contiguous()
    z, zpp = fptr(zp.reshape(-1), "zero_point")
    a, ap = fptr(d1.reshape(-1), "scale")
    b, bp = fptr(d2.reshape(-1), "col_scale") if d2 is not None else (None, None)
    call("ssq_pack_decode", _vp(packed), zpp, ap, int(per_ci), bp, Co, Ci, Kk, n_bits, qmin,
         _vp(out), stream_of(out))
    return out


# ------------------------------------------------------------------ K21-K23 integer inference
def code_offset(n_bits, sym):
    """K21 / K22 store a code q as the int8 q - code_offset (= qmin + 128)."""
    return qrange(n_bits, sym)[0] + 128


def _i8_dev(t, name):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise A.SSQError(f"{name}: ssq kernels run on the MI355X (HIP) device only")
    return t.contiguous()


def act_encode(x, delta, zp, n_bits, sym=False, bad=None):
    """An act quantizer's output x = (q - zp) * delta (fp32 NCHW or (N, C); scalar delta, zp)
    -> (int8 codes q - code_offset(n_bits, sym) in NHWC order, channels zero-padded to a
    multiple of 16; the device int32 counter).  The counter -- `bad` when given (it is ADDED
    to), else a fresh zero -- receives the number of elements that are not bit-identical to a
    grid point (NaN / inf included, stored as qmin).  Nothing syncs."""
    x, xp = fptr(x, "x")
    if x.dim() not in (2, 4):
        raise A.SSQError(f"act_encode: expected (N, C, H, W) or (N, C), got {tuple(x.shape)}")
    N, Cc = int(x.shape[0]), int(x.shape[1])
    H, W = (int(x.shape[2]), int(x.shape[3])) if x.dim() == 4 else (1, 1)
    lo, hi = qrange(n_bits, sym)
    Cp = query("ssq_qinfer_cpad", Cc)
    codes = torch.empty((N, H, W, Cp) if x.dim() == 4 else (N, Cp), dtype=torch.int8,
                        device=x.device)
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=x.device)
    call("ssq_act_encode", xp, N, Cc, H, W, float(delta), float(zp), lo, hi, _vp(codes), _vp(bad),
         stream_of(x))
    return codes, bad


class QPrepared:
    """A layer's weight as K23's operand (K22's output) with its (Co, Ci[, R, S]) shape -- at
    `groups` > 1 the grouped kernels' operand (K24's output), Ci then being the channels per
    group; `bad` counts the channels whose zero point is not an integer code (device int32).
    `centred`: the blob holds a column-scaled weight's centred operand m = (q - z) * kcol[j]
    (qweight_prepare(..., kcol=...)), cwz = 0: the dense convs run it without the window sum,
    and `bad` also counts the elements whose |m| exceeds 127.  `wide` (with `centred`, dense
    only): the blob holds m as two int8 digits (qweight_prepare(..., wide=True)), |m| up to
    QWIDE_MAX; only K23's wide forms read it.  `wide_all` (with `wide`, `groups` > 1): the blob is
    the grouped kernels' wide one (qweight_prepare(..., wide=True, wide_all=True)): K26's two digit
    planes, or K25's int32 blob with |m| up to QWIDE_MAX; only the grouped wide forms read it."""

    def __init__(self, blob, shape, bad, groups=1, centred=False, wide=False, wide_all=False):
        self.blob, self.shape, self.bad = blob, tuple(int(s) for s in shape), bad
        self.groups = int(groups)
        self.centred = bool(centred)
        self.wide = bool(wide)
        self.wide_all = bool(wide_all)

    def geometry(self):
        Co, Ci = self.shape[:2]
        R, S = (self.shape[2], self.shape[3]) if len(self.shape) == 4 else (1, 1)
        return Co, Ci, R, S


COLSCALE_MAX_L = 127
QWIDE_MAX = 16319        # |m| and the factors of the wide operand: 128 * 127 + 63
QWIDE_MAX_L = 1024


def colscale_grid(col_scale, max_l=COLSCALE_MAX_L, kmax=COLSCALE_MAX_L):
    """The common integer grid of a column scale (ChannelQuantMSE's c[j] = k[j] / level): the
    smallest L in 1..max_l with, for every j, k[j] = rint(c[j] * L) an integer >= 1 and
    fp32(k[j] / L) == c[j] bit for bit -> (L, k as an int32 CPU tensor); None when there is no
    such L with every k[j] <= kmax (a zero, negative or non-finite entry included).  Host
    arithmetic on a CPU copy of the J floats; L may be smaller than the level the search ran
    with.  The defaults are the int8 operand's limits; the wide operand's are QWIDE_MAX_L and
    QWIDE_MAX."""
    import numpy as np
    c = np.ascontiguousarray(col_scale.detach().reshape(-1).float().cpu().numpy(), dtype=np.float32)
    if c.size == 0 or not np.all(np.isfinite(c)) or not np.all(c > 0):
        return None
    for L in range(1, int(max_l) + 1):
        k = np.rint(c.astype(np.float64) * L)      # exact product: 24 + 10 bits
        if k.min() < 1 or k.max() > kmax:
            continue
        if np.array_equal((k.astype(np.float32) / np.float32(L)).view(np.int32), c.view(np.int32)):
            return L, torch.from_numpy(k.astype(np.int32))
    return None


def _perci_try(v, pad, L, kmax):
    """One L of perci_grid on rows of distinct values `v` [R, U] (fp32; `pad` marks the filler
    entries, which hold the row's maximum): per row the first (kr, base) in ascending order that
    satisfies the predicate -> (found[R], base[R] fp32, k[R, U] int64)."""
    import numpy as np
    R, U = v.shape
    kr = np.arange(1, min(int(kmax), 2 * L) + 1, dtype=np.float64)
    vmax = v.max(axis=1).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        b0 = (vmax[:, None] * L / kr[None, :]).astype(np.float32)                   # [R, Kr]
        bases = np.stack([np.nextafter(b0, np.float32(0)), b0,
                          np.nextafter(b0, np.float32(np.inf))], axis=2)             # [R, Kr, 3]
        k = np.rint(v[:, None, None, :].astype(np.float64) / bases[..., None].astype(np.float64) * L)
        inside = (k >= 1) & (k <= kmax)
        prod = bases[..., None] * (np.where(inside, k, 1).astype(np.float32) / np.float32(L))
        hit = inside & (prod.view(np.int32) == v[:, None, None, :].view(np.int32))
        ok = (hit | pad[:, None, None, :]).all(axis=3) & (bases > 0) & np.isfinite(bases)
    flat = ok.reshape(R, -1)
    first = flat.argmax(axis=1)
    found = flat[np.arange(R), first]
    ik, ib = first // 3, first % 3
    return found, bases[np.arange(R), ik, ib], k[np.arange(R), ik, ib].astype(np.int64)


def perci_grid(scale, Co, Ci, kmax=COLSCALE_MAX_L, max_l=None):
    """The integer grid of a per-(co, ci) weight scale (ChannelQuant's shifted scale, delta[co]
    times a shift target per input channel), from the stored floats alone: one integer L for the
    layer, per row an fp32 base[co] > 0 and per element an integer 1 <= k <= kmax with
        fp32(base[co] * fp32(k / L)) == scale[co, ci]   bit for bit
    -> (L, base as an fp32 CPU tensor [Co], k as an int32 CPU tensor [Co * Ci]); None when there
    is none (a zero, negative or non-finite entry included).  L <= max_l, by default 127 for
    kmax <= 127 and QWIDE_MAX_L beyond.  Among the solutions: the smallest L; then per row the
    smallest k at the row's largest scale; then the smaller base.  A shifted scale stays below
    twice its base, so the search takes k <= 2 L (without that bound every grid with exact k / L
    would be found at L = 1 with the k of its true L, e.g. 31, 32, 33).  Per (L, k at the row's
    maximum) the base is one of the three fp32 neighbours of max * L / k.

    Host arithmetic on a CPU copy, on each row's distinct values, vectorised over rows and the
    candidate (k, base); an L is first tried on the row with the most distinct values (eight of
    them), which rejects nearly every L that fails."""
    import numpy as np
    Co, Ci = int(Co), int(Ci)
    c = np.ascontiguousarray(scale.detach().reshape(-1).float().cpu().numpy(), dtype=np.float32)
    if c.size == 0 or c.size != Co * Ci or not np.all(np.isfinite(c)) or not np.all(c > 0):
        return None
    if max_l is None:
        max_l = COLSCALE_MAX_L if kmax <= COLSCALE_MAX_L else QWIDE_MAX_L
    c = c.reshape(Co, Ci)
    srt = np.sort(c, axis=1)
    new = np.concatenate([np.ones((Co, 1), bool), srt[:, 1:] != srt[:, :-1]], axis=1)
    U = int(new.sum(axis=1).max())
    # v[co]: the row's distinct values, ascending, filled up with its maximum (pad)
    slot = np.cumsum(new, axis=1) - 1
    v = np.repeat(srt[:, -1:], U, axis=1)
    v[np.arange(Co)[:, None], slot] = srt
    pad = np.arange(U)[None, :] >= new.sum(axis=1)[:, None]
    probe = int(new.sum(axis=1).argmax())
    pv = v[probe:probe + 1, np.unique(np.linspace(0, U - 1, min(U, 8)).astype(int))]
    ppad = np.zeros(pv.shape, bool)
    for L in range(1, int(max_l) + 1):
        if not _perci_try(pv, ppad, L, kmax)[0][0]:
            continue
        per = max(1, (1 << 21) // (min(int(kmax), 2 * L) * 3 * U))
        base, kk, good = np.empty(Co, np.float32), np.empty((Co, U), np.int64), True
        for r0 in range(0, Co, per):
            found, b, k = _perci_try(v[r0:r0 + per], pad[r0:r0 + per], L, kmax)
            if not found.all():
                good = False
                break
            base[r0:r0 + per], kk[r0:r0 + per] = b, k
        if not good:
            continue
        # back from the distinct values to the elements
        idx = (c[:, :, None] == v[:, None, :]).argmax(axis=2) if U <= 16 else np.stack(
            [np.searchsorted(v[i, :int(new[i].sum())], c[i]) for i in range(Co)])
        k = np.take_along_axis(kk, idx, axis=1)
        return L, torch.from_numpy(base), torch.from_numpy(k.reshape(-1).astype(np.int32))
    return None


def perci_plain(grid):
    """A perci_grid result whose every k equals L: a plain per-co weight with scale = base."""
    return grid is not None and bool((grid[2] == grid[0]).all())


def wide_digits(m):
    """The wide operand's two int8 digits of an integer array |m| <= QWIDE_MAX: (h, l) with
    m = 128 h + l, l = ((m + 64) mod 128) - 64 in [-64, 63] (floor mod), h in [-127, 127]."""
    import numpy as np
    m = np.asarray(m, dtype=np.int64)
    lo = np.mod(m + 64, 128) - 64
    return (m - lo) // 128, lo


# (grouped, factors: None | "col" | "perci") -> (the blob's byte query, the prepare entry point)
_QPREPARE_FNS = {
    (False, None): ("ssq_qweight_prepared_bytes", "ssq_qweight_prepare"),
    (False, "col"): ("ssq_qweight_prepared_bytes", "ssq_qweight_prepare_colscale"),
    (False, "perci"): ("ssq_qweight_prepared_bytes", "ssq_qweight_prepare_perci"),
    (True, None): ("ssq_qweight_prepared_bytes_grouped", "ssq_qweight_prepare_grouped"),
    (True, "col"): ("ssq_qweight_prepared_bytes_grouped", "ssq_qweight_prepare_grouped_colscale"),
    (True, "perci"): ("ssq_qweight_prepared_bytes_grouped", "ssq_qweight_prepare_grouped_perci"),
}

# SSQ_QCONV_WIDE=auto|1 (qweight_prepare_scaled): auto, the wide blob only where the int8 one
# does not hold the scaled weight; 1, every dense centred blob on it (the A/B run,
# profiles/int_infer_wide_rate.txt, and the bit-identity test).
QCONV_WIDE = os.environ.get("SSQ_QCONV_WIDE", "auto")
if QCONV_WIDE not in ("auto", "1"):
    raise ValueError(f"SSQ_QCONV_WIDE={QCONV_WIDE!r}: expected auto or 1")


def qweight_prepare(packed, shape, zp, n_bits, qmin, groups=1, kcol=None, kfac=None, wide=False,
                    wide_all=False):
    """Packed codes (pack_encode's layout) + zp[co] -> QPrepared.  `shape` is the weight's own
    (Co, Cig, R, S); `groups` > 1 prepares for the grouped kernels (K24).  `kcol`: the int32
    column factors k[j], j = (ci, r, s) (colscale_grid), of a column-scaled weight: the blob then
    holds the centred operand (q - zp[co]) * k[j] (`centred`).  `kfac`: the int32 factors
    k[co, ci] (perci_grid) of a per-(co, ci) scaled weight instead, the operand
    (q - zp[co]) * k[co, ci].  `wide` (with either, dense only): the two-digit blob, factors and
    |m| up to QWIDE_MAX instead of 127.  `wide_all` (with `wide`): a grouped weight too, on the
    grouped kernels' wide blob (K26's two digit planes; a depthwise weight's int32 blob, column
    factors only)."""
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8:
        raise A.SSQError("qweight_prepare: packed codes must be a uint8 tensor")
    packed = _i8_dev(packed, "qweight_prepare")
    if len(shape) not in (2, 4):
        raise A.SSQError(f"qweight_prepare: weight shape {tuple(shape)} is neither Linear nor Conv2d")
    groups = int(groups)
    if groups < 1 or (groups > 1 and len(shape) != 4):
        raise A.SSQError(f"qweight_prepare: groups = {groups} needs a Conv2d weight and groups >= 1")
    if kcol is not None and kfac is not None:
        raise A.SSQError("qweight_prepare: a column scale and a per-(co, ci) scale do not go together")
    if wide and kcol is None and kfac is None:
        raise A.SSQError("qweight_prepare: the wide blob holds a scaled weight (kcol or kfac)")
    if wide and groups > 1 and not wide_all:
        raise A.SSQError("qweight_prepare: the wide blob is dense only: the grouped kernels (K26) "
                         "read int8 operands")
    prep = QPrepared(None, shape, torch.zeros(1, dtype=torch.int32, device=packed.device), groups)
    Co, Ci, R, S = prep.geometry()
    if packed.numel() < query("ssq_pack_bytes", Co * Ci * R * S, n_bits):
        raise A.SSQError("qweight_prepare: packed buffer too small for the shape")
    z, zpp = fptr(zp.detach().reshape(-1), "zero_point")
    if z.numel() != Co:
        raise A.SSQError("qweight_prepare: zero point must have one entry per output channel")
    extra, factors = (), None
    if kcol is not None or kfac is not None:
        factors, name, want = (("col", "kcol", Ci * R * S) if kfac is None else ("perci", "kfac", Co * Ci))
        kc = torch.as_tensor(kcol if kfac is None else kfac).detach().reshape(-1)
        lim = QWIDE_MAX if wide else COLSCALE_MAX_L
        if kc.dtype.is_floating_point or kc.numel() != want:
            raise A.SSQError(f"qweight_prepare: {name} must hold one integer per " +
                             ("(ci, r, s) column" if kfac is None else "(co, ci)"))
        if int(kc.min()) < 1 or int(kc.max()) > lim:
            raise A.SSQError(f"qweight_prepare: {name} must lie in [1, {lim}]")
        kc = kc.to(device=packed.device, dtype=torch.int32).contiguous()
        prep.centred, prep.wide = True, bool(wide)
        prep.wide_all = bool(wide) and groups > 1
        extra = (_vp(kc),)
    geo = (Co, Ci, R, S) + ((groups,) if groups > 1 else ())
    if wide:
        size_fn, prepare_fn = (("ssq_qweight_prepared_bytes_grouped_wide", "ssq_qweight_prepare_grouped_wide")
                               if groups > 1 else
                               ("ssq_qweight_prepared_bytes_wide", "ssq_qweight_prepare_wide"))
        extra += (int(kfac is not None),)
    else:
        size_fn, prepare_fn = _QPREPARE_FNS[groups > 1, factors]
    prep.blob = torch.empty(max(query(size_fn, *geo), 1), dtype=torch.uint8, device=packed.device)
    call(prepare_fn, _vp(packed), zpp, *extra, *geo, int(n_bits), int(qmin), _vp(prep.blob),
         _vp(prep.bad), stream_of(packed))
    return prep


def qweight_prepare_scaled(packed, shape, zp, n_bits, qmin, groups=1, kcol=None, kfac=None,
                           wide=False, wide_all=False):
    """qweight_prepare for a scaled weight whose operand may leave int8: the int8 blob where it
    holds the weight (every factor <= 127 and `bad` zero, one device word read), else, with
    `wide` and a dense weight, the wide blob; elsewhere the int8 blob with its `bad` set (no
    factor above 127 reaches it: None then).  SSQ_QCONV_WIDE=1: with `wide`, every dense scaled
    weight takes the wide blob.  `wide_all` (with `wide`): a grouped or depthwise weight counts as
    a dense one here and takes the grouped kernels' wide blob by the same rule."""
    k = torch.as_tensor(kcol if kfac is None else kfac)
    dense = int(groups) == 1 or bool(wide_all)
    fits = int(k.max()) <= COLSCALE_MAX_L
    if not (wide and dense and (QCONV_WIDE == "1" or not fits)):
        if not fits:
            return None
        prep = qweight_prepare(packed, shape, zp, n_bits, qmin, groups, kcol, kfac)
        if not (wide and dense and int(prep.bad.item())):
            return prep
    return qweight_prepare(packed, shape, zp, n_bits, qmin, groups, kcol, kfac, wide=True,
                           wide_all=wide_all)


QCONV_KINDS = {1: "depthwise", 2: "grouped"}

# A centred blob (a column-scaled weight's, QPrepared.centred) on K23's CENTRED instantiations:
# no window-sum MFMA, no 0/1-row traffic; bit-identical to the shift-and-correct ones on such a
# blob (profiles/int_infer_colscale_rate.txt).  A/B knob: SSQ_QCONV_CENTRED=0.
QCONV_CENTRED = os.environ.get("SSQ_QCONV_CENTRED", "1") != "0"


def _qconv_fn(prepared, groups, form):
    """The entry point of `form` ("fwd" | "codes_fwd" | "codes_res_fwd") for a prepared weight."""
    if getattr(prepared, "wide", False):
        if int(groups) > 1:
            if not getattr(prepared, "wide_all", False):
                raise A.SSQError("qconv: a wide blob is dense only: the grouped kernels (K26) read "
                                 "int8 operands")
            if form == "codes_res_fwd":
                raise A.SSQError("qconv: the grouped kernels (K25 / K26) take no residual operand")
            return f"ssq_qconv_i8_grouped_wide_{form}"
        return f"ssq_qconv_i8_wide_{form}"
    if int(groups) > 1:
        return f"ssq_qconv_i8_grouped_{form}"
    if QCONV_CENTRED and getattr(prepared, "centred", False):
        return f"ssq_qconv_i8_centred_{form}"
    return f"ssq_qconv_i8_{form}"


# K23 split along K (csrc/qinfer.hip, "K23 split along K"): Z workgroups per output tile each walk
# a slice of the k steps, a finish kernel adds the slices and runs K23's epilogue; bit-identical
# to the one-kernel form.  qconv_splits is the host rule.  A/B knob: SSQ_QCONV_SPLITK=auto|0|<Z>.
QCONV_SPLITK = os.environ.get("SSQ_QCONV_SPLITK", "auto")
if QCONV_SPLITK != "auto" and not QCONV_SPLITK.isdigit():
    raise ValueError(f"SSQ_QCONV_SPLITK={QCONV_SPLITK!r}: expected auto, 0 or a number of slices")
QSPLIT_MAX = 16          # the ABI's bound on Z
# The rule's two thresholds, from profiles/int_infer_smallplane_rate.txt ("keep rule" there, which
# the tool derives from its in-graph medians; a Z is kept where it saves more than the unsplit
# form's spread in BOTH the fp32 and the code-emitting form, the rule not knowing which will
# run): a shape is split, doubling Z up to 8, only while its grid, ceil(M/64) * ceil(Co/64) * Z
# workgroups, stays at or below QSPLIT_WORKGROUPS and each slice keeps at least QSPLIT_STEPS k
# steps.  QSPLIT_STEPS is the fewest steps per slice of a kept (class, Z); QSPLIT_WORKGROUPS the
# largest split grid of one.  The file's rows (saved us, fp32 / code-emitting form):
#   56 wgs, nk 72 (512 3x3 @7, batch 8):   Z=4 saves 18.4 / 12.1 of 32.7 / 37.9   (224 wgs, 18 steps)
#   100 wgs, nk 36 (256 3x3 @14, batch 8): Z=2 saves 5.2 / 2.0; Z=4 loses on codes   (200 wgs, 18 steps)
#   56 wgs, nk 32 (1x1 2048->512, batch 8): Z=2 saves 5.6 / 1.7; Z=4 loses on codes  (112 wgs, 16 steps)
#   784 wgs, nk 36 and 392 wgs, nk 32 (batch 64): no Z clears
#   392 wgs, nk 72 (512 3x3 @7, batch 64): Z=2 saves 3.6 / 1.8 and is given up: two thresholds
#   cannot admit its 784-workgroup split and refuse the 1x1's at batch 64, which loses
# so QSPLIT_WORKGROUPS = 224 and QSPLIT_STEPS = 16: no class is split that was not measured to clear.
QSPLIT_WORKGROUPS = 224
QSPLIT_STEPS = 16


def qconv_splits(M, Co, Kp):
    """The number of K slices Z in {1, 2, 4, 8} for a dense integer conv of M output pixels, Co
    channels and Kp padded taps (a pure function of the three and of SSQ_QCONV_SPLITK): 1 unless
    the split grid stays within QSPLIT_WORKGROUPS workgroups and nk / Z, nk = Kp / 64, at or above
    QSPLIT_STEPS.  Never above nk.  SSQ_QCONV_SPLITK=0: always 1; =<Z>: the largest of 1, 2, 4, 8
    that is <= min(Z, nk) whatever the grid."""
    nk = max(int(Kp) // 64, 1)
    if QCONV_SPLITK == "0":
        return 1
    if QCONV_SPLITK != "auto":
        if not QCONV_SPLITK.isdigit():
            raise A.SSQError(f"qconv_splits: SSQ_QCONV_SPLITK={QCONV_SPLITK!r} is not auto, 0 or a "
                             f"number of slices")
        want, Z = min(int(QCONV_SPLITK), nk, 8), 1
        while 2 * Z <= want:
            Z *= 2
        return Z
    wg = -(-int(M) // 64) * -(-int(Co) // 64)
    Z = 1
    while Z < 8 and 2 * Z <= nk and wg * 2 * Z <= QSPLIT_WORKGROUPS and nk // (2 * Z) >= QSPLIT_STEPS:
        Z *= 2
    return Z


def qconv_split_workspace_bytes(prepared, N, H, W, stride, padding, splits):
    """Bytes of the split-K workspace for a dense prepared weight on an (N, H, W) code plane
    (ssq_qconv_i8_splitk_workspace_size); 0 where the entry points refuse the split."""
    Co, Ci, R, S = prepared.geometry()
    return query("ssq_qconv_i8_splitk_workspace_size", int(N), int(H), int(W), Co, R, S,
                 int(stride), int(padding), query("ssq_qinfer_cpad", Ci), int(splits),
                 int(QCONV_CENTRED and getattr(prepared, "centred", False)))


def _qconv_split(name, prepared, groups, form, splits, workspace, codes, stride, padding):
    """A split-K call of `form`: (the entry point; the workspace tensor, which the caller holds
    until its call is issued; the (splits, ws, ws_bytes) arguments that follow the parent's).
    The workspace is the caller's, or a torch.empty per call like the output (every element is
    written before it is read).  A grouped weight has no split form.  A split the ABI refuses
    reaches it with no workspace, so the refusal and its message are the entry point's."""
    if int(groups) > 1:
        raise A.SSQError(f"{name}: splits need a dense weight (groups == 1), got groups = {groups}")
    if getattr(prepared, "wide", False):
        raise A.SSQError(f"{name}: a wide blob has no split-K form (the partial kernel holds one "
                         "int32 accumulator set)")
    centred = QCONV_CENTRED and getattr(prepared, "centred", False)
    fn = f"ssq_qconv_i8_{'centred_' if centred else ''}splitk_{form}"
    if workspace is None:
        N = int(codes.shape[0])
        H, W = (int(codes.shape[1]), int(codes.shape[2])) if codes.dim() == 4 else (1, 1)
        nbytes = qconv_split_workspace_bytes(prepared, N=N, H=H, W=W, stride=_pair(stride)[0],
                                             padding=_pair(padding)[0], splits=splits)
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=codes.device) if nbytes else None
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8
          or workspace.device != codes.device or not workspace.is_contiguous()):
        raise A.SSQError(f"{name}: workspace must be a contiguous uint8 tensor on the output's device")
    nb = 0 if workspace is None else workspace.numel()
    return fn, workspace, (int(splits), None if workspace is None else _vp(workspace), nb)


def qconv_kind(prepared):
    """The kernel `qconv` runs for a prepared weight: "dense" (K23), "depthwise" (K25) or
    "grouped" (K26)."""
    if prepared.groups == 1:
        return "dense"
    Co, Cig, _, _ = prepared.geometry()
    kind = query("ssq_qconv_grouped_kind", Co, Cig, prepared.groups)
    if kind not in QCONV_KINDS:
        raise A.SSQError(f"qconv_kind: invalid grouped geometry {prepared.shape}, groups = {prepared.groups}")
    return QCONV_KINDS[kind]


def qconv(codes_or_x, prepared, scale, stride=1, padding=0, groups=1, act_zp=0.0, act_bits=8,
          act_sym=False, act_delta=None, bad=None, splits=None, workspace=None):
    """y = fp32(I) * scale[co] (fp32 NCHW / (N, Co)), I the exact integer conv of the centred
    codes.  `codes_or_x`: act_encode's int8 codes, or the fp32 activation itself, which is then
    encoded with (act_delta, act_zp, act_bits, act_sym), off-grid elements ADDED to `bad`.
    (act_zp, act_bits, act_sym) are the act quantizer's either way.
    `splits` (dense weights only): None or 1 the one-kernel form; Z in 2..16 (at most the weight's
    k steps) the split-K form, the same bits; `workspace`: a caller-owned uint8 device tensor of
    qconv_split_workspace_bytes for it instead of one allocated per call."""
    args, keep, (N, Co, OH, OW, conv) = _qconv_args(
        "qconv", codes_or_x, prepared, scale, stride, padding, groups, act_zp, act_bits, act_sym,
        act_delta, bad)
    y = torch.empty((N, Co, OH, OW) if conv else (N, Co), dtype=torch.float32,
                    device=keep[0].device)
    if splits is not None and int(splits) != 1:
        fn, ws, tail = _qconv_split("qconv", prepared, groups, "fwd", splits, workspace, keep[0],
                                    stride, padding)
        call(fn, *args, _vp(y), *tail, stream_of(y))
        return y
    call(_qconv_fn(prepared, groups, "fwd"), *args, _vp(y), stream_of(y))
    return y


def _qconv_args(name, codes_or_x, prepared, scale, stride, padding, groups, act_zp, act_bits,
                act_sym, act_delta, bad):
    """qconv's and qconv_codes's shared front: the int8 operand (an fp32 input encoded first)
    and the first sixteen arguments of the conv entry points, + (N, Co, OH, OW, 4-D?)."""
    stride, padding = _pair(stride), _pair(padding)
    if padding is None or stride[0] != stride[1] or padding[0] != padding[1]:
        raise A.SSQError(f"{name}: square stride / padding only")
    if codes_or_x.dtype == torch.float32:
        if act_delta is None:
            raise A.SSQError(f"{name}: an fp32 input needs act_delta to be encoded")
        codes, _ = act_encode(codes_or_x, act_delta, act_zp, act_bits, act_sym, bad=bad)
    elif codes_or_x.dtype == torch.int8:
        codes = _i8_dev(codes_or_x, name)
    else:
        raise A.SSQError(f"{name}: expected int8 codes or an fp32 activation, got {codes_or_x.dtype}")
    groups = int(groups)
    pg = getattr(prepared, "groups", 1)
    if groups != pg:
        raise A.SSQError(f"{name}: groups = {groups}, but the weight was prepared with groups = {pg} "
                         f"(qweight_prepare(..., groups=...))")
    Co, Cig, R, S = prepared.geometry()
    Ci = Cig * groups      # the activation's channels
    Cp = query("ssq_qinfer_cpad", Ci)
    if codes.dim() not in (2, 4) or codes.shape[-1] != Cp or (codes.dim() == 2) != (len(prepared.shape) == 2):
        raise A.SSQError(f"{name}: codes {tuple(codes.shape)} do not match the weight {prepared.shape}")
    N = int(codes.shape[0])
    H, W = (int(codes.shape[1]), int(codes.shape[2])) if codes.dim() == 4 else (1, 1)
    s, sp = fptr(scale.detach().reshape(-1), "scale")
    if s.numel() != Co:
        raise A.SSQError(f"{name}: scale must have one entry per output channel")
    OH = (H + 2 * padding[0] - R) // stride[0] + 1
    OW = (W + 2 * padding[0] - S) // stride[0] + 1
    lo, hi = qrange(act_bits, act_sym)
    args = (_vp(codes), _vp(prepared.blob), sp, N, Ci, H, W, Co, R, S, int(stride[0]),
            int(padding[0]), groups, float(act_zp), lo, hi)
    return args, (codes, s), (N, Co, max(OH, 0), max(OW, 0), codes.dim() == 4)


ActQuant = collections.namedtuple("ActQuant", "delta zp n_bits sym")   # a per-tensor act quantizer


class _Quantized:
    """A tagged tensor's act quantizer: `q`, an ActQuant (what quantizer() returns), with its
    fields also as plain attributes.  Built in the subclass's __init__ by tuple.__new__: one is
    made per emitting layer per forward, and the namedtuple's own constructor costs as much as
    the rest of the object."""

    def quantizer(self):
        return self.q


class CarriedCodes(_Quantized):
    """What an int8 code tensor carried between two integer layers stands for (the tensor's
    `_ssq_codes`): the logical (N, C, H, W) -- (N, C) for a Linear's -- and the act quantizer
    (delta, zp, n_bits, sym) whose output (q - zp) * delta the codes hold, q = code +
    code_offset.  materialize_epi decodes it for a consumer that is not an integer layer."""

    def __init__(self, shape, delta, zp, n_bits, sym):
        self.shape = tuple(int(v) for v in shape)
        self.q = q = tuple.__new__(ActQuant, (float(delta), float(zp), int(n_bits), bool(sym)))
        self.delta, self.zp, self.n_bits, self.sym = q

    def decode(self, codes):
        x = act_decode(codes, self.shape[1], self.delta, self.zp, self.n_bits, self.sym)
        return x.view(self.shape)


def _channel_vecs(name, C, bias, gamma, phi, per="output channel"):
    """The epilogue's optional per-channel vectors -> (the contiguous tensors, which the caller
    holds until its call is issued; their [bias, gamma, phi] device pointers)."""
    keep, ptrs = [], []
    for t, nm in ((bias, "bias"), (gamma, "gamma"), (phi, "phi")):
        v, vp = (None, None) if t is None else fptr(t.detach().reshape(-1), nm)
        if v is not None and v.numel() != C:
            raise A.SSQError(f"{name}: {nm} must have one entry per {per}")
        keep.append(v)
        ptrs.append(vp)
    return keep, ptrs


def _nhwc_codes(name, codes):
    """act_encode's 4-D int8 codes, contiguous on the device -> (codes, (N, H, W, Cpad))."""
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.int8:
        raise A.SSQError(f"{name}: expected int8 codes")
    codes = _i8_dev(codes, name)
    if codes.dim() != 4 or codes.shape[-1] % 16:
        raise A.SSQError(f"{name}: codes {tuple(codes.shape)} are not (N, H, W, Cpad)")
    return codes, tuple(int(v) for v in codes.shape)


def carried(codes, shape, delta, zp, n_bits, sym):
    """`codes` tagged as a carried tensor (see CarriedCodes)."""
    codes._ssq_codes = CarriedCodes(shape, delta, zp, n_bits, sym)
    return codes


def act_decode(codes, C, delta, zp, n_bits, sym=False):
    """act_encode's inverse: int8 codes (N, H, W, Cpad) or (N, Cpad) with C real channels ->
    fp32 (N, C, H, W) / (N, C), (q - zp) * delta."""
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.int8:
        raise A.SSQError("act_decode: expected int8 codes")
    codes = _i8_dev(codes, "act_decode")
    C = int(C)
    if codes.dim() not in (2, 4) or codes.shape[-1] != query("ssq_qinfer_cpad", C):
        raise A.SSQError(f"act_decode: codes {tuple(codes.shape)} do not hold {C} channels")
    N = int(codes.shape[0])
    H, W = (int(codes.shape[1]), int(codes.shape[2])) if codes.dim() == 4 else (1, 1)
    x = torch.empty((N, C, H, W) if codes.dim() == 4 else (N, C), dtype=torch.float32,
                    device=codes.device)
    call("ssq_act_decode", _vp(codes), N, C, H, W, float(delta), float(zp),
         qrange(n_bits, sym)[0], _vp(x), stream_of(x))
    return x


def qconv_codes(codes_or_x, prepared, scale, stride=1, padding=0, groups=1, act_zp=0.0, act_bits=8,
                act_sym=False, act_delta=None, bias=None, gamma=None, phi=None, relu=0,
                out_delta=None, out_zp=0.0, out_bits=8, out_sym=False, bad=None, residual=None,
                splits=None, workspace=None):
    """qconv with the layer's epilogue and output act quantizer applied in the kernel
    (csrc/qinfer_epi.h): returns the int8 codes of clamp(round(act((I * scale + bias) * gamma +
    phi) / out_delta) + out_zp) in act_encode's layout (N, OH, OW, Cpad) -- what act_encode
    derives from the K13 epilogue's output of qconv's.  `relu`: 0 identity, 1 ReLU, 2 ReLU6.
    A NaN result is stored as qmin and ADDED to `bad`, as are the off-grid elements of an fp32
    input; `bad` must be given (a device int32 word).
    `residual` (dense convs only, ssq_qconv_i8_codes_res_fwd): a block tail's residual, added
    between the affine and the activation as the K13 epilogue adds it -- an fp32 tensor of the
    output's (N, Co, OH, OW), or a carried code tensor (`carried`) of that logical shape, which
    enters as the fp32 value act_decode gives it.
    `splits`, `workspace`: as qconv's."""
    if out_delta is None or bad is None:
        raise A.SSQError("qconv_codes: out_delta and bad are required")
    if len(prepared.shape) != 4:
        raise A.SSQError("qconv_codes: conv layers only")
    if (gamma is None) != (phi is None):
        raise A.SSQError("qconv_codes: gamma and phi go together")
    args, keep, (N, Co, OH, OW, _) = _qconv_args(
        "qconv_codes", codes_or_x, prepared, scale, stride, padding, groups, act_zp, act_bits,
        act_sym, act_delta, bad)
    held, vecs = _channel_vecs("qconv_codes", Co, bias, gamma, phi)
    out = torch.empty((N, OH, OW, query("ssq_qinfer_cpad", Co)), dtype=torch.int8,
                      device=keep[0].device)
    olo, ohi = qrange(out_bits, out_sym)
    form, rargs, fn_groups = "codes_fwd", (), groups
    if residual is not None:
        form, fn_groups = "codes_res_fwd", 1
        cc = getattr(residual, "_ssq_codes", None)
        if cc is not None:
            if (residual.dtype != torch.int8 or cc.shape != (N, Co, OH, OW)
                    or tuple(residual.shape) != tuple(out.shape)):
                raise A.SSQError(f"qconv_codes: residual codes {cc.shape} do not match the output "
                                 f"{(N, Co, OH, OW)}")
            res = _i8_dev(residual, "qconv_codes")
            rlo, rhi = qrange(cc.n_bits, cc.sym)
            rargs = (None, _vp(res), cc.delta, cc.zp, rlo, rhi)
        else:
            if residual.dtype != torch.float32 or tuple(residual.shape) != (N, Co, OH, OW):
                raise A.SSQError(f"qconv_codes: residual must be fp32 {(N, Co, OH, OW)} or carried "
                                 f"codes, got {residual.dtype} {tuple(residual.shape)}")
            res, rp = fptr(residual.detach(), "residual")
            rargs = (rp, None, 0.0, 0.0, 0, 0)
    epi = (*vecs, int(relu), float(out_delta), float(out_zp), olo, ohi, _vp(out), _vp(bad), *rargs)
    if splits is not None and int(splits) != 1:
        fn, ws, tail = _qconv_split("qconv_codes", prepared, groups, form, splits, workspace,
                                    keep[0], stride, padding)
        call(fn, *args, *epi, *tail, stream_of(out))
        return out
    call(_qconv_fn(prepared, fn_groups, form), *args, *epi, stream_of(out))
    return out


def epilogue_codes(y, bias, gamma, phi, relu, out_delta, out_zp, out_bits, out_sym, bad):
    """The K13 epilogue of an fp32 conv output y (N, C, H, W) leaving as int8 codes
    (ssq_epilogue_codes_fwd): clamp(round(act((y + bias) * gamma + phi) / out_delta) + out_zp) in
    act_encode's layout (N, H, W, Cpad) -- what act_encode derives from the fp32 epilogue's
    output.  `relu`: 0 identity, 1 ReLU, 2 ReLU6.  A NaN result is stored as qmin and ADDED to
    `bad` (a device int32 word)."""
    if bad is None:
        raise A.SSQError("epilogue_codes: bad is required")
    if (gamma is None) != (phi is None):
        raise A.SSQError("epilogue_codes: gamma and phi go together")
    y, yp = fptr(y, "y")
    if y.dim() != 4:
        raise A.SSQError(f"epilogue_codes: expected (N, C, H, W), got {tuple(y.shape)}")
    N, Cc, H, W = (int(v) for v in y.shape)
    held, vecs = _channel_vecs("epilogue_codes", Cc, bias, gamma, phi, per="channel")
    out = torch.empty((N, H, W, query("ssq_qinfer_cpad", Cc)), dtype=torch.int8, device=y.device)
    olo, ohi = qrange(out_bits, out_sym)
    call("ssq_epilogue_codes_fwd", yp, *vecs, N, Cc, H, W, int(relu),
         float(out_delta), float(out_zp), olo, ohi, _vp(out), _vp(bad), stream_of(out))
    return out


# ------------------------------------------------------------------ K31 fused stem conv
STEM_MAX_CI, STEM_MAX_RS = 4, 7


class StemWeight:
    """A stem weight prepared for K31 (stem_weight_prepare): `blob`, the device bytes;
    `shape`, the weight's (Co, Ci, R, S)."""

    def __init__(self, blob, shape):
        self.blob, self.shape = blob, tuple(int(v) for v in shape)


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def stem_geometry_reason(Co, Ci, R, S, stride, padding, dilation=1, groups=1):
    """Why K31 does not take this conv, None when it does (ssq_stem_conv_fwd's geometry)."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    if groups != 1:
        return "grouped conv"
    if (dh, dw) != (1, 1) or not (1 <= Ci <= STEM_MAX_CI and 1 <= R <= STEM_MAX_RS
                                  and 1 <= S <= STEM_MAX_RS and Co >= 1 and sh >= 1 and sw >= 1
                                  and 0 <= ph < R and 0 <= pw < S):
        return (f"geometry (Ci {Ci}, kernel {R}x{S}, stride {(sh, sw)}, padding {(ph, pw)}, "
                f"dilation {(dh, dw)}: K31 takes Ci <= {STEM_MAX_CI}, R, S <= {STEM_MAX_RS}, "
                "padding below the kernel, dilation 1)")
    return None


def stem_weight_prepare(weight):
    """fp32 OIHW weight (Co, Ci <= 4, R <= 7, S <= 7) -> StemWeight, the operand of stem_conv /
    stem_conv_codes (ssq_stem_weight_prepare; layout: csrc/qinfer_layout.h, SLayout)."""
    w, wp = fptr(weight.detach(), "weight")
    if w.dim() != 4:
        raise A.SSQError(f"stem_weight_prepare: expected (Co, Ci, R, S), got {tuple(w.shape)}")
    Co, Ci, R, S = (int(v) for v in w.shape)
    nbytes = query("ssq_stem_weight_prepared_bytes", Co, Ci, R, S)
    if nbytes == 0:
        raise A.SSQError(f"stem_weight_prepare: weight {tuple(w.shape)} is outside K31's geometry "
                         f"(Ci <= {STEM_MAX_CI}, R, S <= {STEM_MAX_RS})")
    blob = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    call("ssq_stem_weight_prepare", wp, Co, Ci, R, S, _vp(blob), stream_of(blob))
    return StemWeight(blob, w.shape)


def _stem_args(name, x, prepared, stride, padding):
    if not isinstance(prepared, StemWeight):
        raise A.SSQError(f"{name}: prepared must come from stem_weight_prepare")
    x, xp = fptr(x, "x")
    Co, Ci, R, S = prepared.shape
    if x.dim() != 4 or int(x.shape[1]) != Ci:
        raise A.SSQError(f"{name}: expected (N, {Ci}, H, W), got {tuple(x.shape)}")
    N, _, H, W = (int(v) for v in x.shape)
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    OH = (H + 2 * ph - R) // max(sh, 1) + 1
    OW = (W + 2 * pw - S) // max(sw, 1) + 1
    args = (xp, _vp(prepared.blob), prepared.blob.numel(), N, Ci, H, W, Co, R, S, sh, sw, ph, pw)
    return x, args, (N, Co, max(OH, 0), max(OW, 0))


def stem_conv(x, prepared, stride=1, padding=0):
    """K31's fp32 form (ssq_stem_conv_fwd): the conv of an fp32 image x (N, Ci, H, W) with a
    prepared weight as fp32 (N, Co, OH, OW), each output the k-ordered fp32 fma chain over
    (ci, r, s) from +0 (include/ssq.h).  `stride`, `padding`: an int or (h, w)."""
    x, args, (N, Co, OH, OW) = _stem_args("stem_conv", x, prepared, stride, padding)
    y = torch.empty((N, Co, OH, OW), dtype=torch.float32, device=x.device)
    call("ssq_stem_conv_fwd", *args, _vp(y), stream_of(y))
    return y


def stem_conv_codes(x, prepared, bias, gamma, phi, relu, out_delta, out_zp, out_bits, out_sym, bad,
                    stride=1, padding=0):
    """K31's code form (ssq_stem_conv_codes_fwd): epilogue_codes(stem_conv(x, prepared), ...)
    byte for byte in one kernel, without the fp32 tensor.  The epilogue's arguments are
    epilogue_codes'."""
    if bad is None:
        raise A.SSQError("stem_conv_codes: bad is required")
    if (gamma is None) != (phi is None):
        raise A.SSQError("stem_conv_codes: gamma and phi go together")
    x, args, (N, Co, OH, OW) = _stem_args("stem_conv_codes", x, prepared, stride, padding)
    held, vecs = _channel_vecs("stem_conv_codes", Co, bias, gamma, phi)
    out = torch.empty((N, OH, OW, query("ssq_qinfer_cpad", Co)), dtype=torch.int8, device=x.device)
    olo, ohi = qrange(out_bits, out_sym)
    call("ssq_stem_conv_codes_fwd", *args, *vecs, int(relu), float(out_delta), float(out_zp), olo,
         ohi, _vp(out), _vp(bad), stream_of(out))
    return out


# ------------------------------------------------------------------ K32 uint8 stem conv
class StemU8Weight:
    """A stem weight prepared for K32 (stem_u8_weight_prepare): `blob`, the device bytes;
    `shape`, the weight's (Co, Ci, R, S); `bad`, the device word of the zero points that are not
    integer codes."""

    def __init__(self, blob, shape, bad):
        self.blob, self.shape, self.bad = blob, tuple(int(v) for v in shape), bad


def stem_u8_geometry_reason(Co, Ci, R, S, stride, padding, dilation=1, groups=1):
    """Why K32 does not take this conv, None when it does: K31's geometry
    (ssq_stem_conv_u8_fwd's), by its refusals' names -- a grouped stem, Ci > 4, R or S > 7,
    dilation != 1, padding not below the kernel."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    if groups != 1:
        return "grouped conv"
    if not 1 <= Ci <= STEM_MAX_CI:
        return f"Ci = {Ci} exceeds {STEM_MAX_CI}"
    if not (1 <= R <= STEM_MAX_RS and 1 <= S <= STEM_MAX_RS):
        return f"kernel {R}x{S} exceeds {STEM_MAX_RS}x{STEM_MAX_RS}"
    if (dh, dw) != (1, 1):
        return f"dilation {(dh, dw)} != 1"
    if not (0 <= ph < R and 0 <= pw < S):
        return f"padding {(ph, pw)} not below the kernel {R}x{S}"
    if Co < 1 or sh < 1 or sw < 1:
        return f"geometry (Co {Co}, stride {(sh, sw)})"
    return None


def stem_u8_weight_prepare(packed, shape, zp, n_bits, qmin):
    """Packed codes (pack_encode's layout) + zp[co] of a stem weight `shape` = (Co, Ci <= 4,
    R <= 7, S <= 7) -> StemU8Weight, the operand of stem_conv_u8 / stem_conv_u8_codes
    (ssq_stem_u8_weight_prepare; layout: csrc/qinfer_layout.h, ULayout).  Its `bad` counts the
    channels whose zero point is not an integer code, as qweight_prepare's."""
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8:
        raise A.SSQError("stem_u8_weight_prepare: packed codes must be a uint8 tensor")
    packed = _i8_dev(packed, "stem_u8_weight_prepare")
    if len(shape) != 4:
        raise A.SSQError(f"stem_u8_weight_prepare: expected (Co, Ci, R, S), got {tuple(shape)}")
    Co, Ci, R, S = (int(v) for v in shape)
    nbytes = query("ssq_stem_u8_weight_prepared_bytes", Co, Ci, R, S)
    if nbytes == 0:
        raise A.SSQError(f"stem_u8_weight_prepare: weight {tuple(shape)} is outside K32's geometry "
                         f"(Ci <= {STEM_MAX_CI}, R, S <= {STEM_MAX_RS})")
    if packed.numel() < query("ssq_pack_bytes", Co * Ci * R * S, n_bits):
        raise A.SSQError("stem_u8_weight_prepare: packed buffer too small for the shape")
    z, zpp = fptr(zp.detach().reshape(-1), "zero_point")
    if z.numel() != Co:
        raise A.SSQError("stem_u8_weight_prepare: zero point must have one entry per output channel")
    blob = torch.empty(nbytes, dtype=torch.uint8, device=packed.device)
    bad = torch.zeros(1, dtype=torch.int32, device=packed.device)
    call("ssq_stem_u8_weight_prepare", _vp(packed), zpp, Co, Ci, R, S, int(n_bits), int(qmin),
         _vp(blob), _vp(bad), stream_of(packed))
    return StemU8Weight(blob, shape, bad)


def stem_u8_tables(mean, std, scale, Co, Ci):
    """The two fp32 tables of K32 in their stated operation order ("uint8 stem (K32)"):
    M[c] = fp32(255 * mean[c]) and s[co, c] = fp32(fp32(1 / fp32(255 * std[c])) * d[co, c]), from
    the caller's fp32 per-channel `mean`, `std` (Ci entries each) and the weight's scale d, `scale`:
    Co entries (per co) or Co * Ci (per (co, ci)).  Each operation is one fp32 torch operation on
    the scale's device; returns (M [Ci], s [Co, Ci]), contiguous."""
    d = torch.as_tensor(scale).detach().float()
    dev = d.device
    mean = torch.as_tensor(mean, dtype=torch.float32).detach().reshape(-1).to(dev)
    std = torch.as_tensor(std, dtype=torch.float32).detach().reshape(-1).to(dev)
    if mean.numel() != Ci or std.numel() != Ci:
        raise A.SSQError(f"stem_u8_tables: mean and std must have {Ci} entries")
    if d.numel() == Co:
        d = d.reshape(Co, 1).expand(Co, Ci)
    elif d.numel() == Co * Ci:
        d = d.reshape(Co, Ci)
    else:
        raise A.SSQError(f"stem_u8_tables: scale must have {Co} or {Co * Ci} entries")
    c255 = torch.full((1,), 255.0, dtype=torch.float32, device=dev)
    M = (c255 * mean).contiguous()
    inv = torch.ones(1, dtype=torch.float32, device=dev) / (c255 * std)
    return M, (inv.reshape(1, Ci) * d).contiguous()


STEM_U8_FORMS = ("planar", "interleaved", "generic")


def _stem_u8_view(u):
    """(form, byte strides) of the uint8 view `u` (N, Ci, H, W) as K32 stages it, or ("copied",
    None) where the ABI refuses the view (ssq_stem_u8_view_span: a span of 2^31 bytes or more) or
    its span leaves the tensor's storage.  Host only."""
    lo, hi, form = C.c_int64(0), C.c_int64(0), C.c_int(0)
    strides = tuple(int(v) for v in u.stride())
    rc = query("ssq_stem_u8_view_span", *(int(v) for v in u.shape), *strides, C.byref(lo),
               C.byref(hi), C.byref(form))
    off, size = int(u.storage_offset()), int(u.untyped_storage().nbytes())
    if rc != 0 or off + lo.value < 0 or off + hi.value >= size:
        return "copied", None
    return STEM_U8_FORMS[form.value], strides


def stem_u8_view_form(u):
    """How stem_conv_u8 / stem_conv_u8_codes stage the uint8 view `u` (N, Ci, H, W): "planar"
    (unit stride along W: NCHW, planar crops, batch-strided views), "interleaved" (HWC pixels of
    Ci .. 4 bytes, `hwc.permute(0, 3, 1, 2)`), "generic" (any other non-negative strides), each
    read in place, or "copied" (the view is made dense first)."""
    if not isinstance(u, torch.Tensor) or u.dtype != torch.uint8 or u.dim() != 4:
        raise A.SSQError("stem_u8_view_form: expected a 4-D uint8 tensor")
    return _stem_u8_view(u)[0]


def _stem_u8_args(name, u, prepared, M, s, stride, padding, every_tile_border):
    if not isinstance(prepared, StemU8Weight):
        raise A.SSQError(f"{name}: prepared must come from stem_u8_weight_prepare")
    if not isinstance(u, torch.Tensor) or u.dtype != torch.uint8:
        raise A.SSQError(f"{name}: the image must be a uint8 tensor")
    if u.device.type != "cuda":
        raise A.SSQError(f"{name}: ssq kernels run on the MI355X (HIP) device only")
    Co, Ci, R, S = prepared.shape
    if u.dim() != 4 or int(u.shape[1]) != Ci:
        raise A.SSQError(f"{name}: expected (N, {Ci}, H, W), got {tuple(u.shape)}")
    # the view as it stands, through its byte strides; one the ABI refuses is copied dense
    strides = _stem_u8_view(u)[1] if u.numel() else None
    if strides is None:
        u = u.contiguous()
        strides = tuple(int(v) for v in u.stride())
    M, Mp = fptr(M.detach().reshape(-1), "M")
    s, sp = fptr(s.detach().reshape(-1), "s")
    if M.numel() != Ci or s.numel() != Co * Ci:
        raise A.SSQError(f"{name}: M must have {Ci} entries and s {Co} x {Ci} (stem_u8_tables)")
    N, _, H, W = (int(v) for v in u.shape)
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    OH = (H + 2 * ph - R) // max(sh, 1) + 1
    OW = (W + 2 * pw - S) // max(sw, 1) + 1
    args = (_vp(u), _vp(prepared.blob), prepared.blob.numel(), Mp, sp, N, Ci, H, W, Co, R, S, sh,
            sw, ph, pw, *strides, int(bool(every_tile_border)))
    return (u, M, s), args, (N, Co, max(OH, 0), max(OW, 0))


def stem_u8_tiles(prepared, ushape, stride=1, padding=0, codes=True):
    """(interior, border): the workgroups of stem_conv_u8_codes (`codes`; else stem_conv_u8) on an
    image of `ushape` that read B_c from the blob's full-window sums, and those that sum the valid
    taps (ssq_stem_u8_tiles; host only)."""
    Co, Ci, R, S = prepared.shape
    N, _, H, W = (int(v) for v in ushape)
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    inner, border = C.c_int64(0), C.c_int64(0)
    call("ssq_stem_u8_tiles", N, Ci, H, W, Co, R, S, sh, sw, ph, pw, int(bool(codes)),
         C.byref(inner), C.byref(border))
    return int(inner.value), int(border.value)


def stem_conv_u8(u, prepared, M, s, stride=1, padding=0, every_tile_border=False):
    """K32's fp32 form (ssq_stem_conv_u8_strided_fwd): the stem conv of the uint8 image u, any
    (N, Ci, H, W)-shaped view read in place (`stem_u8_view_form`; an HWC batch is
    `hwc.permute(0, 3, 1, 2)`), standing for x = (u/255 - mean)/std, with a prepared weight and the tables of stem_u8_tables,
    as fp32 (N, Co, OH, OW) in the stated operation order (include/ssq.h).  `stride`, `padding`:
    an int or (h, w).  `every_tile_border`: no workgroup takes the interior shortcut (the same
    bits)."""
    keep, args, (N, Co, OH, OW) = _stem_u8_args("stem_conv_u8", u, prepared, M, s, stride, padding,
                                                every_tile_border)
    y = torch.empty((N, Co, OH, OW), dtype=torch.float32, device=keep[0].device)
    call("ssq_stem_conv_u8_strided_fwd", *args, _vp(y), stream_of(y))
    return y


def stem_conv_u8_codes(u, prepared, M, s, bias, gamma, phi, relu, out_delta, out_zp, out_bits,
                       out_sym, bad, stride=1, padding=0, every_tile_border=False):
    """K32's code form (ssq_stem_conv_u8_strided_codes_fwd): epilogue_codes(stem_conv_u8(u, ...), ...) byte
    for byte in one kernel, without the fp32 tensor.  The epilogue's arguments are
    stem_conv_codes'."""
    if bad is None:
        raise A.SSQError("stem_conv_u8_codes: bad is required")
    if (gamma is None) != (phi is None):
        raise A.SSQError("stem_conv_u8_codes: gamma and phi go together")
    keep, args, (N, Co, OH, OW) = _stem_u8_args("stem_conv_u8_codes", u, prepared, M, s, stride,
                                                padding, every_tile_border)
    held, vecs = _channel_vecs("stem_conv_u8_codes", Co, bias, gamma, phi)
    out = torch.empty((N, OH, OW, query("ssq_qinfer_cpad", Co)), dtype=torch.int8,
                      device=keep[0].device)
    olo, ohi = qrange(out_bits, out_sym)
    call("ssq_stem_conv_u8_strided_codes_fwd", *args, *vecs, int(relu), float(out_delta), float(out_zp),
         olo, ohi, _vp(out), _vp(bad), stream_of(out))
    return out


def maxpool_codes(codes, k, stride, padding):
    """Max-pool (ssq_maxpool2d_fwd's geometry) on act_encode's int8 codes (N, H, W, Cpad) ->
    (N, OH, OW, Cpad) (ssq_maxpool_i8_fwd): the codes act_encode derives from the fp32 max-pool
    of the tensor the codes stand for."""
    codes, (N, H, W, Cp) = _nhwc_codes("maxpool_codes", codes)
    k, stride, padding = int(k), int(stride), int(padding)
    OH = (H + 2 * padding - k) // max(stride, 1) + 1
    OW = (W + 2 * padding - k) // max(stride, 1) + 1
    out = torch.empty((N, max(OH, 0), max(OW, 0), Cp), dtype=torch.int8, device=codes.device)
    call("ssq_maxpool_i8_fwd", _vp(codes), N, Cp, H, W, k, stride, padding, _vp(out),
         stream_of(codes))
    return out


# ------------------------------------------------------------------ K29-K30 pooling head on codes
HEAD_MAX_HW = 126   # the pooled plane's H * W: keeps the high digit of a plane sum inside int8


def avgpool_codes(codes):
    """The plane sums of act_encode's int8 codes (N, H, W, Cpad), H * W <= 126
    (ssq_avgpool_i8_digits_fwd): P_s[n, c] = sum_hw code as two int8 digits (N, Cpad),
    hi = (P_s + 64) >> 7 and lo = P_s - 128 * hi in [-64, 63], padded channels 0, and
    sp[n] = sum_c P_s[n, c] (int32) -> (hi, lo, sp)."""
    codes, (N, H, W, Cp) = _nhwc_codes("avgpool_codes", codes)
    digits = torch.empty((2, N, Cp), dtype=torch.int8, device=codes.device)
    sp = torch.empty((N,), dtype=torch.int32, device=codes.device)
    call("ssq_avgpool_i8_digits_fwd", _vp(codes), N, Cp, H, W, _vp(digits[0]), _vp(digits[1]),
         _vp(sp), stream_of(codes))
    return digits[0], digits[1], sp


def head_scale(scale, HW):
    """K30's scale_h[co] = fp32(scale[co] / fp32(HW)) from a layer's s[co] = fp32(delta_a *
    d1[co]): the mean's 1 / HW folded into the scale by one correctly rounded fp32 division
    (made on the host; one copy each way)."""
    import numpy as np
    s = scale.detach().reshape(-1).float().cpu().numpy()
    return torch.from_numpy((s / np.float32(int(HW))).astype(np.float32)).to(scale.device)


def qlinear_pooled(hi, lo, sp, prepared, scale_h, HW, act_zp=0.0, act_bits=8, act_sym=False,
                   wide_all=False):
    """The fc on avgpool_codes's digits (ssq_qlinear_pooled_fwd): y[n, co] = fp32(I) *
    scale_h[co] (fp32 (N, Co)), I = sum_c P[n, c] (q_w[co, c] - z_w[co]) the exact integer with
    P[n, c] = sum_hw (q_a - z_a) over the HW pooled pixels.  `prepared`: the Linear's
    qweight_prepare output; `scale_h`: head_scale(s, HW); (act_zp, act_bits, act_sym): the
    pooled codes' act quantizer.  No bias.  A scaled Linear's centred int8 blob runs as it stands
    with scale_h = head_scale(s, L * HW); `wide_all`: its dense wide blob too
    (ssq_qlinear_pooled_wide_fwd), refused otherwise."""
    for t, nm in ((hi, "hi"), (lo, "lo")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int8:
            raise A.SSQError(f"qlinear_pooled: {nm} must be int8 digits")
    if not isinstance(sp, torch.Tensor) or sp.dtype != torch.int32:
        raise A.SSQError("qlinear_pooled: sp must be an int32 tensor")
    hi, lo, sp = (_i8_dev(t, "qlinear_pooled") for t in (hi, lo, sp))
    if len(prepared.shape) != 2 or getattr(prepared, "groups", 1) != 1:
        raise A.SSQError("qlinear_pooled: the weight must be a prepared Linear")
    wide = bool(getattr(prepared, "wide", False))
    if wide and not wide_all:
        raise A.SSQError("qlinear_pooled: a wide blob is not K30's operand (the pooled-operand fc "
                         "reads one int8 weight plane)")
    Co, Ci, _, _ = prepared.geometry()
    Cp = query("ssq_qinfer_cpad", Ci)
    if hi.dim() != 2 or hi.shape[1] != Cp or tuple(lo.shape) != tuple(hi.shape):
        raise A.SSQError(f"qlinear_pooled: digits {tuple(hi.shape)}, {tuple(lo.shape)} do not "
                         f"match the weight {prepared.shape} (Cpad = {Cp})")
    N = int(hi.shape[0])
    if sp.dim() != 1 or sp.numel() != N:
        raise A.SSQError("qlinear_pooled: sp must have one entry per image")
    s, shp = fptr(scale_h.detach().reshape(-1), "scale_h")
    if s.numel() != Co:
        raise A.SSQError("qlinear_pooled: scale_h must have one entry per output channel")
    alo, ahi = qrange(act_bits, act_sym)
    y = torch.empty((N, Co), dtype=torch.float32, device=hi.device)
    call("ssq_qlinear_pooled_wide_fwd" if wide else "ssq_qlinear_pooled_fwd", _vp(hi), _vp(lo),
         _vp(sp), _vp(prepared.blob), shp, N, Ci, Co,
         int(HW), float(act_zp), alo, ahi, _vp(y), stream_of(y))
    return y


def qlinear_pooled_tile(tile=0):
    """Measurement plumbing: set K30's image tile (16, the default, or 64); returns the previous
    one (any other value only queries)."""
    return query("ssq_qlinear_pooled_set_tile", int(tile))


class PooledCodes(_Quantized):
    """What a pooled digit tensor stands for (the hi tensor's `_ssq_pooled`): the lo digits and
    the per-image sums that go with it, the logical (N, C), the HW pixels that were summed and
    the act quantizer (delta, zp, n_bits, sym) of the pooled codes.  Only the planned fc reads
    it; it stands for no fp32 tensor, so materialize_epi refuses it."""

    def __init__(self, lo, sp, shape, HW, delta, zp, n_bits, sym):
        self.lo, self.sp = lo, sp
        self.shape, self.HW = tuple(int(v) for v in shape), int(HW)
        self.q = q = tuple.__new__(ActQuant, (float(delta), float(zp), int(n_bits), bool(sym)))
        self.delta, self.zp, self.n_bits, self.sym = q


def pooled(hi, lo, sp, shape, HW, delta, zp, n_bits, sym):
    """`hi` tagged as a pooled digit tensor (see PooledCodes)."""
    hi._ssq_pooled = PooledCodes(lo, sp, shape, HW, delta, zp, n_bits, sym)
    return hi


# ------------------------------------------------------------------ conv geometry
# The numbers of one F.conv2d call, parsed once (conv_geometry).  single: the input and the
# weight are 4-D and stride and padding each stand for one integer.  A tuple with unequal
# entries or a string padding does not: every other field but dil and groups is then 0 and no
# kernel of this file takes the conv.  dil: the one dilation, 0 for unequal entries.
ConvGeo = collections.namedtuple("ConvGeo", "Nb C H W Co Cig R S st pad dil groups OH OW single")


def _one(v):
    """The integer an int-or-tuple argument of F.conv2d stands for; None for a string or a
    tuple with unequal entries.  The one place that unpacks such an argument."""
    if isinstance(v, int):
        return v
    return None if isinstance(v, str) or len(set(v)) != 1 else int(v[0])


def conv_geometry(x_shape, w_shape, stride, padding, dilation=1, groups=1):
    """ConvGeo of F.conv2d(x, w, None, stride, padding, dilation, groups); a layer asks for the
    same one every iteration, so the hashable argument forms are remembered."""
    try:
        return _geometry(x_shape, w_shape, stride, padding, dilation, groups)
    except TypeError:                                   # a list among the arguments
        return _geometry.__wrapped__(x_shape, w_shape, stride, padding, dilation, groups)


@functools.lru_cache(maxsize=1024)
def _geometry(x_shape, w_shape, stride, padding, dilation, groups):
    st, pad, dil = _one(stride), _one(padding), _one(dilation) or 0
    if len(x_shape) != 4 or len(w_shape) != 4 or st is None or pad is None:
        return ConvGeo(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, dil, groups, 0, 0, False)
    Nb, C, H, W = x_shape
    Co, Cig, R, S = w_shape
    return ConvGeo(Nb, C, H, W, Co, Cig, R, S, st, pad, dil, groups,
                   (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1, True)


def _k17_dims(g):
    """The ten shape arguments of ssq_conv_wgrad and of its planner queries."""
    return g.Nb, g.C, g.H, g.W, g.Co, g.R, g.S, g.st, g.pad, g.groups


def _dev_f32(x):
    return x.is_cuda and x.dtype == torch.float32


# ------------------------------------------------------------------ K17 conv weight gradient
def conv_wgrad_supported(x, weight, stride, padding, dilation, groups, geo=None):
    """Shapes ssq_conv_wgrad handles: 4-D fp32 NCHW on the device, square stride /
    padding, dilation 1, and a plan whose LDS tile fits (nonzero workspace size)."""
    g = geo or conv_geometry(x.shape, weight.shape, stride, padding, dilation, groups)
    return (g.single and g.dil == 1 and _dev_f32(x)
            and query("ssq_conv_wgrad_workspace_size", *_k17_dims(g)) > 0)


def wgrad_kind(x_shape, w_shape, stride, padding, groups, geo=None):
    """The K17 kernel ssq_conv_wgrad runs for this shape (0 unsupported, 1 row tile,
    2 im2col-DMA, 3 band with 16-B staging, 4 1x1 GEMM, 5 depthwise, 6 band with 4-B
    staging)."""
    g = geo or conv_geometry(x_shape, w_shape, stride, padding, 1, groups)
    return int(query("ssq_conv_wgrad_kind", *_k17_dims(g))) if g.single else 0


def set_wgrad_form(form):
    """K17 non-depthwise form: 0 auto, 1 input-row-tile (+1x1 GEMM), 2 im2col-DMA, 3 band
    (3x3 pad 1 shapes, Cin / Cout multiples of 32, else the row tile), 4 band at 4 waves per
    workgroup (one per SIMD; 3 runs 8); returns the previous value."""
    return int(query("ssq_conv_wgrad_set_form", int(form)))


def conv_wgrad(x, dy, w_shape, stride, padding, groups):
    """d loss / d weight of F.conv2d(x, w, stride, padding, groups) given dy (K17)."""
    dims = _k17_dims(conv_geometry(x.shape, w_shape, stride, padding, 1, groups))
    x, xp = fptr(x.detach(), "x")
    dy, dp = fptr(dy.detach(), "dy")
    ws, wsn = workspace(query("ssq_conv_wgrad_workspace_size", *dims), x.device)
    dw = torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
    call("ssq_conv_wgrad", xp, dp, *dims, _vp(dw), ws, wsn, stream_of(x))
    return dw


def gemm_operands(x, dy, w_shape, stride, padding, want_col=True, want_dy2=True):
    """ssq_wgrad_gemm_operands: the im2col matrix col (N*P x C*R*S) of x and/or the
    permuted gradient dy2 (Co x N*P), in one launch."""
    g = conv_geometry(x.shape, w_shape, stride, padding)
    NP, dev_ = g.Nb * g.OH * g.OW, x.device
    col = torch.empty(NP, g.C * g.R * g.S, dtype=torch.float32, device=dev_) if want_col else None
    dy2 = torch.empty(g.Co, NP, dtype=torch.float32, device=dev_) if want_dy2 else None
    # (the contiguous tensors are held to the launch: a copy made here must not be freed
    # and its block reused by the next one before the kernel has read it)
    xt, xp = fptr(x.detach(), "x") if want_col else (None, None)
    dt, dp = fptr(dy.detach(), "dy") if want_dy2 else (None, None)
    call("ssq_wgrad_gemm_operands", xp, dp, g.Nb, g.C, g.H, g.W, g.Co, g.R, g.S, g.st, g.pad,
         _vp(col), _vp(dy2), stream_of(col if want_col else dy2))
    return col, dy2


def conv_wgrad_gemm(x, dy, w_shape, stride, padding, col=None):
    """The conv weight gradient as ONE fp32 library GEMM: dw = dy2 @ col
    (torch.matmul -> hipBLASLt; one kernel per shape, bit-identical run to run), the
    operands from ssq_wgrad_gemm_operands (col may be the forward's, saved).  Ungrouped
    convs.  Faster than the band kernel on small output planes."""
    c2, dy2 = gemm_operands(x, dy, w_shape, stride, padding, want_col=col is None, want_dy2=True)
    col = c2 if col is None else col
    return torch.matmul(dy2, col).view(tuple(w_shape))


def conv_fwd_gemm(x, weight, stride, padding):
    """F.conv2d (no bias, ungrouped) as one fp32 strided-batched library GEMM over the
    im2col matrix, y[n] = W[Co, C*R*S] @ col_n^T (col_n: sample n's P rows), written in
    NCHW directly.  Bit-identical to the one-GEMM y2 = W @ col^T + permute form it replaced
    and 1-4 us faster per ResNet-18 layer3/4 conv (tools/fwd_gemm_layout_probe.py,
    profiles/r3_fwd_gemm_layout.json).  Returns (y, col); col serves the weight gradient."""
    g = conv_geometry(x.shape, weight.shape, stride, padding)
    col, _ = gemm_operands(x, None, weight.shape, stride, padding, want_col=True, want_dy2=False)
    crs = g.C * g.R * g.S
    y = torch.matmul(weight.detach().reshape(g.Co, crs),
                     col.view(g.Nb, g.OH * g.OW, crs).transpose(1, 2))
    return y.view(g.Nb, g.Co, g.OH, g.OW), col


# ------------------------------------------------------------------ K18 depthwise conv
def dwconv_supported(x, weight, stride, padding, dilation, groups, geo=None):
    """Depthwise shapes K18 handles: fp32 NCHW on the device, groups == C == Co, square
    stride / padding, dilation 1, R*S <= 25, and forward AND input-gradient LDS stages
    (weight rows + padded planes) within the 128 KiB opt-in (ssq_dwconv_supported)."""
    g = geo or conv_geometry(x.shape, weight.shape, stride, padding, dilation, groups)
    if not g.single or g.dil != 1 or not _dev_f32(x):
        return False
    if groups <= 1 or groups != g.C or groups != g.Co or g.Cig != 1:
        return False
    # both the forward and the input-gradient stage must fit (the planner's own sizes)
    return g.R * g.S <= 25 and bool(query("ssq_dwconv_supported", *_dw_dims(g)))


def _dw_dims(g):
    """The eight shape arguments of the K18 launches and their planner query."""
    return g.Nb, g.C, g.H, g.W, g.R, g.S, g.st, g.pad


def dwconv_fwd(x, weight, stride, padding):
    g = conv_geometry(x.shape, weight.shape, stride, padding)
    x, xp = fptr(x.detach(), "x")
    w, wp = fptr(weight.detach(), "weight")
    y = torch.empty((g.Nb, g.C, g.OH, g.OW), dtype=torch.float32, device=x.device)
    call("ssq_dwconv_fwd", xp, wp, _vp(y), *_dw_dims(g), stream_of(x))
    return y


def dwconv_bwd_data(dy, weight, x_shape, stride, padding):
    g = conv_geometry(x_shape, weight.shape, stride, padding)
    dy, dp = fptr(dy.detach(), "dy")
    w, wp = fptr(weight.detach(), "weight")
    dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=dy.device)
    call("ssq_dwconv_bwd_data", dp, wp, _vp(dx), *_dw_dims(g), stream_of(dy))
    return dx


class DwConv2dFn(torch.autograd.Function):
    """Depthwise F.conv2d on K18 (forward, input gradient) and K17's depthwise reduction
    (weight gradient): deterministic, no MIOpen naive kernels."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding):
        ctx.save_for_backward(x, weight)
        ctx.cfg = (stride, padding)
        return dwconv_fwd(x, weight, stride, padding)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        stride, padding = ctx.cfg
        g = g.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = dwconv_bwd_data(g, weight, x.shape, stride, padding)
        if ctx.needs_input_grad[1]:
            gw = conv_wgrad(x, g, weight.shape, stride, padding, int(weight.shape[0]))
        return gx, gw, None, None


def _pair(v):
    """An int or (h, w) argument of F.conv2d as [h, w]; None for a string padding ('same' /
    'valid'): no rule takes such a conv (ConvGeo.single), so none reaches the
    aten.convolution_backward calls, which take this form."""
    if isinstance(v, str):
        return None
    return [int(v), int(v)] if isinstance(v, int) else [int(t) for t in v]


class Conv2dFn(torch.autograd.Function):
    """F.conv2d whose weight gradient runs on K17 (deterministic, MFMA) or a library GEMM
    form; the forward and the input gradient stay on MIOpen except where a GEMM form is
    faster (small-plane im2col forwards, 1x1 stride-2 forwards, 1x1 stride-1 input gradients)."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding, dilation, groups, route):
        """route: conv_route's answer for this call; the backward runs what it names.  kept:
        the forward's im2col matrix (im2col_gemm, grouped_gemm) or its subsampled input
        (gemm_1x1, where the weight gradient is bmm_s2)."""
        ctx.cfg, ctx.route, kept = (stride, padding, dilation, groups), route, None
        if route.fwd == "im2col_gemm":
            y, kept = conv_fwd_gemm(x, weight, stride, padding)
        elif route.fwd == "grouped_gemm":
            y, kept = conv_fwd_grouped_gemm(x, weight, stride, padding, groups)
        elif route.fwd == "gemm_1x1":
            y, xs = conv1x1_fwd_gemm(x, weight, stride, keep_xs=True)
            kept = xs if route.dw == "bmm_s2" else None
        else:
            y = torch.nn.functional.conv2d(x, weight, None, stride, padding, dilation, groups)
        ctx.save_for_backward(x, weight, kept)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, kept = ctx.saved_tensors
        stride, padding, dilation, groups = ctx.cfg
        route, need = ctx.route, ctx.needs_input_grad
        g = g.contiguous()
        gx = gw = None

        def lib(which):
            # the saved input itself, not torch.nn.grad.conv2d_input's expanded dummy: the
            # MIOpen backend makes an expanded input contiguous first (one activation-sized
            # copy per call, 8.4 us on a ResNet-18 layer1 batch)
            return torch.ops.aten.convolution_backward(
                g, x, weight, None, _pair(stride), _pair(padding), _pair(dilation), False,
                [0, 0], groups, tuple(i == which for i in range(3)))[which]
        if need[0]:
            gx = conv1x1_dgrad_gemm(g, weight) if route.dx == "gemm_1x1" else lib(0)
        if need[1] and route.dw == "im2col_gemm":
            gw = conv_wgrad_gemm(x, g, weight.shape, stride, padding, col=kept)
        elif need[1] and route.dw == "bmm_1x1":
            gw = conv_wgrad_1x1_bmm(x, g, weight.shape)
        elif need[1] and route.dw == "bmm_s2":
            gw = conv_wgrad_1x1_bmm(kept, g, weight.shape)
        elif need[1] and route.dw == "grouped_gemm":
            gw = conv_wgrad_grouped_gemm(x, g, weight.shape, stride, padding, groups, col=kept)
        elif need[1]:
            gw = conv_wgrad(x, g, weight.shape, stride, padding, groups) if route.dw == "k17" \
                else lib(1)
        return gx, gw, None, None, None, None, None


# When the conv weight gradient runs on K17 (tools/wgrad_bench.py, batch 32, MI355X,
# profiles/r2_wgrad_band.log):
#   'auto'   every shape the band kernel stages with 16-B pieces (3x3 pad 1: ResNet layer1,
#            layer2, layer3.0's stride-2 conv), in either mode -- it beats MIOpen's fastest
#            non-deterministic solver there (layer1 3x3: 97 vs 110 us, layer2.0 s2: 66 vs
#            81, layer3.0 s2: 66 vs 85); every grouped conv: depthwise ones on K17's
#            LDS-staged reduction (MobileNetV2 144x56x56 3x3: 60 vs 866 us on MIOpen, either
#            mode), other grouped ones on its MFMA GEMM (RegNetX g=2: 326 vs 960 us); under
#            the reference's torch.backends.cudnn.deterministic also every stride-2 conv and
#            every output plane >= 100 pixels, where MIOpen's deterministic solvers are
#            slower (layer3 3x3 14x14: band 132 vs 172 us, layer4.0 s2: 106 vs 372; the
#            7x7 planes of layer4 stay on MIOpen: 98 vs 166).
#   'always' / 'never' (MIOpen's choice) for A/B runs.
WGRAD_POLICY = "auto"


# Conv weight gradients as ONE library GEMM over an im2col matrix (conv_wgrad_gemm) where
# the output plane is small: 3x3 (or larger) ungrouped convs with OH*OW <= 196,
# Co >= 128 and C*R*S >= 1152 -- ResNet-18 layer3 / layer4 (tools/gemm_probe.py,
# profiles/r2_wgrad_gemm.log: the GEMM runs at 94-115 TF there, the band kernel at 57 TF
# on 14x14 planes).  'never' keeps K17 / MIOpen (A/B).
WGRAD_GEMM = "auto"


# The rules conv_route consults, each at most once per call.  Called on their own they parse
# the arguments themselves; conv_route hands them its ConvGeo (geo).
def _use_wgrad_gemm(x, weight, stride, padding, groups=1, geo=None):
    # WGRAD_POLICY 'never' is the all-MIOpen A/B mode: no GEMM convs either
    g = geo or conv_geometry(x.shape, weight.shape, stride, padding, 1, groups)
    if WGRAD_GEMM != "auto" or WGRAD_POLICY == "never" or groups != 1 or not g.single:
        return False
    NP, crs = g.Nb * g.OH * g.OW, g.Cig * g.R * g.S
    if NP * crs >= (1 << 31) or g.Co * NP >= (1 << 31) or g.OH * g.OW > 196:
        return False
    if g.R * g.S == 1:
        # 1x1 (the ResNet downsamples): layer3.0 / layer4.0 33 / 23 us vs K17's 1x1 kernel
        # 44 / 44; layer2.0's (28x28 plane) stays on K17 (84 vs 42; tools/ds_gemm_probe.py).
        # Under cudnn.deterministic also every 1x1 on a 7x7 plane: MIOpen's deterministic
        # weight gradient takes 74-137 us there (MobileNetV2 960 -> 160: GEMM 25, K17 45;
        # tools/conv1x1_probe.py, profiles/r6_conv1x1_probe.jsonl)
        return g.Co >= 256 or (g.OH * g.OW <= 49 and torch.backends.cudnn.deterministic)
    return g.Co >= 128 and crs >= 1152


# 1x1 stride-1 convs on large planes (OH*OW >= 400: ResNet-50's bottleneck 1x1s and layer1
# downsample, MobileNetV2's expand / project convs, RegNetX's 'a' convs on 28x28 and up): the
# weight gradient as ONE strided-batched library GEMM, sum_n dy[n] @ x[n]^T, then the batch
# summed in order (conv_wgrad_1x1_bmm), instead of K17's 1x1 kernel, whose per-lane 4-B
# LDS-DMA staging holds it at 11-31 TF there.  tools/wgrad1x1_probe.py
# (profiles/r6_wgrad1x1_probe.jsonl), batch 32: ResNet-50 layer1.0 conv1 / conv3 / downsample
# 74.6 / 120.8 / 120.9 -> 20.9 / 35.3 / 35.0 us, RegNetX-3200M s3.b1 'a' 133.7 -> 54.3 us;
# bit-identical run to run, within 1e-6 of float64 (K17: 3e-7).  Planes <= 196 pixels keep
# the im2col GEMM (_use_wgrad_gemm) or K17.
def _use_wgrad_bmm(x, weight, stride, padding, groups=1, geo=None):
    g = geo or conv_geometry(x.shape, weight.shape, stride, padding, 1, groups)
    if WGRAD_POLICY != "auto" or groups != 1 or (g.R, g.S, g.st, g.pad) != (1, 1, 1, 0):
        return False
    # 14x14 planes too under cudnn.deterministic (MobileNetV2's 14x14 1x1s: 16-27 us vs K17's
    # 39-44; tools/conv1x1_probe.py) where the im2col GEMM does not take them
    p = g.H * g.W
    return p >= 400 or (p >= 100 and torch.backends.cudnn.deterministic)


# The input gradient of 1x1 stride-1 convs as ONE strided-batched library GEMM,
# dx[n] = W^T @ dy[n] (conv1x1_dgrad_gemm), on the shapes where MIOpen's deterministic
# backward-data solver is slower (tools/conv1x1_probe.py over every 1x1 stride-1 conv of
# ResNet-50 / MobileNetV2 / RegNetX-3200M at batch 32, profiles/r6_conv1x1_probe.jsonl):
#   112x112 planes, all (MobileNetV2 16 -> 96: 110 -> 38 us);
#   7x7 planes with Co <= 4 C (ResNet-50 512 -> 2048: 157 -> 37; MobileNetV2 960 -> 160:
#       15.1 -> 12.5; 160 -> 960 is slower as a GEMM, 16.5 -> 41.6);
#   14x14 / 28x28 planes with C >= 128 and Co >= C, and Co >= 2 C on 14x14 (ResNet-50
#       256 -> 1024: 53 -> 35; RegNetX 192 -> 432: 103 -> 51; 432 -> 432 on 14x14 is not);
#   56x56 planes never (the GEMM is 1.3-2.5x slower there).
def _use_dgrad_1x1(x, weight, stride, padding, groups=1, geo=None):
    g = geo or conv_geometry(x.shape, weight.shape, stride, padding, 1, groups)
    if WGRAD_POLICY == "never" or groups != 1 or not torch.backends.cudnn.deterministic:
        return False
    if (g.R, g.S, g.st, g.pad) != (1, 1, 1, 0) or not _dev_f32(x):
        return False
    co, c, p = g.Co, g.Cig, g.H * g.W
    if p >= 12544:
        return True
    if p <= 49:
        return co <= 4 * c
    if 196 <= p <= 784:
        return c >= 128 and co >= c and (p >= 784 or co >= 2 * c)
    return False


def conv1x1_dgrad_gemm(dy, weight):
    """d loss / d input of a 1x1 / stride 1 / pad 0 ungrouped conv: W^T @ dy[n] for every
    sample as one strided-batched GEMM (torch.matmul -> hipBLASLt)."""
    n, co, h, w = (int(v) for v in dy.shape)
    c = int(weight.shape[1])
    gx = torch.matmul(weight.detach().reshape(co, c).t(), dy.reshape(n, co, h * w))
    return gx.view(n, c, h, w)


def conv_wgrad_1x1_bmm(x, dy, w_shape):
    """d loss / d weight of a 1x1 / stride 1 / pad 0 ungrouped conv: sum_n dy[n] @ x[n]^T as
    one strided-batched GEMM (torch.matmul -> hipBLASLt) and an in-order batch sum."""
    n, c = int(x.shape[0]), int(x.shape[1])
    co, p = int(w_shape[0]), int(x.shape[2] * x.shape[3])
    gw = torch.matmul(dy.detach().reshape(n, co, p), x.detach().reshape(n, c, p).transpose(1, 2))
    return gw.sum(0).view(tuple(w_shape))


# Grouped (not depthwise) convs on small output planes (OH*OW <= 196: RegNetX-3200M's g = 9 /
# 21 'b' convs of stages 3 and 4): the weight gradient as the im2col operands of every channel
# (ssq_wgrad_gemm_operands) and ONE strided-batched library GEMM over the groups,
# dW[g] = dy2[g rows] @ col[:, g columns] (conv_wgrad_grouped_gemm), instead of K17's implicit
# GEMM, which runs at 6-11 TF there.  tools/wgrad_grouped_probe.py
# (profiles/r6_wgrad_grouped_probe.jsonl), batch 32: s3.b1 268.6 -> 115.5 us, s3.b2 205.4 ->
# 91.0, s4.b1 243.9 -> 70.3, s4.b2 121.7 -> 57.6; on the larger planes of stages 1-2 (g = 2,
# 4) K17 stays faster and keeps them.  Bit-identical run to run, within 1e-6 of float64.
# ... and the forward of those convs as one GEMM over the groups on the same im2col matrix,
# built once, in the forward (conv_fwd_grouped_gemm).
def _use_wgrad_grouped_gemm(x, weight, stride, padding, groups=1, geo=None):
    g = geo or conv_geometry(x.shape, weight.shape, stride, padding, 1, groups)
    if WGRAD_POLICY != "auto" or groups <= 1 or g.Cig <= 1:
        return False
    NP = g.Nb * g.OH * g.OW
    if NP * g.Cig * groups * g.R * g.S >= (1 << 31) or g.Co * NP >= (1 << 31):
        return False
    return g.OH * g.OW <= 196


def conv_wgrad_grouped_gemm(x, dy, w_shape, stride, padding, groups, col=None):
    """d loss / d weight of a grouped conv: the im2col matrix of every input channel and the
    permuted gradient (ssq_wgrad_gemm_operands, as for an ungrouped conv of C_in = Cig * G),
    then one strided-batched GEMM over the groups (group g: its Cog rows of dy2 against its
    Cig * R * S columns of col).  col may be the forward's (conv_fwd_grouped_gemm), saved."""
    Co, Cig, R, S = (int(v) for v in w_shape)
    c2, dy2 = gemm_operands(x, dy, (Co, Cig * groups, R, S), stride, padding,
                            want_col=col is None, want_dy2=True)
    col = c2 if col is None else col
    NP = col.shape[0]
    a = dy2.view(groups, Co // groups, NP)
    b = col.view(NP, groups, Cig * R * S).transpose(0, 1)
    return torch.matmul(a, b).reshape(tuple(w_shape))


def conv_fwd_grouped_gemm(x, weight, stride, padding, groups):
    """F.conv2d of a grouped conv (no bias) on _use_wgrad_grouped_gemm's shapes as the im2col
    matrix of every input channel (the one its weight gradient reads: returned, to be saved)
    and ONE strided-batched GEMM over the groups, Y[g] = W[g] @ col[:, g]^T (G x Cog x N*P),
    then permuted to NCHW.  RegNetX-3200M s3.b1's 'b' conv (g = 9, stride 2): MIOpen's
    deterministic forward 102.5 us; here the im2col build moves from the backward to the
    forward (tools/recon_configs_trace.py).  Returns (y, col)."""
    g = conv_geometry(x.shape, weight.shape, stride, padding, 1, groups)
    k = g.Cig * g.R * g.S
    col, _ = gemm_operands(x, None, (g.Co, g.Cig * groups, g.R, g.S), stride, padding,
                           want_col=True, want_dy2=False)
    y = torch.matmul(weight.detach().reshape(groups, g.Co // groups, k),
                     col.view(-1, groups, k).permute(1, 2, 0))
    y = y.view(groups, g.Co // groups, g.Nb, g.OH * g.OW).permute(2, 0, 1, 3).contiguous()
    return y.view(g.Nb, g.Co, g.OH, g.OW), col


def _use_fwd_gemm(x, weight, stride, padding, groups=1):
    """The forward as the im2col GEMM on the weight-gradient GEMM's 3x3 (or larger) shapes:
    MIOpen's deterministic forward takes 99 / 173 us on layer3.0 / layer4.0's stride-2 convs
    where the GEMM takes 42 / 38 (profiles/r2_wgrad_gemm.log), and the im2col matrix is then
    shared with the weight gradient.  Extending it to layer2.0's stride-2 conv (MIOpen's
    deterministic forward 99 us standalone, the GEMM 40 + the 58 MB im2col pass) measured no
    gain in the loop (1639 -> 1617 it/s, profiles/r2_wgrad_gemm.log), so it is not.
    conv_route, which has _use_wgrad_gemm's answer already, applies the kernel-size test to
    it instead of calling this."""
    return (weight.shape[2] * weight.shape[3] > 1
            and _use_wgrad_gemm(x, weight, stride, padding, groups))


# 1x1 stride-2 convs (the ResNet downsamples) forward as ONE strided-batched library GEMM
# on the subsampled input, y[n] = W @ x[n, :, ::s, ::s]: NCHW in, NCHW out (MIOpen
# transposes NCHW <-> CNHW around its own GEMM).  tools/ds_fwd_probe.py
# (profiles/r3_ds_fwd_probe.json), deterministic solvers: layer2.0 35.9 -> 22.3 us and
# layer4.0 30.9 -> 14.4 at batch 32 (recon), 112 -> 66 and 103 -> 34 at batch 128
# (validation); layer3.0's 14x14 plane is slower at batch 32 (27.5 -> 56.6, hipBLASLt's
# pick for that batched shape), so output planes of 100-400 pixels stay on MIOpen below
# batch 128.  Bit-identical run to run.  Stride-1 1x1 convs stay on MIOpen (unmeasured).
# A/B knob: SSQ_FWD_1X1_GEMM=0.
FWD_1X1_GEMM = os.environ.get("SSQ_FWD_1X1_GEMM", "1") != "0"


def _use_fwd_1x1(x, weight, stride, padding, dilation, groups, geo=None):
    # WGRAD_POLICY 'never' is the all-MIOpen A/B mode: no GEMM convs there either
    g = geo or conv_geometry(x.shape, weight.shape, stride, padding, dilation, groups)
    if not FWD_1X1_GEMM or WGRAD_POLICY == "never" or groups != 1 or not _dev_f32(x):
        return False
    if (g.R, g.S, g.pad, g.dil) != (1, 1, 0, 1) or g.st < 2:
        return False
    return not (100 < g.OH * g.OW < 400 and g.Nb < 128)


def conv1x1_fwd_gemm(x, weight, stride, keep_xs=False):
    """F.conv2d of a 1x1 / pad 0 / stride s conv as one strided-batched GEMM on the
    subsampled input (see FWD_1X1_GEMM); keep_xs: also return that input, contiguous (the
    weight gradient's operand, conv_wgrad_1x1_bmm)."""
    st = conv_geometry(x.shape, weight.shape, stride, 0).st
    xs = x[:, :, ::st, ::st].contiguous()
    n, c, oh, ow = xs.shape
    co = int(weight.shape[0])
    y = torch.matmul(weight.detach().reshape(co, c), xs.view(n, c, oh * ow))
    y = y.view(n, co, oh, ow)
    return (y, xs) if keep_xs else y


# 1x1 stride-2 weight gradients on output planes >= 400 pixels (the forward GEMM above made
# the subsampled input contiguous) with channel counts in whole 64s: one strided-batched GEMM
# + batch sum over that input (conv_wgrad_1x1_bmm) instead of K17's 1x1 kernel.
# tools/ds_wgrad_probe.py (profiles/r6_ds_wgrad_probe.jsonl), batch 32: ResNet-18 layer2.0
# 41.1 -> 31.6 us, ResNet-50 layer2.0 138.9 -> 65.3; RegNetX s2.b1 (96 -> 192) is slower as
# the GEMM (79.3 vs 43.6) and keeps K17; on 14x14 and 7x7 planes the im2col GEMM stays.
def _use_wgrad_bmm_s2(x, weight, stride, padding, groups=1, geo=None):
    g = geo or conv_geometry(x.shape, weight.shape, stride, padding, 1, groups)
    if WGRAD_POLICY != "auto" or groups != 1 or (g.R, g.S, g.pad) != (1, 1, 0) or g.st < 2:
        return False
    return g.OH * g.OW >= 400 and g.Cig % 64 == 0 and g.Co % 64 == 0


# ------------------------------------------------------------------ the conv router
# What one conv2d call runs: the forward, the input gradient and the weight gradient kernel
# (None: not needed), decided once by conv_route and carried to the backward.
#   fwd  lib (MIOpen) | k18 | im2col_gemm | grouped_gemm | gemm_1x1 | epi_gemm
#   dx   lib | k18 | gemm_1x1 | None
#   dw   lib | k17 | im2col_gemm | bmm_1x1 | bmm_s2 | grouped_gemm | None
ConvRoute = collections.namedtuple("ConvRoute", "geo fwd dx dw")


def conv_route(x, weight, stride, padding, dilation, groups, need_dx, need_dw):
    """The ConvRoute of conv2d(x, weight, stride, padding, dilation, groups) when the input /
    the weight needs a gradient: a function of shapes, device, dtype, contiguity, WGRAD_POLICY,
    WGRAD_GEMM, FWD_1X1_GEMM and cudnn.deterministic.  Launches and allocates nothing.  The
    rules' order of precedence is the order of this function."""
    g = conv_geometry(x.shape, weight.shape, stride, padding, dilation, groups)
    a = (x, weight, stride, padding)
    ours = need_dw and g.dil == 1       # K17 and the GEMM weight gradients: dilation 1 only
    gemm = ours and _use_wgrad_gemm(*a, groups, g)
    if getattr(x, "_ssq_epi", None) is not None and gemm and g.R * g.S > 1:
        # a LazyEpi input (a BasicBlock's conv1 epilogue) on _use_fwd_gemm's shapes: folded
        # into the im2col build (EpiConvGemmFn); any other route materialises it
        return ConvRoute(g, "epi_gemm", "lib" if need_dx else None, "im2col_gemm")
    # depthwise convs on K18 + K17 (MIOpen runs them on naive direct kernels)
    if groups > 1 and dwconv_supported(*a, dilation, groups, g) and x.is_contiguous():
        return ConvRoute(g, "k18", "k18" if need_dx else None, "k17" if need_dw else None)
    if ours:
        grouped = not gemm and _use_wgrad_grouped_gemm(*a, groups, g)
        if gemm or grouped or (conv_wgrad_supported(*a, dilation, groups, g) and _k17_rule(g)):
            # small planes: the forward as one library GEMM over the im2col matrix, kept for
            # the weight gradient's GEMM (_use_fwd_gemm; grouped: conv_fwd_grouped_gemm)
            fwd = "im2col_gemm" if gemm and g.R * g.S > 1 else "grouped_gemm" if grouped else \
                "gemm_1x1" if _use_fwd_1x1(*a, dilation, groups, g) else "lib"
            dw = "im2col_gemm" if gemm else "bmm_1x1" if _use_wgrad_bmm(*a, groups, g) else \
                "bmm_s2" if fwd == "gemm_1x1" and _use_wgrad_bmm_s2(*a, groups, g) else \
                "grouped_gemm" if grouped else "k17"
            dx = None if not need_dx else "gemm_1x1" if _use_dgrad_1x1(*a, groups, g) else "lib"
            return ConvRoute(g, fwd, dx, dw)
    if need_dx and _use_dgrad_1x1(*a, groups, g):
        # a 1x1 conv K17 does not take (an activation-phase conv, or a small plane): its
        # input gradient as a GEMM, its weight gradient (if any) on MIOpen as before
        return ConvRoute(g, "lib", "gemm_1x1", "lib" if need_dw else None)
    fwd = "gemm_1x1" if not (need_dx or need_dw) and _use_fwd_1x1(*a, dilation, groups, g) \
        else "lib"
    return ConvRoute(g, fwd, "lib" if need_dx else None, "lib" if need_dw else None)


def _k17_rule(g):
    """WGRAD_POLICY (above) for a conv K17 supports and no GEMM form took."""
    if WGRAD_POLICY != "auto":
        return WGRAD_POLICY == "always"
    if g.groups > 1 or wgrad_kind(g[:4], g[4:8], g.st, g.pad, g.groups, g) == 3:
        return True
    return torch.backends.cudnn.deterministic and (g.st > 1 or g.OH * g.OW >= 100)


def conv2d(x, weight, stride=1, padding=0, dilation=1, groups=1):
    """F.conv2d without bias on the kernels conv_route names: depthwise convs on K18/K17,
    otherwise MIOpen with the K17 or a GEMM weight gradient when the weight needs one
    (WGRAD_POLICY); 1x1 stride-2 forwards as one batched GEMM (FWD_1X1_GEMM); a LazyEpi input
    folded into the im2col GEMM of conv_fwd_gemm's shapes, else materialised."""
    grad, lazy = torch.is_grad_enabled(), getattr(x, "_ssq_epi", None) is not None
    # (a LazyEpi placeholder exists only inside the graph of a block being trained)
    route = conv_route(x, weight, stride, padding, dilation, groups,
                       grad and (lazy or x.requires_grad), grad and weight.requires_grad)
    if route.fwd == "epi_gemm":
        return epi_conv_gemm(x, weight, stride, padding)
    if lazy:
        x = materialize_epi(x)
    if route.fwd == "k18":
        if route.dx or route.dw:
            return DwConv2dFn.apply(x, weight, stride, padding)
        return dwconv_fwd(x, weight, stride, padding)
    if route.dw not in (None, "lib") or route.dx == "gemm_1x1":
        return Conv2dFn.apply(x, weight, stride, padding, dilation, groups, route)
    if route.fwd == "gemm_1x1":
        return conv1x1_fwd_gemm(x, weight, stride)
    return torch.nn.functional.conv2d(x, weight, None, stride, padding, dilation, groups)
