"""The fp32 conv kernels on non-square planes, R x S kernels and stride 3 (the case lists of
tests/test_conv_rect_host.py): K17's six kernels through kernels.conv_wgrad, the GEMM forms
called directly (operand kernel + the Python reshapes), K18 forward / input gradient at the
compile-time and the runtime stride, and kernels.conv2d's routing with tuple / string
arguments.  The reference is torch on the CPU in float64; the bounds are the ones the square
tests of tests/test_kernels_gpu.py hold the same kernels to."""
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_conv_rect_host import (BAND, GEMM_1X1_FWD, GEMM_1X1_S1, GEMM_FORMS, GEMM_FORMS_GROUPED,
                                 K17, K18, ROUTER, make_inputs, out_hw, ref_col, ref_dgrad, ref_fwd,
                                 ref_wgrad)

pytestmark = pytest.mark.gpu

WGRAD_REL, K18_REL, GEMM_REL = 1e-5, 1e-6, 1e-5


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return host(t).view(np.int32)


def same_bits(a, b):
    np.testing.assert_array_equal(bits(a), bits(b))


def parity_log(rec):
    """Print the figure and append it to $SSQ_PARITY_LOG (jsonl) when set."""
    print(json.dumps(rec))
    path = os.environ.get("SSQ_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def within(got, ref_mag, rel, what):
    """Assert |got - ref| <= rel * mag + 1e-30 elementwise; returns the worst err / bound."""
    ref, mag = ref_mag
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    err = (got.detach().double().cpu() - ref).abs()
    worst = float((err / (rel * mag + 1e-30)).max())
    print(what, "worst err / bound", worst)
    assert bool((err <= rel * mag + 1e-30).all()), (what, worst)
    return worst


class policy:
    """kernels' routing switches set for a block, restored after it."""

    def __init__(self, K, **kw):
        self.K, self.kw = K, kw

    def __enter__(self):
        self.old = {k: getattr(self.K, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.K, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(self.K, k, v)


class deterministic:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = self.on

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.old


def wrapper_wgrad(K, xd, wd_shape, w, dyd, st, pad, g):
    """w.grad of kernels.conv2d's autograd with the weight gradient forced onto K17."""
    wd = w.cuda().requires_grad_(True)
    with policy(K, WGRAD_POLICY="always", WGRAD_GEMM="never"):
        K.conv2d(xd, wd, st, pad, 1, g).backward(dyd)
    assert tuple(wd.grad.shape) == tuple(wd_shape)
    return wd.grad


# ---------------------------------------------------------------- K17 through conv_wgrad
K17_CASES = [(f, c) for f in ("row_tile", "i2c", "gemm_1x1", "depthwise") for c in K17[f][0]]


@pytest.mark.parametrize("family,cfg", K17_CASES)
def test_conv_wgrad_rect_matches_fp64(K, family, cfg):
    """K17's row tile, im2col-DMA, 1x1 GEMM and depthwise kernels on rectangular cases: the
    kernel the list names, within the fp32 accumulation bound of the float64 gradient,
    bit-identical run to run, and the autograd wrapper's bits."""
    Nb, C, H, W, Co, R, S, st, pad, g = cfg
    x, w, dy = make_inputs(cfg)
    ref = ref_wgrad(x, w.shape, dy, st, pad, g)
    xd, dyd = x.cuda(), dy.cuda()
    old = K.set_wgrad_form(K17[family][1])
    try:
        kind = K.wgrad_kind(x.shape, w.shape, st, pad, g)
        assert kind in K17[family][2], (cfg, kind)
        dw1 = K.conv_wgrad(xd, dyd, w.shape, st, pad, g)
        dw2 = K.conv_wgrad(xd, dyd, w.shape, st, pad, g)
        gw = wrapper_wgrad(K, xd, w.shape, w, dyd, st, pad, g)
    finally:
        K.set_wgrad_form(old)
    worst = within(dw1, ref, WGRAD_REL, (family, cfg))
    parity_log({"test": "conv_wgrad_rect", "family": family, "case": list(cfg), "kind": kind,
                "worst_err_over_bound": worst})
    same_bits(dw1, dw2)
    same_bits(gw, dw1)


@pytest.mark.parametrize("cfg,kind,V", BAND)
def test_band_wgrad_rect_matches_fp64(K, cfg, kind, V):
    """The band kernel on rectangular planes at 8 and at 4 waves per workgroup: the staging
    (kind 3: 16-byte, 6: 4-byte) band_plan's arithmetic gives, the two forms' bits equal, each
    bit-identical run to run and within the bound, and the autograd wrapper's bits."""
    Nb, C, H, W, Co, R, S, st, pad, g = cfg
    x, w, dy = make_inputs(cfg)
    ref = ref_wgrad(x, w.shape, dy, st, pad, g)
    xd, dyd = x.cuda(), dy.cuda()
    old = K.set_wgrad_form(3)
    try:
        assert K.wgrad_kind(x.shape, w.shape, st, pad, g) == kind
        dw8 = K.conv_wgrad(xd, dyd, w.shape, st, pad, g)
        dw8b = K.conv_wgrad(xd, dyd, w.shape, st, pad, g)
        gw = wrapper_wgrad(K, xd, w.shape, w, dyd, st, pad, g)
        K.set_wgrad_form(4)
        assert K.wgrad_kind(x.shape, w.shape, st, pad, g) == kind
        dw4 = K.conv_wgrad(xd, dyd, w.shape, st, pad, g)
        dw4b = K.conv_wgrad(xd, dyd, w.shape, st, pad, g)
    finally:
        K.set_wgrad_form(old)
    worst = within(dw8, ref, WGRAD_REL, ("band", cfg))
    parity_log({"test": "conv_wgrad_rect", "family": "band", "case": list(cfg), "kind": kind,
                "pixels_per_step": V, "worst_err_over_bound": worst})
    same_bits(dw8, dw8b)
    same_bits(dw4, dw4b)
    same_bits(dw8, dw4)
    same_bits(gw, dw8)


def test_band_cases_run_four_pixels_per_step_on_both_stagings():
    """Kinds 3 and 6 each occur at OW % 4 == 0 among the cases above, so the V = 4 step has
    run on 16-byte and on 4-byte staging."""
    at_v4 = {kind for (_, _, H, W, _, R, S, st, pad, _), kind, V in BAND
             if out_hw(H, W, R, S, st, pad)[1] % 4 == 0}
    assert at_v4 == {3, 6}


# ---------------------------------------------------------------- the GEMM forms, directly
def _operands(K, xd, dyd, Nb, C, H, W, Co, R, S, st, pad, want_col, want_dy2):
    OH, OW = out_hw(H, W, R, S, st, pad)
    NP = Nb * OH * OW
    col = torch.full((NP, C * R * S), float("nan"), device="cuda") if want_col else None
    dy2 = torch.full((Co, NP), float("nan"), device="cuda") if want_dy2 else None
    vp = lambda t: None if t is None else K.C.c_void_p(t.data_ptr())
    K.call("ssq_wgrad_gemm_operands", vp(xd if want_col else None), vp(dyd if want_dy2 else None),
           Nb, C, H, W, Co, R, S, st, pad, vp(col), vp(dy2), K.stream_of(xd))
    return col, dy2


@pytest.mark.parametrize("cfg", GEMM_FORMS)
def test_gemm_operands_rect_exact(K, cfg):
    """ssq_wgrad_gemm_operands == the host im2col / permute exactly: both outputs in one
    launch, and each alone."""
    Nb, C, H, W, Co, R, S, st, pad = cfg
    x, w, dy = make_inputs(cfg + (1,))
    cref = ref_col(x, R, S, st, pad).numpy()
    dref = dy.permute(1, 0, 2, 3).reshape(Co, -1).numpy()
    xd, dyd = x.cuda(), dy.cuda()
    for want_col, want_dy2 in ((True, True), (True, False), (False, True)):
        col, dy2 = _operands(K, xd, dyd, Nb, C, H, W, Co, R, S, st, pad, want_col, want_dy2)
        if want_col:
            np.testing.assert_array_equal(host(col), cref)
        if want_dy2:
            np.testing.assert_array_equal(host(dy2), dref)
    c3, d3 = K.gemm_operands(xd, dyd, w.shape, st, pad)
    np.testing.assert_array_equal(host(c3), cref)
    np.testing.assert_array_equal(host(d3), dref)
    parity_log({"test": "gemm_operands_rect", "case": list(cfg), "kind": "operands",
                "worst_err_over_bound": 0.0})


@pytest.mark.parametrize("cfg", GEMM_FORMS)
def test_conv_gemm_forms_rect_match_fp64(K, cfg):
    """kernels.conv_fwd_gemm and conv_wgrad_gemm (own and saved im2col matrix)."""
    Nb, C, H, W, Co, R, S, st, pad = cfg
    x, w, dy = make_inputs(cfg + (1,))
    xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
    y1, col = K.conv_fwd_gemm(xd, wd, st, pad)
    y2, _ = K.conv_fwd_gemm(xd, wd, st, pad)
    assert y1.is_contiguous()
    same_bits(y1, y2)
    np.testing.assert_array_equal(host(col), ref_col(x, R, S, st, pad).numpy())
    wf = within(y1, ref_fwd(x, w, st, pad), GEMM_REL, ("conv_fwd_gemm", cfg))
    dw1 = K.conv_wgrad_gemm(xd, dyd, w.shape, st, pad)
    dw2 = K.conv_wgrad_gemm(xd, dyd, w.shape, st, pad)
    dw3 = K.conv_wgrad_gemm(xd, dyd, w.shape, st, pad, col=col)
    same_bits(dw1, dw2)
    same_bits(dw1, dw3)
    ww = within(dw1, ref_wgrad(x, w.shape, dy, st, pad), WGRAD_REL, ("conv_wgrad_gemm", cfg))
    parity_log({"test": "conv_gemm_rect", "case": list(cfg), "kind": "im2col_gemm",
                "worst_err_over_bound": max(wf, ww)})


@pytest.mark.parametrize("cfg", GEMM_FORMS_GROUPED)
def test_grouped_gemm_forms_rect_match_fp64(K, cfg):
    """kernels.conv_fwd_grouped_gemm and conv_wgrad_grouped_gemm (own and saved matrix)."""
    Nb, C, H, W, Co, R, S, st, pad, g = cfg
    x, w, dy = make_inputs(cfg)
    xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
    y1, col = K.conv_fwd_grouped_gemm(xd, wd, st, pad, g)
    y2, _ = K.conv_fwd_grouped_gemm(xd, wd, st, pad, g)
    assert y1.is_contiguous()
    same_bits(y1, y2)
    np.testing.assert_array_equal(host(col), ref_col(x, R, S, st, pad).numpy())
    wf = within(y1, ref_fwd(x, w, st, pad, g), GEMM_REL, ("conv_fwd_grouped_gemm", cfg))
    dw1 = K.conv_wgrad_grouped_gemm(xd, dyd, w.shape, st, pad, g)
    dw2 = K.conv_wgrad_grouped_gemm(xd, dyd, w.shape, st, pad, g)
    dw3 = K.conv_wgrad_grouped_gemm(xd, dyd, w.shape, st, pad, g, col=col)
    same_bits(dw1, dw2)
    same_bits(dw1, dw3)
    ww = within(dw1, ref_wgrad(x, w.shape, dy, st, pad, g), WGRAD_REL,
                ("conv_wgrad_grouped_gemm", cfg))
    parity_log({"test": "conv_gemm_rect", "case": list(cfg), "kind": "grouped_gemm",
                "worst_err_over_bound": max(wf, ww)})


@pytest.mark.parametrize("cfg", GEMM_1X1_FWD)
def test_conv1x1_fwd_gemm_rect_matches_fp64(K, cfg):
    """kernels.conv1x1_fwd_gemm at stride 2 and 3 on rectangular planes, and the subsampled
    input it keeps for the weight gradient (conv_wgrad_1x1_bmm over it)."""
    Nb, C, H, W, Co, st = cfg
    x, w, dy = make_inputs((Nb, C, H, W, Co, 1, 1, st, 0, 1))
    xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
    y1, xs = K.conv1x1_fwd_gemm(xd, wd, st, keep_xs=True)
    same_bits(y1, K.conv1x1_fwd_gemm(xd, wd, st))
    np.testing.assert_array_equal(host(xs), x[:, :, ::st, ::st].numpy())
    wf = within(y1, ref_fwd(x, w, st, 0), GEMM_REL, ("conv1x1_fwd_gemm", cfg))
    gw = K.conv_wgrad_1x1_bmm(xs, dyd, w.shape)
    ww = within(gw, ref_wgrad(x, w.shape, dy, st, 0), WGRAD_REL, ("conv_wgrad_1x1_bmm(xs)", cfg))
    parity_log({"test": "conv1x1_gemm_rect", "case": list(cfg), "kind": "fwd_1x1_gemm",
                "worst_err_over_bound": max(wf, ww)})


@pytest.mark.parametrize("cfg", GEMM_1X1_S1)
def test_conv1x1_dgrad_and_wgrad_bmm_rect_match_fp64(K, cfg):
    """kernels.conv1x1_dgrad_gemm and conv_wgrad_1x1_bmm on rectangular planes."""
    Nb, C, H, W, Co = cfg
    x, w, dy = make_inputs((Nb, C, H, W, Co, 1, 1, 1, 0, 1))
    xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
    g1, g2 = K.conv1x1_dgrad_gemm(dyd, wd), K.conv1x1_dgrad_gemm(dyd, wd)
    same_bits(g1, g2)
    wg = within(g1, ref_dgrad(x.shape, w, dy, 1, 0), GEMM_REL, ("conv1x1_dgrad_gemm", cfg))
    d1, d2 = K.conv_wgrad_1x1_bmm(xd, dyd, w.shape), K.conv_wgrad_1x1_bmm(xd, dyd, w.shape)
    same_bits(d1, d2)
    ww = within(d1, ref_wgrad(x, w.shape, dy, 1, 0), WGRAD_REL, ("conv_wgrad_1x1_bmm", cfg))
    parity_log({"test": "conv1x1_gemm_rect", "case": list(cfg), "kind": "dgrad_gemm+wgrad_bmm",
                "worst_err_over_bound": max(wg, ww)})


@pytest.mark.parametrize("full", [True, False], ids=["bias_affine_relu_quant", "bias_only"])
@pytest.mark.parametrize("cfg", GEMM_FORMS)
def test_gemm_col_epilogue_rect_exact(K, cfg, full):
    """ssq_gemm_col_epilogue == the im2col of the materialised K13 epilogue, exactly."""
    Nb, C, H, W, Co, R, S, st, pad = cfg
    x, _, _ = make_inputs(cfg + (1,))
    gen = torch.Generator().manual_seed(sum(cfg) + 5)
    yd = x.cuda()
    bias = torch.randn(C, generator=gen).cuda()
    vp = lambda t: None if t is None else K.C.c_void_p(t.data_ptr())
    OH, OW = out_hw(H, W, R, S, st, pad)
    col = torch.full((Nb * OH * OW, C * R * S), float("nan"), device="cuda")
    with torch.no_grad():
        if full:
            gamma = (torch.rand(C, generator=gen) + 0.5).cuda()
            phi = (torch.randn(C, generator=gen) * 0.5).cuda()
            d, z = torch.tensor([0.125]).cuda(), torch.tensor([2.0]).cuda()
            q = types.SimpleNamespace(delta=d, zero_point=z, n_bits=4, sym=False)
            mat = K.epilogue(yd, bias, gamma, phi, None, 1, q)
            lo, hi = K.qrange(4, False)
            args = (vp(bias), vp(gamma), vp(phi), 1, vp(d), vp(z), lo, hi)
            # ReLU's zeros sit at the zero point, the top clamps, and an interior is kept
            codes = torch.unique(torch.round(mat / 0.125 + 2.0)).tolist()
            assert codes[0] == 2 and codes[-1] == hi and len(codes) > 4, codes
        else:
            mat = K.bias_act(yd, bias, None, False)
            args = (vp(bias), None, None, 0, None, None, 0, 1)
    K.call("ssq_gemm_col_epilogue", vp(yd), *args, Nb, C, H, W, R, S, st, pad, vp(col),
           K.stream_of(yd))
    np.testing.assert_array_equal(bits(col), ref_col(mat.cpu(), R, S, st, pad).numpy().view(np.int32))
    parity_log({"test": "gemm_col_epilogue_rect", "case": list(cfg), "kind": "full" if full else "bias",
                "worst_err_over_bound": 0.0})


# ---------------------------------------------------------------- K18
@pytest.mark.parametrize("cfg", K18)
def test_dwconv_rect_matches_fp64(K, cfg):
    """K18 forward and input gradient on rectangular planes and kernels, at the compile-time
    strides and the runtime one (stride 3): within the fp32 rounding bound of an R*S-term sum,
    bit-identical run to run, and what kernels.conv2d's autograd hands back."""
    Nb, C, H, W, R, S, st, pad = cfg
    full = (Nb, C, H, W, C, R, S, st, pad, C)
    x, w, dy = make_inputs(full)
    xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
    assert K.dwconv_supported(xd, wd, st, pad, 1, C)
    y1, y2 = K.dwconv_fwd(xd, wd, st, pad), K.dwconv_fwd(xd, wd, st, pad)
    same_bits(y1, y2)
    wf = within(y1, ref_fwd(x, w, st, pad, C), K18_REL, ("dwconv_fwd", cfg))
    dx1 = K.dwconv_bwd_data(dyd, wd, x.shape, st, pad)
    dx2 = K.dwconv_bwd_data(dyd, wd, x.shape, st, pad)
    same_bits(dx1, dx2)
    wb = within(dx1, ref_dgrad(x.shape, w, dy, st, pad, C), K18_REL, ("dwconv_bwd_data", cfg))
    parity_log({"test": "dwconv_rect", "case": list(cfg), "kind": "runtime_stride" if st > 2 else f"stride{st}",
                "worst_err_over_bound": max(wf, wb)})
    xg, wg = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
    out = K.conv2d(xg, wg, st, pad, 1, C)
    assert type(out.grad_fn).__name__ == "DwConv2dFnBackward"
    same_bits(out, y1)
    out.backward(dyd)
    same_bits(xg.grad, dx1)
    same_bits(wg.grad, K.conv_wgrad(xd, dyd, w.shape, st, pad, C))
    within(wg.grad, ref_wgrad(x, w.shape, dy, st, pad, C), WGRAD_REL, ("dw wgrad", cfg))


# ---------------------------------------------------------------- the router
def _conv2d_vs_fp64(K, x, w, dy, what, grad=True, **kw):
    """kernels.conv2d(x, w, **kw) -- forward, x.grad, w.grad -- against float64 torch with
    the same arguments; returns (output, x.grad, w.grad, worst err / bound)."""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, **kw)
    ymag = F.conv2d(x.double().abs(), w.double().abs(), None, **kw)
    if dy is None:
        dy = torch.randn(yr.shape, generator=torch.Generator().manual_seed(17))
    yr.backward(dy.double())
    xa, wa = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    F.conv2d(xa, wa, None, **kw).backward(dy.double().abs())
    if not grad:
        with torch.no_grad():
            y = K.conv2d(x.cuda(), w.cuda(), **kw)
        return y, None, None, within(y, (yr.detach(), ymag), GEMM_REL, (what, "forward"))
    xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    y = K.conv2d(xg, wg, **kw)
    worst = within(y, (yr.detach(), ymag), GEMM_REL, (what, "forward"))
    y.backward(dy.cuda())
    worst = max(worst, within(xg.grad, (xr.grad, xa.grad), GEMM_REL, (what, "x.grad")))
    worst = max(worst, within(wg.grad, (wr.grad, wa.grad), WGRAD_REL, (what, "w.grad")))
    return y, xg.grad, wg.grad, worst


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "nondeterministic"])
@pytest.mark.parametrize("family,cfg", ROUTER)
def test_conv2d_routes_rect_cases(K, family, cfg, det):
    """kernels.conv2d on one case per rectangular family: forward, x.grad and w.grad against
    float64 under both cudnn.deterministic settings; depthwise cases run on K18 / K17, bit for
    bit the direct calls."""
    Nb, C, H, W, Co, R, S, st, pad, g = cfg
    x, w, dy = make_inputs(cfg, scale_w=0.2)
    with deterministic(det):
        y, gx, gw, worst = _conv2d_vs_fp64(K, x, w, dy, (family, cfg, det), stride=st, padding=pad,
                                           groups=g)
        kind = K.wgrad_kind(x.shape, w.shape, st, pad, g)
    assert kind in K17[family][2] | ({2} if family == "row_tile" else set())
    if family == "depthwise":
        assert type(y.grad_fn).__name__ == "DwConv2dFnBackward"
        xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
        same_bits(y, K.dwconv_fwd(xd, wd, st, pad))
        same_bits(gx, K.dwconv_bwd_data(dyd, wd, x.shape, st, pad))
        same_bits(gw, K.conv_wgrad(xd, dyd, w.shape, st, pad, g))
    parity_log({"test": "conv2d_router_rect", "family": family, "case": list(cfg), "kind": kind,
                "deterministic": det, "worst_err_over_bound": worst})


# (name, x shape, w shape, F.conv2d keyword arguments)
ARG_FORMS = [
    ("stride_1_2", (2, 6, 7, 10), (8, 6, 3, 3), dict(stride=(1, 2), padding=1)),
    ("stride_2_1_1x1", (2, 6, 7, 10), (8, 6, 1, 1), dict(stride=(2, 1))),
    ("padding_1_0", (2, 6, 7, 10), (8, 6, 3, 3), dict(padding=(1, 0))),
    ("padding_0_1_1x3", (2, 6, 7, 10), (8, 6, 1, 3), dict(padding=(0, 1))),
    ("same_3x3", (2, 6, 7, 10), (8, 6, 3, 3), dict(padding="same")),
    ("valid_3x3", (2, 6, 7, 10), (8, 6, 3, 3), dict(padding="valid")),
    ("same_1x1", (2, 6, 10, 7), (8, 6, 1, 1), dict(padding="same")),
    ("valid_1x1", (2, 6, 10, 7), (8, 6, 1, 1), dict(padding="valid")),
    ("valid_1x1_stride2", (2, 6, 10, 7), (8, 6, 1, 1), dict(stride=2, padding="valid")),
    ("same_depthwise", (2, 6, 7, 10), (6, 1, 3, 3), dict(padding="same", groups=6)),
    ("dilation2", (2, 6, 9, 12), (8, 6, 3, 3), dict(padding=2, dilation=2)),
    ("dilation2_depthwise", (2, 6, 9, 12), (6, 1, 3, 3), dict(padding=2, dilation=2, groups=6)),
]


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "nondeterministic"])
@pytest.mark.parametrize("grad", [True, False], ids=["grad", "no_grad"])
@pytest.mark.parametrize("name,xs,ws,kw", ARG_FORMS, ids=[a[0] for a in ARG_FORMS])
def test_conv2d_argument_forms_match_torch(K, name, xs, ws, kw, grad, det):
    """Tuple strides / paddings, string paddings and dilation: kernels.conv2d returns
    F.conv2d's result (and gradients) and does not raise."""
    gen = torch.Generator().manual_seed(len(name) + 31 * xs[2])
    x, w = torch.randn(xs, generator=gen), torch.randn(ws, generator=gen) * 0.2
    with deterministic(det):
        worst = _conv2d_vs_fp64(K, x, w, None, (name, grad, det), grad=grad, **kw)[3]
    parity_log({"test": "conv2d_argument_forms", "case": name, "kind": "grad" if grad else "no_grad",
                "deterministic": det, "worst_err_over_bound": worst})
