"""kernels.conv_route's fields against the code that runs: for every route value, on the
smallest shape that selects it, conv2d's output, x.grad and w.grad are bit for bit the direct
call of the executor the route names.  A route field and the dispatch in conv2d / Conv2dFn can
therefore not drift apart.  (The numbers themselves are held to float64 by
tests/test_conv_rect_gpu.py and tests/test_kernels_gpu.py.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


@pytest.fixture
def deterministic():
    """The reference's setting: MIOpen's own gradients are then bit-identical run to run, and
    the rules that only hold under it (bmm_1x1, the 1x1 input-gradient GEMM) apply."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def same_bits(a, b, what):
    assert tuple(a.shape) == tuple(b.shape), what
    np.testing.assert_array_equal(a.detach().cpu().numpy().view(np.int32),
                                  b.detach().cpu().numpy().view(np.int32), err_msg=str(what))


# (name, x shape, Co, kernel, stride, pad, groups, x needs grad, w needs grad, (fwd, dx, dw))
CASES = [
    ("im2col_gemm_3x3", (1, 128, 4, 5), 128, 3, 1, 1, 1, True, True, ("im2col_gemm", "lib", "im2col_gemm")),
    ("im2col_gemm_1x1", (1, 8, 4, 5), 256, 1, 1, 0, 1, True, True, ("lib", "lib", "im2col_gemm")),
    ("bmm_1x1", (1, 8, 20, 21), 8, 1, 1, 0, 1, True, True, ("lib", "lib", "bmm_1x1")),
    ("bmm_s2", (1, 64, 40, 41), 64, 1, 2, 0, 1, True, True, ("gemm_1x1", "lib", "bmm_s2")),
    ("grouped_gemm", (1, 8, 5, 6), 8, 3, 1, 1, 2, True, True, ("grouped_gemm", "lib", "grouped_gemm")),
    ("k17", (1, 8, 15, 16), 8, 3, 1, 1, 2, True, True, ("lib", "lib", "k17")),
    ("dx_gemm_1x1", (1, 8, 3, 4), 8, 1, 1, 0, 1, True, False, ("lib", "gemm_1x1", None)),
    ("dx_gemm_1x1_trained", (1, 8, 3, 4), 8, 1, 1, 0, 1, True, True, ("lib", "gemm_1x1", "im2col_gemm")),
    ("k18", (1, 4, 5, 7), 4, 3, 1, 1, 4, True, True, ("k18", "k18", "k17")),
    ("k18_forward", (1, 4, 5, 7), 4, 3, 1, 1, 4, False, False, ("k18", None, None)),
    ("gemm_1x1_forward", (1, 8, 20, 20), 8, 1, 2, 0, 1, False, False, ("gemm_1x1", None, None)),
    ("lib", (1, 8, 5, 6), 8, 3, 1, 1, 1, True, True, ("lib", "lib", "lib")),
    ("lib_weight_only", (1, 8, 5, 6), 8, 3, 1, 1, 1, False, True, ("lib", None, "lib")),
]


def _direct(K, route, x, w, dy, st, pad, g):
    """The executors the route's three fields name, called directly."""
    xs, ws = x.shape, w.shape
    if route.fwd == "lib" and {route.dx, route.dw} <= {None, "lib"}:
        # all three on the library: conv2d hands the conv to F.conv2d and its autograd
        xa, wa = x.clone().requires_grad_(route.dx == "lib"), w.clone().requires_grad_(route.dw == "lib")
        ya = F.conv2d(xa, wa, None, st, pad, 1, g)
        ya.backward(dy)
        return ya, xa.grad, wa.grad

    def lib(which):
        return torch.ops.aten.convolution_backward(
            dy, x, w, None, [st, st], [pad, pad], [1, 1], False, [0, 0], g,
            tuple(i == which for i in range(3)))[which]
    fwd = {"lib": lambda: F.conv2d(x, w, None, st, pad, 1, g),
           "k18": lambda: K.dwconv_fwd(x, w, st, pad),
           "im2col_gemm": lambda: K.conv_fwd_gemm(x, w, st, pad)[0],
           "grouped_gemm": lambda: K.conv_fwd_grouped_gemm(x, w, st, pad, g)[0],
           "gemm_1x1": lambda: K.conv1x1_fwd_gemm(x, w, st)}[route.fwd]()
    dx = {None: lambda: None, "lib": lambda: lib(0),
          "k18": lambda: K.dwconv_bwd_data(dy, w, xs, st, pad),
          "gemm_1x1": lambda: K.conv1x1_dgrad_gemm(dy, w)}[route.dx]()
    dw = {None: lambda: None, "lib": lambda: lib(1),
          "k17": lambda: K.conv_wgrad(x, dy, ws, st, pad, g),
          "im2col_gemm": lambda: K.conv_wgrad_gemm(x, dy, ws, st, pad),
          "bmm_1x1": lambda: K.conv_wgrad_1x1_bmm(x, dy, ws),
          "bmm_s2": lambda: K.conv_wgrad_1x1_bmm(x[:, :, ::st, ::st].contiguous(), dy, ws),
          "grouped_gemm": lambda: K.conv_wgrad_grouped_gemm(x, dy, ws, st, pad, g)}[route.dw]()
    return fwd, dx, dw


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv2d_runs_what_conv_route_names(K, deterministic, case):
    name, xs, Co, k, st, pad, g, xg, wg, want = case
    gen = torch.Generator().manual_seed(len(name) + 7 * xs[2])
    x = torch.randn(xs, generator=gen).cuda()
    w = (torch.randn(Co, xs[1] // g, k, k, generator=gen) * 0.2).cuda()
    xr, wr = x.clone().requires_grad_(xg), w.clone().requires_grad_(wg)
    route = K.conv_route(xr, wr, st, pad, 1, g, xg, wg)
    assert (route.fwd, route.dx, route.dw) == want
    assert route.geo.single and (route.geo.OH, route.geo.OW) == ((xs[2] + 2 * pad - k) // st + 1,
                                                                 (xs[3] + 2 * pad - k) // st + 1)
    y = K.conv2d(xr, wr, st, pad, 1, g)
    dy = torch.randn(y.shape, generator=gen).cuda()
    if xg or wg:
        y.backward(dy)
    fwd, dx, dw = _direct(K, route, x, w, dy, st, pad, g)
    same_bits(y, fwd, (name, "forward"))
    for got, ref, what in ((xr.grad, dx, "x.grad"), (wr.grad, dw, "w.grad")):
        assert (got is None) == (ref is None), (name, what)
        if ref is not None:
            same_bits(got, ref, (name, what))


def test_lazy_epilogue_input_runs_epi_gemm(K, deterministic):
    """A LazyEpi input on an im2col-GEMM shape: conv_route names epi_gemm and conv2d returns
    epi_conv_gemm's bits (output and weight gradient); on any other shape the placeholder is
    materialised and the conv takes its usual route."""
    gen = torch.Generator().manual_seed(3)
    y1 = torch.randn(1, 128, 4, 5, generator=gen).cuda().requires_grad_(True)
    bias = torch.randn(128, generator=gen).cuda()
    w = (torch.randn(128, 128, 3, 3, generator=gen) * 0.2).cuda()
    outs = []
    for direct in (False, True):
        wr = w.clone().requires_grad_(True)
        x = K.lazy_epilogue(y1, bias, None, None, 1, None)
        route = K.conv_route(x, wr, 1, 1, 1, 1, True, True)
        assert (route.fwd, route.dx, route.dw) == ("epi_gemm", "lib", "im2col_gemm")
        y = K.epi_conv_gemm(x, wr, 1, 1) if direct else K.conv2d(x, wr, 1, 1)
        assert type(y.grad_fn).__name__ == "EpiConvGemmFnBackward"
        y.backward(torch.ones_like(y))
        outs.append((y, wr.grad))
    same_bits(outs[0][0], outs[1][0], "epi_gemm forward")
    same_bits(outs[0][1], outs[1][1], "epi_gemm w.grad")
    same_bits(outs[0][0], K.conv_fwd_gemm(K.bias_act(y1.detach(), bias, None, True), w, 1, 1)[0],
              "epi_gemm against the unfolded forward")
    # a 1x1 conv does not fold: the materialised input takes the 1x1 route
    w1 = (torch.randn(256, 128, 1, 1, generator=gen) * 0.2).cuda().requires_grad_(True)
    x = K.lazy_epilogue(y1, bias, None, None, 1, None)
    route = K.conv_route(x, w1, 1, 0, 1, 1, True, True)
    assert (route.fwd, route.dx, route.dw) == ("lib", "gemm_1x1", "im2col_gemm")
    xm = K.bias_act(y1.detach(), bias, None, True)
    same_bits(K.conv2d(x, w1, 1, 0), F.conv2d(xm, w1.detach()), "materialised input")
