"""Non-square planes, R x S kernels and stride 3, host side: the case lists the device tests
run (tests/test_conv_rect_gpu.py, tests/test_qinfer_rect_gpu.py import them from here), that
those lists cover both plane orientations, both kernel orientations, padding-only rows or
columns and stride 3; the float64 torch reference itself against a plain five-loop numpy
convolution and weight gradient; and that the library's host-side planners (ssq_conv_wgrad_kind,
ssq_conv_wgrad_workspace_size, ssq_dwconv_supported) put every case on the kernel its list
names.  Nothing here needs a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------- case lists
# K17 through kernels.conv_wgrad: (Nb, C, H, W, Co, R, S, stride, pad, groups)
ROW_TILE = [
    (2, 8, 6, 11, 12, 3, 3, 1, 1, 1), (2, 8, 11, 6, 12, 3, 3, 2, 1, 1),
    (2, 6, 7, 9, 10, 1, 3, 1, 1, 1),         # 1x3 with pad 1: OH = H + 2, rows of padding only
    (2, 6, 9, 7, 10, 3, 1, 1, 1, 1),         # 3x1 with pad 1: OW = W + 2
    (1, 4, 10, 13, 8, 2, 3, 3, 1, 1), (1, 3, 12, 20, 16, 5, 7, 2, 3, 1),
    (2, 12, 5, 8, 18, 3, 3, 1, 1, 3), (2, 12, 8, 5, 18, 1, 3, 2, 1, 2)]       # grouped
I2C = [(2, 16, 5, 9, 128, 3, 3, 1, 1, 1), (1, 8, 9, 5, 130, 1, 3, 2, 1, 1),
       (1, 8, 7, 10, 128, 3, 2, 3, 1, 1)]
# band: the kind (3: 16-byte staging, 6: 4-byte) and the pixels per step V follow band_plan
BAND = [
    ((2, 32, 6, 8, 32, 3, 3, 1, 1, 1), 3, 4), ((2, 32, 8, 6, 64, 3, 3, 1, 1, 1), 6, 2),
    ((2, 32, 7, 4, 32, 3, 3, 1, 1, 1), 6, 4),            # V = 4 on 4-byte staging
    ((1, 32, 5, 9, 32, 3, 3, 1, 1, 1), 6, 1), ((2, 32, 6, 16, 32, 3, 3, 2, 1, 1), 3, 4),
    ((2, 32, 12, 6, 32, 3, 3, 2, 1, 1), 6, 1),
    ((1, 32, 4, 8, 128, 3, 3, 1, 1, 1), 3, 4)]           # the wm = 4 tile
GEMM_1X1 = [(3, 24, 5, 9, 40, 1, 1, 1, 0, 1), (2, 16, 9, 5, 24, 1, 1, 2, 0, 1),
            (2, 16, 7, 10, 24, 1, 1, 3, 0, 1), (2, 12, 4, 7, 18, 1, 1, 1, 0, 3)]
DW_STAGED = [(3, 8, 5, 9, 8, 3, 3, 1, 1, 8), (5, 8, 9, 5, 8, 1, 3, 2, 1, 8),
             (2, 6, 8, 11, 6, 3, 5, 1, 2, 6), (2, 6, 11, 8, 6, 5, 3, 1, 2, 6),
             (2, 8, 10, 7, 8, 3, 3, 3, 1, 8)]
DW_ONE_PLANE = [(2, 8, 20, 60, 8, 3, 3, 1, 1, 8)]       # 4 KiB < padded plane <= 8 KiB
DW_BANDED = [(2, 8, 24, 100, 8, 3, 3, 1, 1, 8), (2, 8, 100, 24, 8, 3, 3, 2, 1, 8)]
DEPTHWISE = DW_STAGED + DW_ONE_PLANE + DW_BANDED
# family -> (cases, the ssq_conv_wgrad_set_form that reaches it, the kinds it may report)
K17 = {
    "row_tile": (ROW_TILE, 1, {1}),
    "i2c": (I2C, 0, {2}),
    "band": ([c for c, _, _ in BAND], 0, {3, 6}),
    "gemm_1x1": (GEMM_1X1, 0, {4}),
    "depthwise": (DEPTHWISE, 0, {5}),
}

# the GEMM forms, called directly: (Nb, C, H, W, Co, R, S, stride, pad); C*R*S % 4 != 0 (scalar
# stores), % 4 == 0 (16-byte stores), stride 3
GEMM_FORMS = [(2, 6, 5, 9, 8, 1, 3, 1, 1), (2, 5, 9, 5, 8, 3, 2, 2, 1), (1, 8, 6, 10, 4, 3, 3, 3, 1)]
# ... and with groups = 2 (the 5-channel case at 10 channels): (.., stride, pad, groups)
GEMM_FORMS_GROUPED = [(2, 6, 5, 9, 8, 1, 3, 1, 1, 2), (2, 10, 9, 5, 8, 3, 2, 2, 1, 2),
                      (1, 8, 6, 10, 4, 3, 3, 3, 1, 2)]
# 1x1 forms: (Nb, C, H, W, Co, stride)
GEMM_1X1_FWD = [(2, 6, 5, 9, 8, 2), (2, 5, 9, 5, 8, 3), (1, 8, 6, 10, 4, 3)]
GEMM_1X1_S1 = [(2, 6, 5, 9, 8), (2, 5, 9, 5, 8), (1, 8, 6, 10, 4)]      # dgrad GEMM, wgrad bmm

# K18 through kernels.dwconv_fwd / dwconv_bwd_data: (Nb, C, H, W, R, S, stride, pad)
K18 = [(2, 8, 6, 11, 3, 3, 1, 1), (2, 8, 11, 6, 1, 3, 2, 1),
       (2, 8, 10, 7, 3, 3, 3, 1), (1, 4, 9, 14, 5, 3, 3, 2),          # the runtime-stride form
       (1, 3, 20, 30, 3, 3, 1, 1),                                    # one plane per workgroup
       (4, 6, 3, 5, 3, 3, 1, 1)]                                      # many planes, ragged last group

# the router, one case per rectangular family: (family, case)
ROUTER = [("row_tile", ROW_TILE[2]), ("row_tile", ROW_TILE[3]), ("row_tile", ROW_TILE[4]),
          ("row_tile", ROW_TILE[6]), ("i2c", I2C[1]), ("i2c", I2C[2]), ("band", BAND[2][0]),
          ("band", BAND[0][0]), ("gemm_1x1", GEMM_1X1[2]), ("depthwise", DW_STAGED[1]), ("depthwise", DW_STAGED[4]), ("depthwise", DW_ONE_PLANE[0]),
          ("depthwise", DW_BANDED[1])]

# integer convs: (N, C, H, W, Co, R, S, stride, pad, groups)
Q_DENSE = [(2, 16, 5, 9, 24, 1, 3, 1, 1, 1), (1, 20, 9, 5, 33, 3, 1, 2, 1, 1),
           (1, 8, 8, 11, 8, 7, 1, 1, 3, 1),              # output columns made only of padding
           (1, 8, 10, 7, 16, 2, 3, 3, 1, 1)]
Q_DEPTHWISE = [(2, 5, 6, 9, 5, 1, 3, 1, 1, 5), (1, 17, 9, 6, 17, 3, 1, 2, 1, 17),
               (1, 8, 9, 12, 8, 5, 7, 2, 3, 8)]
Q_GROUPED = [(2, 48, 5, 8, 48, 1, 3, 1, 1, 2), (1, 72, 8, 5, 72, 3, 2, 2, 1, 3)]
Q_KINDS = {"dense": Q_DENSE, "depthwise": Q_DEPTHWISE, "grouped": Q_GROUPED}


# ---------------------------------------------------------------- the float64 reference
def out_hw(H, W, R, S, st, pad):
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1


def make_inputs(cfg, scale_w=1.0):
    """Seeded fp32 (x, w, dy) of a (Nb, C, H, W, Co, R, S, stride, pad, groups) case."""
    Nb, C, H, W, Co, R, S, st, pad, g = cfg
    gen = torch.Generator().manual_seed(1000 + sum(cfg) + 7 * H + 13 * R)
    x = torch.randn(Nb, C, H, W, generator=gen)
    w = torch.randn(Co, C // g, R, S, generator=gen) * scale_w
    OH, OW = out_hw(H, W, R, S, st, pad)
    dy = torch.randn(Nb, Co, OH, OW, generator=gen)
    return x, w, dy


def ref_fwd(x, w, st, pad, g=1):
    """(float64 F.conv2d, the same conv of the absolute values)."""
    xd, wd = x.double(), w.double()
    return F.conv2d(xd, wd, None, st, pad, 1, g), F.conv2d(xd.abs(), wd.abs(), None, st, pad, 1, g)


def ref_wgrad(x, w_shape, dy, st, pad, g=1):
    xd, dd = x.double(), dy.double()
    return (torch.nn.grad.conv2d_weight(xd, tuple(w_shape), dd, st, pad, 1, g),
            torch.nn.grad.conv2d_weight(xd.abs(), tuple(w_shape), dd.abs(), st, pad, 1, g))


def ref_dgrad(x_shape, w, dy, st, pad, g=1):
    wd, dd = w.double(), dy.double()
    return (torch.nn.grad.conv2d_input(tuple(x_shape), wd, dd, st, pad, 1, g),
            torch.nn.grad.conv2d_input(tuple(x_shape), wd.abs(), dd.abs(), st, pad, 1, g))


def ref_col(x, R, S, st, pad):
    """The im2col matrix (N*OH*OW, C*R*S) of ssq_wgrad_gemm_operands, by F.unfold."""
    c = F.unfold(x, (R, S), padding=pad, stride=st)          # (N, C*R*S, P)
    return c.permute(0, 2, 1).reshape(-1, c.shape[1])


def five_loops(x, w, dy, st, pad):
    """Ungrouped conv forward and weight gradient in float64, one scalar product at a time."""
    x, w, dy = (np.asarray(t, np.float64) for t in (x, w, dy))
    Nb, C, H, W = x.shape
    Co, _, R, S = w.shape
    OH, OW = out_hw(H, W, R, S, st, pad)
    y, dw = np.zeros((Nb, Co, OH, OW)), np.zeros(w.shape)
    for n in range(Nb):
        for co in range(Co):
            for oh in range(OH):
                for ow in range(OW):
                    for ci in range(C):
                        for r in range(R):
                            ih = oh * st + r - pad
                            if not 0 <= ih < H:
                                continue
                            for s in range(S):
                                iw = ow * st + s - pad
                                if 0 <= iw < W:
                                    y[n, co, oh, ow] += w[co, ci, r, s] * x[n, ci, ih, iw]
                                    dw[co, ci, r, s] += dy[n, co, oh, ow] * x[n, ci, ih, iw]
    return y, dw


# ---------------------------------------------------------------- 1. the lists cover the issue
def _geo(c):
    """(H, W, R, S, stride, pad) of a K17 / integer case or a K18 case."""
    return (c[2], c[3], c[5], c[6], c[7], c[8]) if len(c) == 10 else (c[2], c[3], c[4], c[5], c[6], c[7])


def _covers(cases, rect_kernel=True, stride3=True, pad_only=True):
    geo = [_geo(c) for c in cases]
    assert any(H < W for H, W, *_ in geo) and any(H > W for H, W, *_ in geo), cases
    if rect_kernel:
        assert any(R < S for _, _, R, S, _, _ in geo) and any(R > S for _, _, R, S, _, _ in geo), cases
    if stride3:
        assert any(st == 3 for *_, st, _ in geo), cases
    if pad_only:
        assert any(pad >= R or pad >= S for _, _, R, S, _, pad in geo), cases


def test_case_lists_cover_orientations_kernels_padding_and_stride():
    _covers(ROW_TILE)
    _covers(I2C)
    # the band kernel is 3x3 / pad 1 / stride 1-2 only; 1x1 convs have one kernel shape
    _covers([c for c, _, _ in BAND], rect_kernel=False, stride3=False, pad_only=False)
    _covers(GEMM_1X1, rect_kernel=False, pad_only=False)
    _covers(DEPTHWISE)
    _covers(K18)
    _covers([(n, c, h, w, co, r, s, st, p, 1) for n, c, h, w, co, r, s, st, p in GEMM_FORMS])
    _covers(GEMM_FORMS_GROUPED)
    assert any(c[1] * c[5] * c[6] % 4 for c in GEMM_FORMS) and any(c[1] * c[5] * c[6] % 4 == 0 for c in GEMM_FORMS)
    _covers([(n, c, h, w, co, 1, 1, st, 0, 1) for n, c, h, w, co, st in GEMM_1X1_FWD],
            rect_kernel=False, pad_only=False)
    assert {c[5] for c in GEMM_1X1_FWD} == {2, 3}
    _covers(Q_DENSE)
    _covers(Q_DEPTHWISE, stride3=False)
    _covers(Q_GROUPED, stride3=False, pad_only=True)
    _covers([c for _, c in ROUTER])
    assert {f for f, _ in ROUTER} == set(K17)
    for cases in list(Q_KINDS.values()) + [c for c, _, _ in K17.values()]:
        for c in cases:
            assert c[1] % c[9] == 0 and c[4] % c[9] == 0, c
    # every band case is a band shape, and V is what OW says
    for (Nb, C, H, W, Co, R, S, st, pad, g), kind, V in BAND:
        OW = out_hw(H, W, R, S, st, pad)[1]
        assert (R, S, pad, g) == (3, 3, 1, 1) and st in (1, 2) and C % 32 == 0 and Co % 32 == 0
        assert V == (4 if OW % 4 == 0 else 2 if OW % 2 == 0 else 1) and kind in (3, 6)
    # both kinds at V = 4: the 4-byte staging with four pixels per step is provably run
    assert {k for _, k, V in BAND if V == 4} == {3, 6}


# ---------------------------------------------------------------- 2. the reference itself
def test_float64_reference_equals_five_loops():
    """torch's float64 conv2d / conv2d_weight / unfold on one rectangular, stride-3, R != S,
    padded case against scalar loops: the device tests' reference is not itself transposed."""
    cfg = (2, 3, 7, 10, 4, 2, 3, 3, 1, 1)
    x, w, dy = make_inputs(cfg)
    st, pad = cfg[7], cfg[8]
    y5, dw5 = five_loops(x, w, dy, st, pad)
    y, ymag = ref_fwd(x, w, st, pad)
    dw, dmag = ref_wgrad(x, w.shape, dy, st, pad)
    assert y.shape == y5.shape == (2, 4, 3, 4)
    # float64 sums of <= 18 / 24 products in another order: 1e-13 of the absolute sum
    assert np.all(np.abs(y.numpy() - y5) <= 1e-13 * ymag.numpy())
    assert np.all(np.abs(dw.numpy() - dw5) <= 1e-13 * dmag.numpy())
    # the input gradient is the adjoint of the forward: <conv(x, w), dy> == <x, dx>
    dx, _ = ref_dgrad(x.shape, w, dy, st, pad)
    lhs, rhs = float((y * dy.double()).sum()), float((x.double() * dx).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((ymag * dy.double().abs()).sum())
    # im2col: col @ W^T is the forward, dy2 @ col the weight gradient
    col = ref_col(x, 2, 3, st, pad).double()
    y2 = (col @ w.double().reshape(4, -1).t()).reshape(2, 3, 4, 4).permute(0, 3, 1, 2)
    assert np.all(np.abs(y2.numpy() - y5) <= 1e-13 * ymag.numpy())
    dy2 = dy.double().permute(1, 0, 2, 3).reshape(4, -1)
    assert np.all(np.abs((dy2 @ col).reshape(w.shape).numpy() - dw5) <= 1e-13 * dmag.numpy())


# ---------------------------------------------------------------- 3. the host planners
@pytest.fixture(scope="module")
def lib():
    from shiftedscalequantization_amd import _capi
    try:
        return _capi.load()
    except _capi.SSQError as e:
        pytest.skip(f"libssq.so is not built: {e}")


@pytest.fixture
def form(lib):
    old = lib.ssq_conv_wgrad_set_form(0)
    yield lib.ssq_conv_wgrad_set_form
    lib.ssq_conv_wgrad_set_form(old)


@pytest.mark.parametrize("family", sorted(K17))
def test_k17_cases_land_on_their_kernel(lib, form, family):
    cases, f, kinds = K17[family]
    form(f)
    for c in cases:
        assert lib.ssq_conv_wgrad_kind(*c) in kinds, c
        assert lib.ssq_conv_wgrad_workspace_size(*c) > 0, c
    if family == "band":
        for c, kind, _ in BAND:
            for f in (0, 3, 4):
                form(f)
                assert lib.ssq_conv_wgrad_kind(*c) == kind, (c, f)
                assert lib.ssq_conv_wgrad_workspace_size(*c) > 0, (c, f)
            form(1)                       # the A/B knob takes the same shape to the row tile
            assert lib.ssq_conv_wgrad_kind(*c) == 1, c


def test_depthwise_cases_pick_the_three_reductions(lib, form):
    """Staged samples (padded plane <= 4 KiB), one plane (<= 8 KiB), row bands (above): the
    workspace holds one partial per split and band, so its size tells the banded form."""
    def plane(c):
        return (c[2] + 2 * c[8]) * (c[3] + 2 * c[8]) * 4
    assert all(plane(c) <= 4096 for c in DW_STAGED)
    assert all(4096 < plane(c) <= 8192 for c in DW_ONE_PLANE)
    assert all(plane(c) > 8192 for c in DW_BANDED)
    for c in DW_STAGED + DW_ONE_PLANE + DW_BANDED:
        Nb, C, _, _, _, R, S = c[:7]
        per_band = lib.ssq_conv_wgrad_workspace_size(*c) // (C * R * S * 4)
        assert 1 <= per_band and (per_band > Nb) == (c in DW_BANDED), (c, per_band)


def test_k18_and_depthwise_cases_are_supported(lib):
    for Nb, C, H, W, R, S, st, pad in K18:
        assert lib.ssq_dwconv_supported(Nb, C, H, W, R, S, st, pad) == 1
    for Nb, C, H, W, _, R, S, st, pad, _ in DEPTHWISE:
        assert lib.ssq_dwconv_supported(Nb, C, H, W, R, S, st, pad) == 1
    assert lib.ssq_dwconv_supported(1, 4, 9, 14, 5, 6, 3, 2) == 0            # R*S > 25


def test_router_cases_are_k17_shapes(lib, form):
    form(0)
    for family, c in ROUTER:
        assert lib.ssq_conv_wgrad_kind(*c) in K17[family][2] | ({2} if family == "row_tile" else set()), c
        assert lib.ssq_conv_wgrad_workspace_size(*c) > 0, c


def test_string_padding_keeps_the_library_conv():
    """kernels._pair maps 'same' / 'valid' to no list at all: every 1x1 predicate that compares
    it answers "not ours" without raising (the device tests run the convs themselves)."""
    from shiftedscalequantization_amd import kernels as K
    assert K._pair("same") is None and K._pair("valid") is None
    assert K._pair(3) == [3, 3] and K._pair((1, 2)) == [1, 2]
    x, w = torch.zeros(1, 4, 5, 7), torch.zeros(6, 4, 1, 1)
    old = torch.backends.cudnn.deterministic
    try:
        for det in (False, True):
            torch.backends.cudnn.deterministic = det
            for pad in ("same", "valid"):
                assert not K._use_fwd_1x1(x, w, 2, pad, 1, 1)
                assert not K._use_dgrad_1x1(x, w, 1, pad)
                assert not K._use_wgrad_bmm(x, w, 1, pad)
                assert not K._use_wgrad_bmm_s2(x, w, 2, pad)
                assert not K._use_wgrad_gemm(x, w, 1, pad)
                assert not K._use_wgrad_grouped_gemm(x, w, 1, pad, 2)
                assert not K.conv_wgrad_supported(x, w, 1, pad, 1, 1)
                assert not K.dwconv_supported(x, w, 1, pad, 1, 4)
    finally:
        torch.backends.cudnn.deterministic = old
