"""K32 on strided views of the image (csrc/qinfer_stemu8.hip, "Strided views"): the same bits
whatever the strides.

Each case's image is laid out as every view its channel count allows -- interleaved pixels, three
channels in 4-byte pixels, a planar crop of a larger frame, the same crop of an interleaved frame
at an odd storage offset, every other image of a doubled batch -- with every byte that is not the
image (the pad byte, the frame around the crop, the skipped images) set to 255.  Both output forms
on the view equal, bit for bit, the dense call on `view.contiguous()`, and the fp32 form the numpy
restatement `u8_stem_ref` of the materialised image: a load that leaked into a neighbouring byte,
or took it for a padded tap, would change them."""
import numpy as np
import pytest
import torch

from test_qinfer_gpu import dev, host
from test_qinfer_stemu8_gpu import CASES, PLAIN, epilogue_args, inputs, operands, reference

pytestmark = pytest.mark.gpu
NAMES = ("r7", "s1", "rect", "far", "plane")
LAYOUTS = ("hwc", "rgbx", "crop", "hwc_crop", "batch2")
POISON = 255
AFFINE4 = (True, True, 2, 4)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def allowed(name, layout):
    return layout != "rgbx" or CASES[name][0][1] == 3


def lay_out(u, layout):
    """The numpy image u (N, Ci, H, W) as a device view of that layout; everything around it 255."""
    N, Ci, H, W = u.shape
    t = torch.as_tensor(u)
    if layout == "hwc":
        return t.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
    if layout == "rgbx":
        px = torch.full((N, H, W, 4), POISON, dtype=torch.uint8)
        px[..., :3] = t.permute(0, 2, 3, 1)
        return px.cuda()[..., :3].permute(0, 3, 1, 2)
    if layout == "crop":
        fr = torch.full((N, Ci, H + 5, W + 7), POISON, dtype=torch.uint8)
        fr[:, :, 2:2 + H, 3:3 + W] = t
        return fr.cuda()[:, :, 2:2 + H, 3:3 + W]
    if layout == "hwc_crop":
        FH, FW = H + 5, W + 7
        lead = 1 if ((2 * FW + 3) * Ci) % 2 == 0 else 2        # the crop's storage offset is odd
        flat = torch.full((lead + N * FH * FW * Ci,), POISON, dtype=torch.uint8)
        fr = flat[lead:].view(N, FH, FW, Ci)
        fr[:, 2:2 + H, 3:3 + W, :] = t.permute(0, 2, 3, 1)
        v = flat.cuda()[lead:].view(N, FH, FW, Ci)[:, 2:2 + H, 3:3 + W, :].permute(0, 3, 1, 2)
        assert v.storage_offset() % 2 == 1
        return v
    if layout == "batch2":
        two = torch.full((2 * N, Ci, H, W), POISON, dtype=torch.uint8)
        two[::2] = t
        return two.cuda()[::2]
    raise KeyError(layout)


def expected_form(name, layout):
    Ci = CASES[name][0][1]
    if layout in ("crop", "batch2") or (Ci == 1 and layout in ("hwc", "hwc_crop")):
        return "planar"
    return "interleaved"


def bits(t):
    return host(t).view(np.int32)


def codes_of(K, name, ops, view, epi, border=False):
    tu, prep, M, s = ops
    stride, pad = CASES[name][3], CASES[name][4]
    bias, gamma, phi, act, d, z, nb = epilogue_args(name, epi, reference(name))
    tb = lambda v: None if v is None else dev(v)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = K.stem_conv_u8_codes(view, prep, M, s, tb(bias), tb(gamma), tb(phi), act, float(d),
                               float(z), nb, False, bad, stride=stride, padding=pad,
                               every_tile_border=border)
    return got, int(bad.item())


@pytest.mark.parametrize("name,layout", [(n, l) for n in NAMES for l in LAYOUTS if allowed(n, l)])
def test_every_view_gives_the_dense_bits(K, name, layout):
    stride, pad = CASES[name][3], CASES[name][4]
    u = inputs(name)[0]
    ops = operands(K, name)
    tu, prep, M, s = ops
    view = lay_out(u, layout)
    assert tuple(view.shape) == u.shape and np.array_equal(host(view), u)
    form = K.stem_u8_view_form(view)
    assert form == expected_form(name, layout) and form != "copied"
    dense = view.contiguous()
    assert K.stem_u8_view_form(dense) == "planar"
    want = reference(name)
    y = K.stem_conv_u8(view, prep, M, s, stride, pad)
    yd = K.stem_conv_u8(dense, prep, M, s, stride, pad)
    assert np.array_equal(bits(y), bits(yd)), "the view's fp32 form differs from the dense call's"
    assert np.array_equal(bits(y), want.view(np.int32)), "the view's fp32 form differs from the restatement"
    yb = K.stem_conv_u8(view, prep, M, s, stride, pad, every_tile_border=True)
    assert np.array_equal(bits(yb), bits(y))
    epis = (PLAIN, AFFINE4) if name == "r7" else (PLAIN,)
    for epi in epis:
        c, bad = codes_of(K, name, ops, view, epi)
        cd, bad_d = codes_of(K, name, ops, dense, epi)
        assert bad == 0 and bad_d == 0 and c.dtype == torch.int8
        assert np.array_equal(host(c), host(cd)), f"the view's codes differ from the dense call's {epi}"
        cb, _ = codes_of(K, name, ops, view, epi, border=True)
        assert np.array_equal(host(cb), host(c))
    # the launch read the view in place: the bytes around it are as they were
    assert np.array_equal(host(view), u)


def test_cases_cover_the_forms_and_both_tile_paths(K):
    tiles = lambda n, codes: K.stem_u8_tiles(
        K.StemU8Weight(None, (CASES[n][1], CASES[n][0][1]) + CASES[n][2], None), CASES[n][0],
        CASES[n][3], CASES[n][4], codes)
    for codes in (False, True):
        inner, border = tiles("plane", codes)
        assert inner > 0 and border > 0
        assert tiles("r7", codes)[0] == 0
    forms = {(n, l): expected_form(n, l) for n in NAMES for l in LAYOUTS if allowed(n, l)}
    assert set(forms.values()) == {"planar", "interleaved"}
    # pixels of 2, 3 and 4 bytes, and 3 channels in 4: every interleaved pixel the form takes
    assert {CASES[n][0][1] for n in NAMES} == {1, 2, 3, 4}
    # a stride above the kernel: the patch's columns are not consecutive in memory
    assert CASES["far"][3][1] > CASES["far"][2][1]


def test_a_generic_view_gives_the_dense_bits(K):
    """Any other strides: W and H swapped in memory, and every other column of a wider frame."""
    name = "r7"
    stride, pad = CASES[name][3], CASES[name][4]
    u = inputs(name)[0]
    tu, prep, M, s = operands(K, name)
    want = reference(name).view(np.int32)
    swapped = torch.as_tensor(u).permute(0, 1, 3, 2).contiguous().cuda().permute(0, 1, 3, 2)
    wide = torch.full(u.shape[:3] + (2 * u.shape[3],), POISON, dtype=torch.uint8)
    wide[..., ::2] = torch.as_tensor(u)
    for view in (swapped, wide.cuda()[..., ::2]):
        assert K.stem_u8_view_form(view) == "generic" and np.array_equal(host(view), u)
        for border in (False, True):
            y = K.stem_conv_u8(view, prep, M, s, stride, pad, every_tile_border=border)
            assert np.array_equal(bits(y), want)


def test_a_batch_expanded_view(K):
    """sN = 0: every image of the batch is the same bytes."""
    name = "rect"
    stride, pad = CASES[name][3], CASES[name][4]
    tu, prep, M, s = operands(K, name)
    view = tu.expand(3, *tu.shape[1:])
    assert view.stride(0) == 0 and K.stem_u8_view_form(view) == "planar"
    y = K.stem_conv_u8(view, prep, M, s, stride, pad)
    want = reference(name).view(np.int32)
    for n in range(3):
        assert np.array_equal(bits(y[n:n + 1]), want)


def test_two_runs_and_a_graph_replay_of_an_interleaved_view(K):
    name = "r7"
    stride, pad = CASES[name][3], CASES[name][4]
    bias = inputs(name)[5]
    want = reference(name)
    args = epilogue_args(name, (True, False, 1, 8), want)
    tu, prep, M, s = operands(K, name)
    view = lay_out(inputs(name)[0], "rgbx")
    assert K.stem_u8_view_form(view) == "interleaved"
    tbias = dev(bias)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    both = lambda v: (K.stem_conv_u8(v, prep, M, s, stride, pad),
                      K.stem_conv_u8_codes(v, prep, M, s, tbias, None, None, 1, float(args[4]),
                                           args[5], 8, False, bad, stride=stride, padding=pad))
    yd, cd = both(tu)
    y1, c1 = both(view)
    y2, c2 = both(view)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)) and torch.equal(c1, c2)
    assert torch.equal(y1.view(torch.int32), yd.view(torch.int32)) and torch.equal(c1, cd)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yg, cg = both(view)
    yg.zero_()
    cg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg.view(torch.int32), y1.view(torch.int32)) and torch.equal(cg, c1)
    assert np.array_equal(bits(yg), want.view(np.int32)) and int(bad.item()) == 0


def test_refusals_raise_before_any_launch(K):
    from shiftedscalequantization_amd._capi import SSQError
    name = "r7"
    tu, prep, M, s = operands(K, name)
    N, Ci, H, W = tu.shape
    Co, _, R, S = prep.shape
    stride, pad = CASES[name][3], CASES[name][4]
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    out = torch.full((N, 10, 19, Co), 0x55, dtype=torch.int8, device="cuda")
    y = torch.full((N, Co, 10, 19), 3.0, device="cuda")
    vp = K._vp

    def raw(strides, codes):
        head = (vp(tu), vp(prep.blob), prep.blob.numel(), vp(M), vp(s), N, Ci, H, W, Co, R, S,
                *stride, *pad, *strides, 0)
        if codes:
            K.call("ssq_stem_conv_u8_strided_codes_fwd", *head, None, None, None, 1, 0.1, 0.0, 0,
                   255, vp(out), vp(bad), K.stream_of(out))
        else:
            K.call("ssq_stem_conv_u8_strided_fwd", *head, vp(y), K.stream_of(y))

    dense = (Ci * H * W, H * W, W, 1)
    for codes in (False, True):
        # the channel reversal, the row reversal
        with pytest.raises(SSQError, match="negative stride"):
            raw((Ci * H * W, -H * W, W, 1), codes)
        with pytest.raises(SSQError, match="negative stride"):
            raw((Ci * H * W, H * W, -W, 1), codes)
        with pytest.raises(SSQError, match="2\\^31"):
            raw((1 << 31, H * W, W, 1), codes)
        with pytest.raises(SSQError, match="2\\^31"):
            raw((Ci * H * W, 1 << 30, W, 1), codes)
    torch.cuda.synchronize()
    assert int(bad.item()) == 7 and bool((out == 0x55).all()) and bool((y == 3.0).all())
    raw(dense, True)                                        # and the same calls, valid, write
    raw(dense, False)
    assert int(bad.item()) == 7 and not bool((out == 0x55).all())
    assert np.array_equal(bits(y), reference(name).view(np.int32))
