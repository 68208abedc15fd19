"""The code-emitting integer conv kernels on the device (ssq_qconv_i8_codes_fwd,
ssq_qconv_i8_grouped_codes_fwd, ssq_act_decode; csrc/qinfer_epi.h).  Every case compares the
int8 bytes, channel padding included, with two references: (a) the host restatement
test_qinfer_carry_host.ref_codes and (b) the route the model runs without carrying, qconv ->
K13 epilogue -> act_encode, whose off-grid count must be 0 as must the fused kernel's NaN
count.  Shapes: partial pixel and channel tiles, channel padding inside and across 64-channel
tiles, depthwise chunk tails, groups that share or straddle 16-B chunks; output quantizers at
2 / 4 / 8 bits, both symmetries, every activation code, bias and gamma^z / phi^z on and off."""
import functools
import itertools
import types
import zlib

import numpy as np
import pytest
import torch

from test_qinfer_carry_host import cpad, ref_codes
from test_qinfer_gpu import dev, encode_weight, host
from test_qinfer_grouped_gpu import encode_weight as encode_weight_grouped
from test_qinfer_host import qrange

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


# (N, C, H, W, Co, R, stride, pad, G)
DENSE = {
    "co5_partial_pixel_tile": (2, 3, 5, 5, 5, 3, 1, 1, 1),
    "co33_s2": (3, 20, 9, 9, 33, 3, 2, 1, 1),
    "co80_two_channel_tiles": (2, 16, 6, 10, 80, 3, 1, 1, 1),
    "exact_tiles_1x1": (2, 64, 8, 8, 64, 1, 1, 0, 1),
}
DEPTHWISE = {
    "dw_c5": (2, 5, 12, 13, 5, 3, 1, 1, 5),             # 312 pixels: two pixel blocks
    "dw_c40_s2": (3, 40, 9, 9, 40, 3, 2, 1, 40),        # a half-filled last chunk
    "dw_c16_5x5": (1, 16, 8, 8, 16, 5, 1, 2, 16),
}
GROUPED = {
    "cog8_shared_chunk": (2, 40, 5, 5, 40, 3, 1, 1, 5),     # last 8 bytes of 48 are padding
    "cog24": (2, 48, 6, 6, 48, 3, 2, 1, 2),
    "cog80_two_tiles": (1, 16, 9, 9, 160, 3, 1, 1, 2),      # 81 pixels: a pixel-tile tail too
    "cog12_wide_padding": (1, 12, 5, 5, 36, 1, 1, 0, 3),    # 12 padded channels, 4 padded rows
    "cog3_byte_stores": (2, 6, 4, 4, 9, 3, 1, 1, 3),
}
SHAPES = {**DENSE, **DEPTHWISE, **GROUPED}

# (out bits, out sym, act, bias, affine): the full product on the first dense shape
FULL = list(itertools.product((2, 4, 8), (False, True), (0, 1, 2), (False, True), (False, True)))
VARIED = [(4, True, 2, True, True), (2, False, 1, False, True), (8, True, 0, True, False),
          (4, False, 1, True, True), (8, False, 2, False, False), (2, True, 0, True, True),
          (4, False, 2, True, False), (8, True, 1, True, True), (2, False, 2, False, True),
          (4, True, 0, False, False), (8, False, 1, True, True)]
FIRST = next(iter(DENSE))
CASES = [(FIRST, c) for c in FULL] + [(n, VARIED[i % len(VARIED)])
                                      for i, n in enumerate(s for s in SHAPES if s != FIRST)]


def pick_quantizer(t, n_bits, sym):
    """(delta, zero point) from the range of the reference's pre-quantizer value: the clamp
    edges sit a quarter of the range inside its minimum and maximum, so both edges (the
    extremes at least) and the interior occur."""
    lo, hi = qrange(n_bits, sym)
    tmin, tmax = float(np.nanmin(t)), float(np.nanmax(t))
    a, b = tmin + 0.25 * (tmax - tmin), tmin + 0.75 * (tmax - tmin)
    d = F32(max(b - a, 1e-3) / (hi - lo))
    z = float(np.clip(np.rint(lo - a / d), lo, hi))
    return d, z


def fp32_epilogue(K, y, bias, gamma, phi, act, d, z, n_bits, sym):
    """K13 as QuantModule.forward runs it: the general epilogue with gamma^z / phi^z, the
    bias + act + quant pass without."""
    dt, zt = dev(np.array([d], F32)), dev(np.array([z], F32))
    with torch.no_grad():
        if gamma is not None:
            q = types.SimpleNamespace(delta=dt, zero_point=zt, n_bits=n_bits, sym=sym)
            return K.epilogue(y, bias, gamma, phi, None, act, q)
        return K.bias_act_quant(y, bias, None, act, dt, zt, n_bits, sym)


def make_layer(K, rng, shape, ab=4, asym=False, wb=4, wsym=False, unit_scale=None):
    """Seeded integer codes of one layer, its prepared weight and the encoded input."""
    N, Cc, H, W, Co, R, stride, pad, G = shape
    alo, ahi = qrange(ab, asym)
    wlo, whi = qrange(wb, wsym)
    L = types.SimpleNamespace(shape=shape, ab=ab, asym=asym)
    L.qa = rng.integers(alo, ahi + 1, (N, Cc, H, W))
    L.za = int(rng.integers(alo, ahi + 1))
    L.qw = rng.integers(wlo, whi + 1, (Co, Cc // G, R, R))
    L.zw = rng.integers(wlo, whi + 1, Co)
    L.da = F32(rng.uniform(0.05, 0.2))
    if G == 1:
        _, L.prep = encode_weight(K, L.qw, L.zw, np.ones(Co, F32), wb, wsym)
    else:
        _, L.prep = encode_weight_grouped(K, L.qw, L.zw, np.ones(Co, F32), wb, wsym, G)
    if unit_scale is None:
        # raw outputs of a few units, so that ReLU6's upper edge is met
        I = ref_codes(L.qa, L.za, L.qw, L.zw, np.ones(Co, F32), stride, pad, None, None, None, 0,
                      1.0, 0.0, 8, False, G)[2]
        L.scale = (F32(4.0 / max(float(I.std()), 1.0)) * rng.uniform(0.5, 1.5, Co)).astype(F32)
    else:
        L.scale = np.full(Co, unit_scale, F32)
    xhat = (L.qa - L.za).astype(F32) * L.da
    L.codes, bad = K.act_encode(dev(xhat), float(L.da), float(L.za), ab, asym)
    assert int(bad.item()) == 0
    return L


def both_routes(K, L, bias, gamma, phi, act, d, z, ob, osym):
    """(fused codes, fused NaN count, uncarried codes, uncarried off-grid count, the uncarried
    route's fp32 epilogue output)."""
    N, Cc, H, W, Co, R, stride, pad, G = L.shape
    tb = lambda v: None if v is None else dev(v)
    kw = dict(groups=G, act_zp=float(L.za), act_bits=L.ab, act_sym=L.asym)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    fused = K.qconv_codes(L.codes, L.prep, dev(L.scale), stride, pad, bias=tb(bias),
                          gamma=tb(gamma), phi=tb(phi), relu=act, out_delta=float(d),
                          out_zp=float(z), out_bits=ob, out_sym=osym, bad=bad, **kw)
    y = K.qconv(L.codes, L.prep, dev(L.scale), stride, pad, **kw)
    yq = fp32_epilogue(K, y, tb(bias), tb(gamma), tb(phi), act, d, z, ob, osym)
    plain, bad_b = K.act_encode(yq, float(d), float(z), ob, osym)
    return host(fused), int(bad.item()), host(plain), int(bad_b.item()), yq


@functools.lru_cache(maxsize=None)
def run_case(name, case):
    from shiftedscalequantization_amd import kernels as K
    ob, osym, act, use_bias, use_affine = case
    shape = SHAPES[name]
    Co, G = shape[4], shape[8]
    rng = np.random.default_rng(zlib.crc32(repr((name, case)).encode()))
    L = make_layer(K, rng, shape)
    bias = rng.normal(0, 1.0, Co).astype(F32) if use_bias else None
    gamma = rng.uniform(0.5, 1.5, Co).astype(F32) if use_affine else None
    phi = rng.normal(0, 0.5, Co).astype(F32) if use_affine else None
    args = (L.qa, L.za, L.qw, L.zw, L.scale, shape[6], shape[7], bias, gamma, phi, act)
    t = ref_codes(*args, 1.0, 0.0, 8, False, G)[2]
    d, z = pick_quantizer(t, ob, osym)
    ref, ref_bad, _ = ref_codes(*args, d, z, ob, osym, G)
    return (ref, ref_bad) + both_routes(K, L, bias, gamma, phi, act, d, z, ob, osym)[:4]


@pytest.mark.parametrize("name,case", CASES)
def test_fused_codes_equal_host_reference_and_uncarried_route(K, name, case):
    ref, ref_bad, fused, bad, plain, bad_b = run_case(name, case)
    ob, osym = case[:2]
    Co = SHAPES[name][4]
    lo, hi = qrange(ob, osym)
    real = ref[..., :Co].astype(np.int64) + (lo + 128)
    # both clamp edges and the interior are in the reference
    assert (real == lo).any() and (real == hi).any() and ((real > lo) & (real < hi)).any()
    assert ref_bad == 0 and bad == 0 and bad_b == 0
    assert fused.dtype == np.int8 and fused.shape == ref.shape and fused.shape[-1] == cpad(Co)
    assert np.array_equal(fused, ref), "fused codes differ from the host reference"
    assert np.array_equal(fused, plain), "fused codes differ from qconv -> K13 -> act_encode"


def test_cases_cover_the_issue():
    first = {c for n, c in CASES if n == FIRST}
    assert first == set(FULL) and len(FULL) == 72
    assert {n for n, _ in CASES} == set(SHAPES)
    rest = [c for n, c in CASES if n != FIRST]
    assert {c[0] for c in rest} == {2, 4, 8} and {c[2] for c in rest} == {0, 1, 2}


@pytest.mark.parametrize("name", ["co80_two_channel_tiles", "dw_c40_s2", "cog8_shared_chunk"])
def test_ties_round_half_even(K, name):
    """scale 0.5, no bias, delta 1: t = I / 2, every odd I sits on a half."""
    shape = SHAPES[name]
    G = shape[8]
    rng = np.random.default_rng(7)
    L = make_layer(K, rng, shape, unit_scale=0.5)
    args = (L.qa, L.za, L.qw, L.zw, L.scale, shape[6], shape[7], None, None, None, 0)
    ref, ref_bad, t = ref_codes(*args, 1.0, 3.0, 8, True, G)
    frac = np.abs(t - np.trunc(t))
    inside = (np.rint(t) + 3 > -128) & (np.rint(t) + 3 < 127)
    assert ((frac == 0.5) & inside).sum() > 10            # ties the clamp does not hide
    fused, bad, plain, bad_b, _ = both_routes(K, L, None, None, None, 0, F32(1.0), 3.0, 8, True)
    assert ref_bad == 0 and bad == 0 and bad_b == 0
    assert np.array_equal(fused, ref) and np.array_equal(fused, plain)


@pytest.mark.parametrize("name", ["co33_s2", "dw_c5", "cog24"])
def test_nan_bias_channel_is_qmin_and_counted(K, name):
    shape = SHAPES[name]
    Co, G = shape[4], shape[8]
    rng = np.random.default_rng(19)
    L = make_layer(K, rng, shape)
    bias = rng.normal(0, 1.0, Co).astype(F32)
    bias[Co // 2] = np.nan
    args = (L.qa, L.za, L.qw, L.zw, L.scale, shape[6], shape[7], bias, None, None, 1)
    d, z = pick_quantizer(ref_codes(*args, 1.0, 0.0, 8, False, G)[2], 4, False)
    ref, ref_bad, _ = ref_codes(*args, d, z, 4, False, G)
    fused, bad, plain, bad_b, _ = both_routes(K, L, bias, None, None, 1, d, z, 4, False)
    npix = ref.shape[0] * ref.shape[1] * ref.shape[2]
    assert ref_bad == npix and bad == npix and bad_b == npix
    assert (fused[..., Co // 2] == -128).all()            # qmin's stored form
    assert np.array_equal(fused, ref) and np.array_equal(fused, plain)


@pytest.mark.parametrize("name,case", [("co33_s2", (4, False, 1, True, True)),
                                       ("dw_c40_s2", (8, True, 2, True, False)),
                                       ("cog8_shared_chunk", (2, False, 0, False, True))])
def test_act_decode_inverts_act_encode_and_decodes_fused_codes(K, name, case):
    ob, osym, act, use_bias, use_affine = case
    shape = SHAPES[name]
    Co, G = shape[4], shape[8]
    rng = np.random.default_rng(23)
    L = make_layer(K, rng, shape)
    bias = rng.normal(0, 1.0, Co).astype(F32) if use_bias else None
    gamma = rng.uniform(0.5, 1.5, Co).astype(F32) if use_affine else None
    phi = rng.normal(0, 0.5, Co).astype(F32) if use_affine else None
    args = (L.qa, L.za, L.qw, L.zw, L.scale, shape[6], shape[7], bias, gamma, phi, act)
    d, z = pick_quantizer(ref_codes(*args, 1.0, 0.0, 8, False, G)[2], ob, osym)
    fused, bad, plain, bad_b, yq = both_routes(K, L, bias, gamma, phi, act, d, z, ob, osym)
    assert bad == 0 and bad_b == 0
    back = K.act_decode(dev(plain, torch.int8), Co, float(d), float(z), ob, osym)
    assert back.shape == yq.shape
    assert np.array_equal(host(back).view(np.int32), host(yq).view(np.int32))
    mine = K.act_decode(dev(fused, torch.int8), Co, float(d), float(z), ob, osym)
    assert np.array_equal(host(mine).view(np.int32), host(yq).view(np.int32))
    # the carried tensor's own decode (materialize_epi) is the same tensor
    carried = K.carried(dev(fused, torch.int8), yq.shape, float(d), float(z), ob, osym)
    assert np.array_equal(host(K.materialize_epi(carried)).view(np.int32), host(yq).view(np.int32))


@pytest.mark.parametrize("first,second", [("co33_s2", (3, 33, 5, 5, 20, 3, 1, 1, 1)),
                                          ("co80_two_channel_tiles", (2, 80, 6, 10, 80, 3, 1, 1, 80)),
                                          ("dw_c40_s2", (3, 40, 5, 5, 24, 1, 1, 0, 1)),
                                          ("cog8_shared_chunk", (2, 40, 5, 5, 40, 3, 1, 1, 5))])
def test_chain_into_a_second_layer(K, first, second):
    """Fused codes as the next layer's operand against the uncarried route's fp32 tensor
    re-encoded by that layer: identical fp32 outputs."""
    shape = SHAPES[first]
    Co, G = shape[4], shape[8]
    rng = np.random.default_rng(29)
    L = make_layer(K, rng, shape)
    bias = rng.normal(0, 1.0, Co).astype(F32)
    args = (L.qa, L.za, L.qw, L.zw, L.scale, shape[6], shape[7], bias, None, None, 1)
    d, z = pick_quantizer(ref_codes(*args, 1.0, 0.0, 8, False, G)[2], 4, False)
    fused, bad, _, bad_b, yq = both_routes(K, L, bias, None, None, 1, d, z, 4, False)
    assert bad == 0 and bad_b == 0 and tuple(yq.shape) == second[:4]
    L2 = make_layer(K, rng, second)
    s2 = dev(rng.uniform(1e-3, 1e-2, second[4]).astype(F32))
    kw = dict(groups=second[8], act_zp=float(z), act_bits=4, act_sym=False)
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    want = K.qconv(yq, L2.prep, s2, second[6], second[7], act_delta=float(d), bad=cnt, **kw)
    got = K.qconv(dev(fused, torch.int8), L2.prep, s2, second[6], second[7], **kw)
    assert int(cnt.item()) == 0
    assert np.array_equal(host(got).view(np.int32), host(want).view(np.int32))


def test_wrappers_refuse_bad_output_quantizers(K):
    from shiftedscalequantization_amd._capi import SSQError
    rng = np.random.default_rng(31)
    for name in ("co5_partial_pixel_tile", "cog24"):
        shape = SHAPES[name]
        L = make_layer(K, rng, shape)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        ones = dev(np.ones(shape[4], F32))
        run = lambda **kw: K.qconv_codes(
            L.codes, L.prep, dev(L.scale), shape[6], shape[7], groups=shape[8],
            act_zp=float(L.za), act_bits=4, bad=bad, **{"out_delta": 0.1, "out_bits": 4, **kw})
        with pytest.raises(SSQError, match="zero point"):
            run(out_zp=0.5)
        with pytest.raises(SSQError, match="zero point"):
            run(out_zp=256.0)
        with pytest.raises(SSQError, match="zero point"):
            run(out_zp=-1.0)
        with pytest.raises(SSQError, match="gamma and phi"):
            run(gamma=ones)
        with pytest.raises(SSQError, match="delta"):
            run(out_delta=0.0)
        with pytest.raises(SSQError, match="activation"):
            run(relu=3)
        with pytest.raises(SSQError, match="one entry per output channel"):
            run(bias=dev(np.ones(shape[4] + 1, F32)))
        assert run(out_zp=3.0).shape[-1] == cpad(shape[4]) and int(bad.item()) == 0
