"""K23's code-emitting epilogue with a residual operand on the device
(ssq_qconv_i8_codes_res_fwd; kernels.qconv_codes(..., residual=...)).  Every case compares the
int8 bytes, channel padding included, with (a) the host restatement
test_qinfer_tail_host.ref_codes_res and (b) the route the model runs without carrying the
tail, qconv -> K13 epilogue with the residual -> act_encode, whose off-grid count must be 0 as
must the fused kernel's NaN count.  Both residual kinds (fp32 NCHW; int8 codes with their own
quantizer, whose fp32 form on route (b) is act_decode's) on every dense shape of
test_qinfer_carry_gpu: a partial pixel tile, a Co tail inside a 16-B chunk, two channel tiles
with padding, exact tiles."""
import functools
import types
import zlib

import numpy as np
import pytest
import torch

from test_qinfer_carry_gpu import DENSE, FULL, VARIED, make_layer, pick_quantizer
from test_qinfer_carry_host import cpad, ref_codes, stored
from test_qinfer_gpu import dev, host
from test_qinfer_host import qrange
from test_qinfer_tail_host import decode_res, ref_codes_res

pytestmark = pytest.mark.gpu
F32 = np.float32
KINDS = ("fp32", "codes")

# the residual codes' quantizer (bits, sym, zero point or None for a drawn one): never the
# output's -- 8-bit asymmetric with a mid-range zero point, 4-bit symmetric, 2-bit
RES_Q = [(8, False, 131.0), (4, True, -2.0), (2, False, 1.0)]

FIRST = next(iter(DENSE))
CASES = [(FIRST, c, k) for c in FULL for k in KINDS] + [
    (n, VARIED[(i + j) % len(VARIED)], k)
    for i, n in enumerate(s for s in DENSE if s != FIRST)
    for j, k in enumerate(KINDS * 3)]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def out_dims(shape):
    N, Cc, H, W, Co, R, stride, pad, _ = shape
    return N, Co, (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def make_residual(rng, shape, kind, rq, spread):
    """(fp32 residual NCHW as route (b) adds it, stored residual codes or None, its quantizer).
    For codes: seeded codes over the whole range of `rq`, the delta sized so that the decoded
    residual spans about `spread`."""
    dims = out_dims(shape)
    if kind == "fp32":
        return rng.normal(0, 0.5 * spread, dims).astype(F32), None, None
    rb, rsym, rz = rq
    lo, hi = qrange(rb, rsym)
    q = rng.integers(lo, hi + 1, dims).astype(F32)
    rd = F32(spread / (hi - lo))
    codes = stored(q, rb, rsym)
    return decode_res(codes, dims[1], rd, rz, rb, rsym), codes, (float(rd), float(rz), rb, rsym)


def tail_routes(K, L, bias, gamma, phi, act, d, z, ob, osym, res, res_codes, rquant):
    """(fused codes, fused NaN count, uncarried codes, uncarried off-grid count)."""
    N, Cc, H, W, Co, R, stride, pad, G = L.shape
    tb = lambda v: None if v is None else dev(v)
    kw = dict(groups=G, act_zp=float(L.za), act_bits=L.ab, act_sym=L.asym)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    if res_codes is None:
        r_fused = r_plain = dev(res)
    else:
        rc = dev(res_codes, torch.int8)
        r_fused = K.carried(rc, out_dims(L.shape), *rquant)
        r_plain = K.act_decode(rc, Co, *rquant)             # the fp32 value route (b) adds
        assert np.array_equal(host(r_plain).view(np.int32), res.view(np.int32))
    fused = K.qconv_codes(L.codes, L.prep, dev(L.scale), stride, pad, bias=tb(bias),
                          gamma=tb(gamma), phi=tb(phi), relu=act, out_delta=float(d),
                          out_zp=float(z), out_bits=ob, out_sym=osym, bad=bad, residual=r_fused,
                          **kw)
    y = K.qconv(L.codes, L.prep, dev(L.scale), stride, pad, **kw)
    dt, zt = dev(np.array([d], F32)), dev(np.array([z], F32))
    with torch.no_grad():
        if gamma is not None:
            q = types.SimpleNamespace(delta=dt, zero_point=zt, n_bits=ob, sym=osym)
            yq = K.epilogue(y, tb(bias), tb(gamma), tb(phi), r_plain, act, q)
        else:
            yq = K.bias_act_quant(y, tb(bias), r_plain, act, dt, zt, ob, osym)
    plain, bad_b = K.act_encode(yq, float(d), float(z), ob, osym)
    return host(fused), int(bad.item()), host(plain), int(bad_b.item())


@functools.lru_cache(maxsize=None)
def run_case(name, case, kind):
    from shiftedscalequantization_amd import kernels as K
    ob, osym, act, use_bias, use_affine = case
    shape = DENSE[name]
    Co = shape[4]
    seed = zlib.crc32(repr((name, case, kind)).encode())
    rng = np.random.default_rng(seed)
    L = make_layer(K, rng, shape)
    bias = rng.normal(0, 1.0, Co).astype(F32) if use_bias else None
    gamma = rng.uniform(0.5, 1.5, Co).astype(F32) if use_affine else None
    phi = rng.normal(0, 0.5, Co).astype(F32) if use_affine else None
    conv = (L.qa, L.za, L.qw, L.zw, L.scale, shape[6], shape[7], bias, gamma, phi)
    t0 = ref_codes(*conv, 0, 1.0, 0.0, 8, False)[2]
    rq = RES_Q[seed % len(RES_Q)]
    res, res_codes, rquant = make_residual(rng, shape, kind, rq, float(t0.std()) * 2.0 + 0.5)
    t = ref_codes_res(*conv, act, 1.0, 0.0, 8, False, res)[2]
    d, z = pick_quantizer(t, ob, osym)
    ref, ref_bad, _ = ref_codes_res(*conv, act, d, z, ob, osym, res)
    got = tail_routes(K, L, bias, gamma, phi, act, d, z, ob, osym, res, res_codes, rquant)
    return (ref, ref_bad) + got + (rquant, (float(d), float(z), ob, osym))


@pytest.mark.parametrize("name,case,kind", CASES)
def test_tail_codes_equal_host_reference_and_uncarried_route(K, name, case, kind):
    ref, ref_bad, fused, bad, plain, bad_b, rquant, oquant = run_case(name, case, kind)
    ob, osym = case[:2]
    Co = DENSE[name][4]
    lo, hi = qrange(ob, osym)
    real = ref[..., :Co].astype(np.int64) + (lo + 128)
    edge = float(((real == lo) | (real == hi)).mean())
    print({"case": (name, case, kind), "edge_fraction": edge, "nan": bad, "off_grid": bad_b})
    # both clamp edges and the interior are in the reference
    assert 0.0 < edge < 1.0 and (real == lo).any() and (real == hi).any()
    assert ref_bad == 0 and bad == 0 and bad_b == 0
    assert fused.dtype == np.int8 and fused.shape == ref.shape and fused.shape[-1] == cpad(Co)
    assert not ref[..., Co:].any()
    assert np.array_equal(fused, ref), "fused codes differ from the host reference"
    assert np.array_equal(fused, plain), "fused codes differ from qconv -> K13 -> act_encode"
    assert (rquant is None) == (kind == "fp32") and rquant != oquant


def test_cases_cover_the_issue():
    first = {(c, k) for n, c, k in CASES if n == FIRST}
    assert first == {(c, k) for c in FULL for k in KINDS} and len(FULL) == 72
    assert {(n, k) for n, _, k in CASES} == {(n, k) for n in DENSE for k in KINDS}
    rest = [c for n, c, _ in CASES if n != FIRST]
    assert {c[0] for c in rest} == {2, 4, 8} and {c[2] for c in rest} == {0, 1, 2}
    assert {c[1] for c in rest} == {False, True}
    # the three residual quantizers all occur among the code cases
    seen = {zlib.crc32(repr(c).encode()) % len(RES_Q) for c in CASES if c[2] == "codes"}
    assert seen == {0, 1, 2}
    assert RES_Q[0][:2] == (8, False) and 0 < RES_Q[0][2] < 255
    assert RES_Q[1][:2] == (4, True) and RES_Q[2][0] == 2


@pytest.mark.parametrize("rq", RES_Q)
def test_each_residual_quantizer_on_two_channel_tiles(K, rq):
    """The three residual quantizers by name (the seeded pick above covers them by chance of
    the seed only), against an 8-bit asymmetric output."""
    name, case = "co80_two_channel_tiles", (8, False, 1, True, True)
    shape = DENSE[name]
    Co = shape[4]
    rng = np.random.default_rng(51 + rq[0])
    L = make_layer(K, rng, shape)
    bias = rng.normal(0, 1.0, Co).astype(F32)
    gamma, phi = rng.uniform(0.5, 1.5, Co).astype(F32), rng.normal(0, 0.5, Co).astype(F32)
    conv = (L.qa, L.za, L.qw, L.zw, L.scale, shape[6], shape[7], bias, gamma, phi)
    res, res_codes, rquant = make_residual(rng, shape, "codes", rq, 6.0)
    d, z = pick_quantizer(ref_codes_res(*conv, 1, 1.0, 0.0, 8, False, res)[2], 8, False)
    assert rquant != (float(d), float(z), 8, False)
    ref, ref_bad, _ = ref_codes_res(*conv, 1, d, z, 8, False, res)
    fused, bad, plain, bad_b = tail_routes(K, L, bias, gamma, phi, 1, d, z, 8, False, res,
                                           res_codes, rquant)
    assert ref_bad == 0 and bad == 0 and bad_b == 0
    assert np.array_equal(fused, ref) and np.array_equal(fused, plain)


@pytest.mark.parametrize("kind", KINDS)
def test_ties_round_half_even_from_the_residual(K, kind):
    """Scale 1, no bias, delta 1: the conv's t is an integer and the residual k + 0.5 (fp32), or
    the codes of a delta-0.5 quantizer, are what put t / d on exact halves."""
    shape = DENSE["co80_two_channel_tiles"]
    rng = np.random.default_rng(7)
    L = make_layer(K, rng, shape, unit_scale=1.0)
    conv = (L.qa, L.za, L.qw, L.zw, L.scale, shape[6], shape[7], None, None, None)
    dims = out_dims(shape)
    if kind == "fp32":
        res = (rng.integers(-3, 4, dims) + 0.5).astype(F32)
        res_codes = rquant = None
    else:
        q = rng.integers(-8, 8, dims).astype(F32)
        res_codes, rquant = stored(q, 4, True), (0.5, 0.0, 4, True)
        res = decode_res(res_codes, dims[1], *rquant)
    ref, ref_bad, t = ref_codes_res(*conv, 0, 1.0, 3.0, 8, True, res)
    frac = np.abs(t - np.trunc(t))
    inside = (np.rint(t) + 3 > -128) & (np.rint(t) + 3 < 127)
    assert ((frac == 0.5) & inside).sum() > 10            # ties the clamp does not hide
    fused, bad, plain, bad_b = tail_routes(K, L, None, None, None, 0, F32(1.0), 3.0, 8, True, res,
                                           res_codes, rquant)
    assert ref_bad == 0 and bad == 0 and bad_b == 0
    assert np.array_equal(fused, ref) and np.array_equal(fused, plain)


def test_nan_residual_channel_is_qmin_and_counted(K):
    shape = DENSE["co33_s2"]
    Co = shape[4]
    rng = np.random.default_rng(19)
    L = make_layer(K, rng, shape)
    bias = rng.normal(0, 1.0, Co).astype(F32)
    conv = (L.qa, L.za, L.qw, L.zw, L.scale, shape[6], shape[7], bias, None, None)
    res = rng.normal(0, 1.0, out_dims(shape)).astype(F32)
    res[:, Co // 2] = np.nan
    d, z = pick_quantizer(ref_codes_res(*conv, 1, 1.0, 0.0, 8, False, res)[2], 4, False)
    ref, ref_bad, _ = ref_codes_res(*conv, 1, d, z, 4, False, res)
    fused, bad, plain, bad_b = tail_routes(K, L, bias, None, None, 1, d, z, 4, False, res, None,
                                           None)
    npix = ref.shape[0] * ref.shape[1] * ref.shape[2]
    assert ref_bad == npix and bad == bad_b == npix
    assert (fused[..., Co // 2] == -128).all()            # qmin's stored form
    assert np.array_equal(fused, ref) and np.array_equal(fused, plain)


IDENTITY = {"exact_tiles_1x1": DENSE["exact_tiles_1x1"],
            "c40_two_pixel_tiles": (3, 40, 5, 7, 40, 1, 1, 0, 1)}      # 105 pixels, 8 padded channels


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(IDENTITY))
def test_identity_weight_pins_the_residual_map(K, name, kind):
    """An identity 1x1 conv at unit scale on an input that is distinct per (pixel, channel),
    plus a residual that is too, nothing clamped: the output code is the sum of the two
    patterns, so a residual read at another row or column than the accumulator's shows."""
    from test_qinfer_gpu import encode_weight
    shape = IDENTITY[name]
    N, Co, OH, OW = out_dims(shape)
    rng = np.random.default_rng(61)
    idx = np.arange(N * Co * OH * OW).reshape(N, Co, OH, OW)
    L = types.SimpleNamespace(shape=shape, ab=8, asym=False, za=0, da=F32(0.125))
    L.qa = idx * 7 % 61                                      # 61 and 59: primes below the strides'
    L.zw = rng.integers(0, 15, Co)                           # common factors, sum below 128
    L.qw = (np.eye(Co, dtype=np.int64) + L.zw.reshape(-1, 1)).reshape(Co, Co, 1, 1)
    L.scale = np.ones(Co, F32)
    _, L.prep = encode_weight(K, L.qw, L.zw, np.ones(Co, F32), 4, False)
    L.codes, nb = K.act_encode(dev(L.qa.astype(F32) * L.da), float(L.da), 0.0, 8, False)
    assert int(nb.item()) == 0
    q = (idx * 11 % 59).astype(F32)
    if kind == "fp32":
        res, res_codes, rquant = q.copy(), None, None
    else:
        res_codes, rquant = stored(q + 100, 8, False), (1.0, 100.0, 8, False)
        res = decode_res(res_codes, Co, *rquant)
        assert np.array_equal(res, q)
    conv = (L.qa, L.za, L.qw, L.zw, L.scale, shape[6], shape[7], None, None, None)
    ref, ref_bad, t = ref_codes_res(*conv, 0, 1.0, 0.0, 8, False, res)
    assert np.array_equal(t, (L.qa + q).astype(F32)) and t.max() < 255
    fused, bad, plain, bad_b = tail_routes(K, L, None, None, None, 0, F32(1.0), 0.0, 8, False, res,
                                           res_codes, rquant)
    assert ref_bad == 0 and bad == 0 and bad_b == 0
    assert np.array_equal(fused, ref) and np.array_equal(fused, plain)


def test_wrapper_refuses_bad_residuals(K):
    from shiftedscalequantization_amd._capi import SSQError
    shape = DENSE[FIRST]
    rng = np.random.default_rng(31)
    L = make_layer(K, rng, shape)
    dims = out_dims(shape)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    run = lambda r, **kw: K.qconv_codes(L.codes, L.prep, dev(L.scale), shape[6], shape[7],
                                        act_zp=float(L.za), act_bits=4, bad=bad, out_delta=0.1,
                                        out_bits=4, residual=r, **kw)
    with pytest.raises(SSQError, match="residual"):
        run(torch.zeros(dims[0], dims[1] + 1, dims[2], dims[3], device="cuda"))
    with pytest.raises(SSQError, match="residual"):
        run(torch.zeros(dims, device="cuda", dtype=torch.float16))
    codes = torch.zeros((dims[0], dims[2], dims[3], cpad(dims[1])), dtype=torch.int8, device="cuda")
    with pytest.raises(SSQError, match="residual"):
        run(K.carried(codes, (dims[0], dims[1], dims[2] + 1, dims[3]), 0.1, 0.0, 4, False))
    with pytest.raises(SSQError, match="residual zero point"):
        run(K.carried(codes, dims, 0.1, 0.5, 4, False))
    with pytest.raises(SSQError, match="residual delta"):
        run(K.carried(codes, dims, 0.0, 0.0, 4, False))
    assert run(K.carried(codes, dims, 0.1, 3.0, 4, False)).shape[-1] == cpad(dims[1])
    assert run(torch.zeros(dims, device="cuda")).dtype == torch.int8 and int(bad.item()) == 0
