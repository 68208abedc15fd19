"""The carried stem's two kernels on the device (csrc/qinfer_stem.hip).

K27 ssq_epilogue_codes_fwd: the int8 bytes, channel padding included and written over a
pre-filled buffer, equal (a) the host restatement of the epilogue that ref_codes uses
(test_qinfer_carry_host.ref_pre_quant / quant_codes / stored) and (b) the route the model runs
without carrying, K13 -> act_encode, whose off-grid count must be 0 as must K27's NaN count.
K28 ssq_maxpool_i8_fwd: the bytes equal a numpy signed-byte pool that skips out-of-bounds taps
and, for an 8-bit and a 4-bit quantizer, act_encode(maxpool2d(act_decode(codes))) with nothing
off the grid.  Then the chain K27 -> K28 -> qconv against K13 -> maxpool2d -> qconv."""
import functools
import itertools
import zlib

import numpy as np
import pytest
import torch

from test_qinfer_carry_gpu import fp32_epilogue, pick_quantizer
from test_qinfer_carry_host import cpad, quant_codes, ref_pre_quant, stored
from test_qinfer_gpu import dev, encode_weight, host
from test_qinfer_host import qrange

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


# ---------------------------------------------------------------- K27
CHANNELS = (3, 16, 17, 40, 64, 72)
PLANES = ((2, 5, 7), (1, 9, 4), (2, 8, 8))        # 70, 36 and 128 pixels; H != W both ways
# (out bits, out sym, act, bias, affine): the full product on the first (C, plane)
FULL = list(itertools.product((2, 4, 8), (False, True), (0, 1, 2), (False, True), (False, True)))
VARIED = [(4, True, 2, True, True), (2, False, 1, False, True), (8, True, 0, True, False),
          (4, False, 0, True, True), (8, False, 2, False, False), (2, True, 0, True, True),
          (4, False, 2, True, False), (8, True, 1, True, True), (2, False, 0, False, True),
          (4, True, 0, False, False), (8, False, 0, True, True)]
FIRST = (17, PLANES[0])
OTHERS = [(c, p) for c in CHANNELS for p in PLANES if (c, p) != FIRST]
CASES = [(FIRST, c) for c in FULL] + [(s, VARIED[i % len(VARIED)]) for i, s in enumerate(OTHERS)]


def case_inputs(shape, case, nan_channel=None):
    Cc, (N, H, W) = shape
    _, _, act, use_bias, use_affine = case
    rng = np.random.default_rng(zlib.crc32(repr((shape, case)).encode()))
    y = (rng.normal(0, 3.0, (N, Cc, H, W))).astype(F32)      # ReLU6's upper edge is met
    bias = rng.normal(0, 1.0, Cc).astype(F32) if use_bias else None
    gamma = rng.uniform(-1.5, 1.5, Cc).astype(F32) if use_affine else None     # both signs
    phi = rng.normal(0, 0.5, Cc).astype(F32) if use_affine else None
    if nan_channel is not None:
        bias[nan_channel] = np.nan
    return y, bias, gamma, phi


def both_routes(K, y, bias, gamma, phi, act, d, z, ob, osym):
    """(K27's bytes, its NaN count, act_encode(K13(y)), its off-grid count, K13's output)."""
    tb = lambda v: None if v is None else dev(v)
    Cc = y.shape[1]
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ty, tbias, tgamma, tphi = dev(y), tb(bias), tb(gamma), tb(phi)
    got = K.epilogue_codes(ty, tbias, tgamma, tphi, act, float(d), float(z), ob, osym, bad)
    # the same launch over a pre-filled buffer: every byte is written
    out = torch.full_like(got, 0x55)
    bad2 = torch.zeros(1, dtype=torch.int32, device="cuda")
    vp = K._vp
    K.call("ssq_epilogue_codes_fwd", vp(ty), vp(tbias), vp(tgamma), vp(tphi), *ty.shape, act,
           float(d), float(z), *qrange(ob, osym), vp(out), vp(bad2), K.stream_of(out))
    assert np.array_equal(host(out), host(got)) and int(bad2.item()) == int(bad.item())
    yq = fp32_epilogue(K, ty, tbias, tgamma, tphi, act, d, z, ob, osym)
    plain, bad_b = K.act_encode(yq, float(d), float(z), ob, osym)
    assert tuple(got.shape) == (y.shape[0], y.shape[2], y.shape[3], cpad(Cc))
    return host(got), int(bad.item()), host(plain), int(bad_b.item()), yq


@functools.lru_cache(maxsize=None)
def run_case(shape, case):
    from shiftedscalequantization_amd import kernels as K
    ob, osym, act = case[:3]
    y, bias, gamma, phi = case_inputs(shape, case)
    t = ref_pre_quant(y, bias, gamma, phi, act)
    d, z = pick_quantizer(t, ob, osym)
    q, ref_bad = quant_codes(t, d, z, ob, osym)
    return (stored(q, ob, osym), ref_bad, z) + both_routes(K, y, bias, gamma, phi, act, d, z, ob,
                                                          osym)[:4]


@pytest.mark.parametrize("shape,case", CASES)
def test_epilogue_codes_equal_host_reference_and_fp32_route(K, shape, case):
    ref, ref_bad, _, got, bad, plain, bad_b = run_case(shape, case)
    ob, osym = case[:2]
    Cc = shape[0]
    lo, hi = qrange(ob, osym)
    real = ref[..., :Cc].astype(np.int64) + (lo + 128)
    # both clamp edges and the interior are in the reference
    assert (real == lo).any() and (real == hi).any() and ((real > lo) & (real < hi)).any()
    assert ref_bad == 0 and bad == 0 and bad_b == 0
    assert got.dtype == np.int8 and got.shape == ref.shape and not got[..., Cc:].any()
    assert np.array_equal(got, ref), "K27's codes differ from the host reference"
    assert np.array_equal(got, plain), "K27's codes differ from K13 -> act_encode"


def test_epilogue_cases_cover_the_issue():
    assert {c for s, c in CASES if s == FIRST} == set(FULL) and len(FULL) == 72
    assert {s for s, _ in CASES} == {(c, p) for c in CHANNELS for p in PLANES}
    rest = [c for s, c in CASES if s != FIRST]
    assert {c[0] for c in rest} == {2, 4, 8} and {c[2] for c in rest} == {0, 1, 2}
    # non-zero zero points at both symmetries
    zs = {(c[1], run_case(s, c)[2] != 0) for s, c in CASES}
    assert (False, True) in zs and (True, True) in zs


@pytest.mark.parametrize("Cc,plane", [(17, (2, 5, 7)), (64, (1, 9, 4))])
def test_epilogue_ties_round_half_even(K, Cc, plane):
    """No bias, delta 1: y = k / 2, every odd k sits on a half."""
    N, H, W = plane
    rng = np.random.default_rng(7)
    y = (rng.integers(-41, 42, (N, Cc, H, W)) * 0.5).astype(F32)
    t = ref_pre_quant(y, None, None, None, 0)
    frac = np.abs(t - np.trunc(t))
    assert (frac == 0.5).sum() > 10
    q, ref_bad = quant_codes(t, 1.0, 3.0, 8, True)
    got, bad, plain, bad_b, _ = both_routes(K, y, None, None, None, 0, F32(1.0), 3.0, 8, True)
    assert ref_bad == 0 and bad == 0 and bad_b == 0
    assert np.array_equal(got, stored(q, 8, True)) and np.array_equal(got, plain)
    # spelled out: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 (+ zero point 3, stored - (qmin + 128) = + 0)
    y0 = np.zeros((1, 3, 1, 1), F32)
    y0[0, :, 0, 0] = [0.5, 1.5, 2.5]
    got0 = both_routes(K, y0, None, None, None, 0, F32(1.0), 3.0, 8, True)[0]
    assert got0[0, 0, 0, :3].tolist() == [3, 5, 5]


@pytest.mark.parametrize("Cc,plane", [(17, (2, 5, 7)), (40, (2, 8, 8))])
def test_epilogue_nan_bias_channel_is_qmin_and_counted(K, Cc, plane):
    case = (4, False, 1, True, False)
    y, bias, gamma, phi = case_inputs((Cc, plane), case, nan_channel=Cc // 2)
    t = ref_pre_quant(y, bias, gamma, phi, 1)
    d, z = pick_quantizer(t, 4, False)
    q, ref_bad = quant_codes(t, d, z, 4, False)
    got, bad, plain, bad_b, _ = both_routes(K, y, bias, gamma, phi, 1, d, z, 4, False)
    npix = plane[0] * plane[1] * plane[2]
    assert ref_bad == npix and bad == npix and bad_b == npix
    assert (got[..., Cc // 2] == -128).all()              # qmin's stored form
    assert np.array_equal(got, stored(q, 4, False)) and np.array_equal(got, plain)


def test_epilogue_codes_refuses_bad_arguments(K):
    from shiftedscalequantization_amd._capi import SSQError
    y = dev(np.zeros((1, 5, 3, 3), F32))
    ones = dev(np.ones(5, F32))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    run = lambda bias=None, gamma=None, phi=None, relu=1, d=0.1, z=0.0, bits=4, y=y: \
        K.epilogue_codes(y, bias, gamma, phi, relu, d, z, bits, False, bad)
    for z in (0.5, 256.0, -1.0):
        with pytest.raises(SSQError, match="zero point"):
            run(z=z)
    with pytest.raises(SSQError, match="gamma and phi"):
        run(gamma=ones)
    for d in (0.0, -1.0, float("inf")):
        with pytest.raises(SSQError, match="delta"):
            run(d=d)
    with pytest.raises(SSQError, match="activation"):
        run(relu=3)
    with pytest.raises(SSQError, match="one entry per channel"):
        run(bias=dev(np.ones(6, F32)))
    with pytest.raises(SSQError, match=r"\(N, C, H, W\)"):
        run(y=dev(np.zeros((5, 3), F32)))
    assert run(z=3.0).shape[-1] == 16 and int(bad.item()) == 0


# ---------------------------------------------------------------- K28
POOLS = ((3, 2, 1), (2, 2, 0), (3, 1, 1), (7, 2, 3), (5, 3, 2), (1, 1, 0))
POOL_PLANES = ((7, 10), (10, 7), (8, 8), (3, 3))
POOL_CHANNELS = (3, 16, 40, 64)
POOL_CASES = list(itertools.product(POOLS, POOL_PLANES, POOL_CHANNELS))
# (bits, sym, delta, zero point) of the decoded comparison
POOL_QUANTIZERS = ((8, False, 0.05, 3.0), (4, True, 0.3, -2.0))


def ref_pool(codes, k, stride, pad):
    """Signed-byte max over the in-bounds taps of every window (floor mode), NHWC."""
    N, H, W, Cp = codes.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = np.empty((N, OH, OW, Cp), np.int8)
    for oh in range(OH):
        h0, h1 = max(oh * stride - pad, 0), min(oh * stride - pad + k, H)
        for ow in range(OW):
            w0, w1 = max(ow * stride - pad, 0), min(ow * stride - pad + k, W)
            assert h1 > h0 and w1 > w0                    # every window has a real tap
            out[:, oh, ow] = codes[:, h0:h1, w0:w1].max(axis=(1, 2))
    return out


def random_codes(rng, N, H, W, Cc, n_bits):
    """Stored codes over the quantizer's whole range, padded channels 0."""
    codes = np.zeros((N, H, W, cpad(Cc)), np.int8)
    codes[..., :Cc] = rng.integers(-128, -128 + 2 ** n_bits, (N, H, W, Cc)).astype(np.int8)
    return codes


@pytest.mark.parametrize("pool,plane,Cc", POOL_CASES)
def test_maxpool_codes_equal_byte_pool_and_decoded_pool(K, pool, plane, Cc):
    k, stride, pad = pool
    H, W = plane
    rng = np.random.default_rng(zlib.crc32(repr((pool, plane, Cc)).encode()))
    for n_bits, sym, d, z in POOL_QUANTIZERS:
        codes = random_codes(rng, 2, H, W, Cc, n_bits)
        codes[0, 0, 0, 0], codes[1, H - 1, W - 1, Cc - 1] = -128, -128 + 2 ** n_bits - 1
        want = ref_pool(codes, k, stride, pad)
        got = K.maxpool_codes(dev(codes, torch.int8), k, stride, pad)
        assert got.dtype == torch.int8 and tuple(got.shape) == want.shape
        assert np.array_equal(host(got), want), "K28 differs from the signed-byte pool"
        assert not host(got)[..., Cc:].any()
        # the fp32 route: decode, fp32 max-pool, re-encode
        x = K.act_decode(dev(codes, torch.int8), Cc, d, z, n_bits, sym)
        back, bad = K.act_encode(K.maxpool2d(x, k, stride, pad), d, z, n_bits, sym)
        assert int(bad.item()) == 0
        assert np.array_equal(host(got), host(back)), "K28 differs from the decoded pool"


def test_maxpool_cases_cover_the_issue():
    assert len(POOL_CASES) == 96
    assert {-128, 127} <= set(np.unique(random_codes(np.random.default_rng(1), 2, 8, 8, 64, 8)))


def test_maxpool_codes_refuses_bad_arguments(K):
    from shiftedscalequantization_amd._capi import SSQError
    codes = dev(np.zeros((1, 6, 6, 16), np.int8), torch.int8)
    for k, stride, pad in ((8, 1, 0), (3, 1, 2), (3, 0, 1), (7, 1, 0)):   # the last: OH < 1
        with pytest.raises(SSQError):
            K.maxpool_codes(codes, k, stride, pad)
    with pytest.raises(SSQError, match="Cpad"):
        K.maxpool_codes(dev(np.zeros((1, 6, 6, 5), np.int8), torch.int8), 3, 2, 1)
    with pytest.raises(SSQError, match="int8"):
        K.maxpool_codes(dev(np.zeros((1, 6, 6, 16), F32)), 3, 2, 1)
    assert tuple(K.maxpool_codes(codes, 3, 2, 1).shape) == (1, 3, 3, 16)


def test_planned_pool_pools_codes_and_an_unplanned_one_decodes(K):
    """SsqMaxPool2d on a tagged tensor: codes out when the plan marks it, the fp32 pool of the
    decoded tensor otherwise; an untagged input is pooled as before."""
    import types
    rng = np.random.default_rng(3)
    codes = random_codes(rng, 2, 9, 7, 20, 4)
    pool = K.SsqMaxPool2d(3, 2, 1)
    x = K.act_decode(dev(codes, torch.int8), 20, 0.3, 2.0, 4, False)
    want = K.maxpool2d(x, 3, 2, 1)
    tag = lambda: K.carried(dev(codes, torch.int8), (2, 20, 9, 7), 0.3, 2.0, 4, False)
    out = pool(tag())
    assert out.dtype == torch.float32 and not hasattr(out, "_ssq_codes")
    assert np.array_equal(host(out).view(np.int32), host(want).view(np.int32))
    # (the pool asks its mark whether the edge is live: Edge.live's hook rule, for this pool)
    pool._int_stem = types.SimpleNamespace(
        pooled={pool: 0}, live=lambda: not (pool._forward_hooks or pool._forward_pre_hooks))
    out = pool(tag())
    assert out.dtype == torch.int8 and out._ssq_codes.shape == (2, 20, 5, 4)
    assert out._ssq_codes.quantizer() == (0.3, 2.0, 4, False) and pool._int_stem.pooled[pool] == 1
    assert np.array_equal(host(K.materialize_epi(out)).view(np.int32), host(want).view(np.int32))
    h = pool.register_forward_hook(lambda m, a, o: None)      # a hook sees fp32
    try:
        assert pool(tag()).dtype == torch.float32 and pool._int_stem.pooled[pool] == 1
    finally:
        h.remove()
    assert np.array_equal(host(pool(x)).view(np.int32), host(want).view(np.int32))


# ---------------------------------------------------------------- chain
@pytest.mark.parametrize("Cc,plane,pool,second", [(64, (2, 9, 11), (3, 2, 1), (64, 3, 1, 1)),
                                                  (20, (2, 8, 8), (2, 2, 0), (33, 1, 1, 0))])
def test_chain_into_a_second_layer(K, Cc, plane, pool, second):
    """K27 -> K28 -> qconv on the codes against K13 -> maxpool2d -> qconv re-encoding the fp32
    tensor: identical fp32 outputs, nothing off the grid."""
    Co, R, stride, pad = second
    case = (8, False, 1, True, True)
    y, bias, gamma, phi = case_inputs((Cc, plane), case)
    d, z = pick_quantizer(ref_pre_quant(y, bias, gamma, phi, 1), 8, False)
    got, bad, _, bad_b, yq = both_routes(K, y, bias, gamma, phi, 1, d, z, 8, False)
    assert bad == 0 and bad_b == 0
    rng = np.random.default_rng(29)
    qw, zw = rng.integers(0, 4, (Co, Cc, R, R)), rng.integers(0, 4, Co)
    _, prep = encode_weight(K, qw, zw, np.ones(Co, F32), 2, False)
    s2 = dev(rng.uniform(1e-3, 1e-2, Co).astype(F32))
    kw = dict(act_zp=float(z), act_bits=8, act_sym=False)
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    want = K.qconv(K.maxpool2d(yq, *pool), prep, s2, stride, pad, act_delta=float(d), bad=cnt, **kw)
    pooled = K.maxpool_codes(dev(got, torch.int8), *pool)
    mine = K.qconv(pooled, prep, s2, stride, pad, **kw)
    assert int(cnt.item()) == 0
    assert np.array_equal(host(mine).view(np.int32), host(want).view(np.int32))
