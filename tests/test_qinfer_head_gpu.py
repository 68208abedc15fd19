"""The pooling head's two kernels on the device (csrc/qinfer_head.hip), against a numpy int64
restatement of their contract:

    P[n,c]  = sum_hw (q_a - z_a)                  I[n,co] = sum_c P[n,c] (q_w[co,c] - z_w[co])
    y[n,co] = fp32_rne(I) * sh[co]                sh[co]  = fp32(fp32(delta_a * d1[co]) / fp32(HW))

K29 ssq_avgpool_i8_digits_fwd: 128 * hi + lo is the plane sum of the stored codes, lo lies in
[-64, 63], sp is the per-image sum, padded channels are 0 in a pre-poisoned output.
K30 ssq_qlinear_pooled_fwd: the fp32 bits equal the restatement's, with both image tiles; the
result lies within 2^-21 * sum_c mean_hw|x_hat| |W_hat| of the decoded head in fp64 (six
roundings: x_hat, W_hat, delta_a * d1, / HW, the conversion, the multiply; 6 * 2^-24 < 2^-21)."""
import functools
import itertools
import zlib

import numpy as np
import pytest
import torch

from test_qinfer_gpu import dev, encode_weight, host, parity_log
from test_qinfer_host import qrange

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def cpad(C):
    return (C + 15) // 16 * 16


def stored_nhwc(a_s):
    """Stored codes (N, C, H, W) in [-128, 127] -> the int8 NHWC tensor, channels zero-padded."""
    N, C, H, W = a_s.shape
    out = np.zeros((N, H, W, cpad(C)), np.int8)
    out[..., :C] = np.moveaxis(a_s, 1, -1)
    return out


# ---------------------------------------------------------------- K29
PLANES = ((1, 1), (7, 7), (3, 5), (9, 14))     # 9 x 14 = 126: the digit limit
CHANNELS = (5, 16, 40)                         # padded channels; one chunk; several chunks
FILLS = ("random", "top", "bottom")


def k29_codes(C, plane, fill):
    rng = np.random.default_rng(zlib.crc32(repr((C, plane, fill)).encode()))
    shape = (3, C) + plane
    if fill == "random":
        return rng.integers(-128, 128, shape)
    return np.full(shape, 127 if fill == "top" else -128)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("plane", PLANES)
def test_avgpool_digits_are_the_plane_sums(K, plane, C, fill):
    a_s = k29_codes(C, plane, fill)
    codes = torch.from_numpy(stored_nhwc(a_s)).cuda()
    hi, lo, sp = K.avgpool_codes(codes)
    P = a_s.reshape(3, C, -1).sum(-1)
    Cp = cpad(C)
    assert tuple(hi.shape) == tuple(lo.shape) == (3, Cp) and tuple(sp.shape) == (3,)
    assert hi.dtype == lo.dtype == torch.int8 and sp.dtype == torch.int32
    h, l = host(hi).astype(np.int64), host(lo).astype(np.int64)
    np.testing.assert_array_equal(128 * h[:, :C] + l[:, :C], P)
    assert l.min() >= -64 and l.max() <= 63
    np.testing.assert_array_equal(h[:, :C], (P + 64) >> 7)
    assert not h[:, C:].any() and not l[:, C:].any()
    np.testing.assert_array_equal(host(sp).astype(np.int64), P.sum(1))
    if plane == (9, 14) and fill != "random":
        assert h[:, :C].min() == h[:, :C].max() == ((127 * 126 + 64) >> 7 if fill == "top" else -126)
    # the same launch over poisoned outputs, the real C given and the input's padded channels
    # holding garbage: every output byte is written, padded channels are 0
    dirty = codes.clone()
    dirty[..., C:] = 0x33
    h2, l2 = torch.full_like(hi, 0x55), torch.full_like(lo, 0x55)
    sp2 = torch.full_like(sp, 0x55555555)
    vp = K._vp
    K.call("ssq_avgpool_i8_digits_fwd", vp(dirty), 3, C, plane[0], plane[1], vp(h2), vp(l2),
           vp(sp2), K.stream_of(dirty))
    assert torch.equal(h2, hi) and torch.equal(l2, lo) and torch.equal(sp2, sp)


def test_avgpool_digits_many_chunks_and_slices(K):
    """Cp / 16 = 128 chunks with 2 pixel slices (ResNet-50's 2048 @ 7 x 7), 80 chunks with 3
    (MobileNetV2's 1280), and more than 256 chunks (a second pass of the workgroup)."""
    for C, plane in ((2048, (7, 7)), (1280, (7, 7)), (4200, (2, 3))):
        rng = np.random.default_rng(C)
        a_s = rng.integers(-128, 128, (2, C) + plane)
        hi, lo, sp = K.avgpool_codes(torch.from_numpy(stored_nhwc(a_s)).cuda())
        P = a_s.reshape(2, C, -1).sum(-1)
        got = 128 * host(hi).astype(np.int64) + host(lo).astype(np.int64)
        np.testing.assert_array_equal(got[:, :C], P)
        assert not got[:, C:].any()
        np.testing.assert_array_equal(host(sp).astype(np.int64), P.sum(1))


# ---------------------------------------------------------------- K30
def ref_head(qa, za, qw, zw, scale, HW):
    """The contract restated on the host: (y fp32, I int64, sh fp32)."""
    P = (qa.astype(np.int64) - za).reshape(qa.shape[0], qa.shape[1], -1).sum(-1)
    I = P @ (qw.astype(np.int64) - zw.reshape(-1, 1)).T
    sh = (scale.astype(F32) / F32(HW)).astype(F32)
    return I.astype(F32) * sh.reshape(1, -1), I, sh


def run_head(K, qa, za, qw, zw, da, d1, ab, asym, wb, wsym, tile=16):
    """K29 -> K30 from integer codes; returns (y, W_hat, scale)."""
    alo, _ = qrange(ab, asym)
    what, prep = encode_weight(K, qw, zw, d1, wb, wsym)
    scale = (F32(da) * d1.astype(F32)).astype(F32)
    codes = torch.from_numpy(stored_nhwc(qa - (alo + 128))).cuda()
    HW = qa.shape[2] * qa.shape[3]
    hi, lo, sp = K.avgpool_codes(codes)
    old = K.qlinear_pooled_tile(tile)
    try:
        y = K.qlinear_pooled(hi, lo, sp, prep, K.head_scale(dev(scale), HW), HW, float(za), ab, asym)
    finally:
        K.qlinear_pooled_tile(old)
    return host(y), what, scale


# (weight bits, weight sym, act bits, act sym)
BITS = [(8, False, 8, False), (2, False, 4, False), (4, True, 8, True), (8, True, 4, True),
        (2, True, 8, False), (4, False, 4, True), (8, False, 4, False), (2, False, 8, True),
        (4, True, 4, False), (8, True, 8, True), (2, True, 4, True), (4, False, 8, False)]
SHAPES = list(itertools.product((1, 5, 64, 70), (16, 72, 200), (10, 64, 70)))
CASES = [(s, BITS[i % len(BITS)], PLANES[(i // 3) % len(PLANES)]) for i, s in enumerate(SHAPES)]


@functools.lru_cache(maxsize=None)
def head_case(shape, bits, plane):
    from shiftedscalequantization_amd import kernels as K
    (N, C, Co), (wb, wsym, ab, asym) = shape, bits
    rng = np.random.default_rng(zlib.crc32(repr((shape, bits, plane)).encode()))
    (alo, ahi), (wlo, whi) = qrange(ab, asym), qrange(wb, wsym)
    qa = rng.integers(alo, ahi + 1, (N, C) + plane)
    za = int(rng.integers(alo + 1, ahi + 1))
    if za == 0:
        za = ahi            # a non-zero z_a in every case
    qw = rng.integers(wlo, whi + 1, (Co, C))
    zw = rng.integers(wlo, whi + 1, Co)
    da = F32(rng.uniform(0.01, 0.2))
    d1 = rng.uniform(1e-3, 2e-2, Co).astype(F32)
    y16, what, scale = run_head(K, qa, za, qw, zw, da, d1, ab, asym, wb, wsym, 16)
    y64, _, _ = run_head(K, qa, za, qw, zw, da, d1, ab, asym, wb, wsym, 64)
    ref, I, _ = ref_head(qa, za, qw, zw, scale, plane[0] * plane[1])
    xhat = ((qa - za).astype(F32) * da).astype(np.float64)
    m = xhat.reshape(N, C, -1).mean(-1)
    ma = np.abs(xhat).reshape(N, C, -1).mean(-1)
    w64 = what.astype(np.float64)
    return y16, y64, ref, m @ w64.T, ma @ np.abs(w64).T


def test_cases_cover_every_width_and_path():
    assert {b[0] for _, b, _ in CASES} == {2, 4, 8} and {b[2] for _, b, _ in CASES} == {4, 8}
    assert {b[1] for _, b, _ in CASES} == {b[3] for _, b, _ in CASES} == {False, True}
    assert {p for _, _, p in CASES} == set(PLANES) and len(CASES) == 36


@pytest.mark.parametrize("shape,bits,plane", CASES)
def test_qlinear_pooled_bit_exact(K, shape, bits, plane):
    y16, y64, ref, _, _ = head_case(shape, bits, plane)
    assert y16.shape == ref.shape == (shape[0], shape[2])
    np.testing.assert_array_equal(y16.view(np.int32), ref.view(np.int32))
    np.testing.assert_array_equal(y64.view(np.int32), ref.view(np.int32))


def test_qlinear_pooled_within_bound_of_decoded_head_fp64(K):
    """|y - sum_c mean_hw(x_hat) W_hat| <= 2^-21 * sum_c mean_hw|x_hat| |W_hat| elementwise."""
    worst = 0.0
    for shape, bits, plane in CASES:
        y, _, _, ref64, A = head_case(shape, bits, plane)
        err = np.abs(y.astype(np.float64) - ref64)
        ratio = float((err[A > 0] / A[A > 0]).max()) if (A > 0).any() else 0.0
        print(shape, bits, plane, "worst err / A in 2^-24:", ratio * 2 ** 24)
        worst = max(worst, ratio)
        assert np.all(err <= 2.0 ** -21 * A), (shape, bits, plane, ratio * 2 ** 24)
    parity_log({"test": "qlinear_pooled_vs_fp64", "cases": len(CASES),
                "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 8.0})


def _ones(n):
    return np.ones(n, F32)


def test_qlinear_pooled_extremes_past_int32(K):
    """C = 2048, HW = 49, all-extreme 8-bit codes: |I| = 2048 * 49 * 255^2 > 2^31, the correction
    runs in int64 and the conversion rounds."""
    N, C, Co, plane = 2, 2048, 8, (7, 7)
    scale = np.linspace(0.5, 1.5, Co).astype(F32)
    for qa_v, za, qw_v, zw_v, sign in ((255, 0, 255, 0, 1), (0, 255, 0, 255, 1),
                                       (255, 0, 0, 255, -1), (0, 255, 255, 0, -1)):
        qa, qw = np.full((N, C) + plane, qa_v), np.full((Co, C), qw_v)
        zw = np.full(Co, zw_v)
        ref, I, _ = ref_head(qa, za, qw, zw, scale, 49)
        assert (sign * I).min() == 2048 * 49 * 255 * 255 > 2 ** 31
        for tile in (16, 64):
            y, _, _ = run_head(K, qa, za, qw, zw, 1.0, scale, 8, False, 8, False, tile)
            np.testing.assert_array_equal(y.view(np.int32), ref.view(np.int32))
    # near the top with odd sums: fp32(I) itself rounds
    rng = np.random.default_rng(13)
    qa, qw = rng.integers(253, 256, (N, C) + plane), rng.integers(253, 256, (Co, C))
    zw = np.zeros(Co, np.int64)
    ref, I, _ = ref_head(qa, 0, qw, zw, scale, 49)
    assert I.min() > 2 ** 31 and np.any(I.astype(F32).astype(np.int64) != I)
    y, _, _ = run_head(K, qa, 0, qw, zw, 1.0, scale, 8, False, 8, False)
    np.testing.assert_array_equal(y.view(np.int32), ref.view(np.int32))


def test_qlinear_pooled_identity_weights_lane_map(K):
    """q_w - z_w = delta(co, c) with asymmetric random codes: y[n, co] = P[n, co] * sh[co], so a
    row / column swap or a wrong lane map shows."""
    rng = np.random.default_rng(17)
    N, C, plane = 5, 32, (3, 5)
    zw = rng.integers(0, 255, C)
    qw = zw.reshape(-1, 1) + np.eye(C, dtype=np.int64)
    qa, za = rng.integers(0, 256, (N, C) + plane), 37
    d1 = rng.uniform(0.5, 2.0, C).astype(F32)
    for tile in (16, 64):
        y, _, scale = run_head(K, qa, za, qw, zw, 1.0, d1, 8, False, 8, False, tile)
        P = (qa - za).reshape(N, C, -1).sum(-1)
        want = P.astype(F32) * (scale / F32(15)).astype(F32).reshape(1, -1)
        np.testing.assert_array_equal(y.view(np.int32), want.view(np.int32))


def test_refusals(K):
    from shiftedscalequantization_amd._capi import SSQError
    rng = np.random.default_rng(3)
    qw, zw = rng.integers(0, 256, (10, 40)), rng.integers(0, 256, 10)
    _, prep = encode_weight(K, qw, zw, _ones(10), 8, False)
    sh = dev(_ones(10))
    with pytest.raises(SSQError, match="exceeds 126"):                  # HW = 127
        K.avgpool_codes(torch.zeros(1, 1, 127, 16, dtype=torch.int8, device="cuda"))
    hi, lo, sp = K.avgpool_codes(torch.zeros(2, 7, 7, 48, dtype=torch.int8, device="cuda"))
    y = K.qlinear_pooled(hi, lo, sp, prep, sh, 49)
    assert tuple(y.shape) == (2, 10)
    with pytest.raises(SSQError, match="digit range"):
        K.qlinear_pooled(hi, lo, sp, prep, sh, 127)
    with pytest.raises(SSQError, match="digit range"):
        K.qlinear_pooled(hi, lo, sp, prep, sh, 0)
    wide = torch.zeros(2, 64, dtype=torch.int8, device="cuda")         # Cpad of another layer
    with pytest.raises(SSQError, match="do not match"):
        K.qlinear_pooled(wide, wide, sp, prep, sh, 49)
    with pytest.raises(SSQError, match="do not match"):
        K.qlinear_pooled(hi, wide, sp, prep, sh, 49)
    with pytest.raises(SSQError, match="one entry per image"):
        K.qlinear_pooled(hi, lo, sp[:1], prep, sh, 49)
    with pytest.raises(SSQError, match="one entry per output channel"):
        K.qlinear_pooled(hi, lo, sp, prep, sh[:9], 49)
    conv = K.QPrepared(prep.blob, (10, 40, 1, 1), prep.bad)
    with pytest.raises(SSQError, match="prepared Linear"):
        K.qlinear_pooled(hi, lo, sp, conv, sh, 49)
    vp = K._vp
    out = torch.zeros(2, 10, device="cuda")
    ptrs = [vp(hi), vp(lo), vp(sp), vp(prep.blob), vp(sh)]
    for i in range(6):
        a = list(ptrs) + [vp(out)]
        a[i] = None
        with pytest.raises(SSQError, match="null"):
            K.call("ssq_qlinear_pooled_fwd", *a[:5], 2, 40, 10, 49, 0.0, 0, 255, a[5],
                   K.stream_of(out))
    codes = torch.zeros(2, 7, 7, 48, dtype=torch.int8, device="cuda")
    for i in range(4):
        a = [vp(codes), vp(hi), vp(lo), vp(sp)]
        a[i] = None
        with pytest.raises(SSQError, match="null"):
            K.call("ssq_avgpool_i8_digits_fwd", a[0], 2, 48, 7, 7, *a[1:], K.stream_of(codes))
    assert not out.any()
