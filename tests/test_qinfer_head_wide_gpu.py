"""The pooled-operand fc (K30) on a scaled weight: the centred int8 blob through the existing
kernel and the dense wide blob through ssq_qlinear_pooled_wide_fwd (qlinear_pooled(...,
wide_all=True)).  y.view(int32) must EQUAL the host int64 restatement
    I = sum_c P[n, c] m[co, c],  P = sum_hw (q_a - z_a),  m = (q_w - z_w[co]) k[co, c]
    y = fp32(I) * sh[co],  sh[co] = fp32(fp32(delta_a * base[co]) / fp32(L * HW))
for N in {3, 17}, Ci in {40, 130}, Co in {10, 70}, HW in {1, 49, 126} and both image tiles; the two
blobs agree bit for bit where |m| <= 127; at Ci = 2048 with the plane sums at either end and
every m = +-16319, |I| passes 2^40; and K29 -> K30 from act_encode's codes equals the host
restatement of the whole head and stays within the derived bound of the decoded head."""
import functools
import itertools
import zlib

import numpy as np
import pytest
import torch

from test_qinfer_gpu import parity_log
from test_qinfer_head_gpu import stored_nhwc
from test_qinfer_host import qrange
from test_qinfer_perci_gpu import dev, draw_perci_weight, encode_perci, host
from test_qinfer_perci_host import perci_operand

pytestmark = pytest.mark.gpu
F32 = np.float32
PLANES = {1: (1, 1), 49: (7, 7), 126: (9, 14)}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def head_scale_ref(da, base, L, HW):
    """sh[co] = fp32(fp32(delta_a * base[co]) / fp32(L * HW)): one product, one division."""
    s = F32(da) * np.asarray(base, F32)
    assert s.dtype == F32 and float(F32(L * HW)) == L * HW
    return s / F32(L * HW)


def ref_head(qa, za, m, sh):
    """The contract restated on the host: (y fp32, I int64)."""
    P = (np.asarray(qa, np.int64) - za).reshape(qa.shape[0], qa.shape[1], -1).sum(-1)
    I = P @ m.reshape(m.shape[0], -1).T
    return I.astype(F32) * sh.reshape(1, -1), I


def pooled_digits(K, qa, alo):
    return K.avgpool_codes(torch.from_numpy(stored_nhwc(qa - (alo + 128))).cuda())


def run_fc(K, digits, prep, sh, HW, za, ab, asym, tile):
    old = K.qlinear_pooled_tile(tile)
    try:
        return host(K.qlinear_pooled(*digits, prep, dev(sh), HW, float(za), ab, asym, wide_all=True))
    finally:
        K.qlinear_pooled_tile(old)


def scaled_fc(K, rng, Co, Ci, wb):
    """A per-(co, ci) scaled Linear on the L = 32 grid -> (m (Co, Ci), L, base, both blobs or None
    for the int8 one where it does not hold the weight)."""
    qw, zw, wscale = draw_perci_weight(rng, (Co, Ci, 1, 1), wb)
    L, base, k = K.perci_grid(torch.from_numpy(wscale), Co, Ci, K.QWIDE_MAX)
    assert L == 32
    m = perci_operand(qw, zw, k.numpy()).reshape(Co, Ci)
    _, packed = encode_perci(K, qw, zw, wscale, wb)
    wide = K.qweight_prepare(packed, (Co, Ci), dev(zw), wb, 0, kfac=k, wide=True)
    assert wide.wide and wide.centred and int(wide.bad.item()) == 0
    narrow = K.qweight_prepare(packed, (Co, Ci), dev(zw), wb, 0, kfac=k)
    assert int(narrow.bad.item()) == int((np.abs(m) > 127).sum())
    return m, L, base.numpy(), wide, (narrow if np.abs(m).max() <= 127 else None)


SHAPES = list(itertools.product((3, 17), (40, 130), (10, 70), (1, 49, 126)))
# (weight bits, act bits, act sym): W2 fits int8 (both blobs), W4 and W8 leave it
BITS = [(2, 8, False), (4, 4, True), (8, 8, True), (4, 8, False), (2, 4, False), (8, 4, True)]
# (i // 3 counts the shapes without their HW, i % 3 the HW: every HW meets every width)
CASES = [(s, BITS[(i // 3 + i % 3) % len(BITS)]) for i, s in enumerate(SHAPES)]


def test_cases_cover_the_issue():
    assert len(CASES) == 24 and {b[0] for _, b in CASES} == {2, 4, 8}
    assert {b[1:] for _, b in CASES} >= {(8, False), (4, True), (8, True), (4, False)}
    for hw in PLANES:
        assert {b[0] for s, b in CASES if s[3] == hw} == {2, 4, 8}


@functools.lru_cache(maxsize=None)
def head_case(shape, bits):
    from shiftedscalequantization_amd import kernels as K
    (N, Ci, Co, HW), (wb, ab, asym) = shape, bits
    rng = np.random.default_rng(zlib.crc32(repr((shape, bits)).encode()))
    alo, ahi = qrange(ab, asym)
    qa = rng.integers(alo, ahi + 1, (N, Ci) + PLANES[HW])
    za = int(rng.integers(alo + 1, ahi + 1)) or ahi
    m, L, base, wide, narrow = scaled_fc(K, rng, Co, Ci, wb)
    da = F32(rng.uniform(0.01, 0.2))
    sh = head_scale_ref(da, base, L, HW)
    ref, I = ref_head(qa, za, m, sh)
    digits = pooled_digits(K, qa, alo)
    out = {}
    for tile in (16, 64):
        out["wide", tile] = run_fc(K, digits, wide, sh, HW, za, ab, asym, tile)
        if narrow is not None:
            out["int8", tile] = run_fc(K, digits, narrow, sh, HW, za, ab, asym, tile)
    return out, ref, int(np.abs(m).max())


@pytest.mark.parametrize("shape,bits", CASES)
def test_pooled_fc_on_scaled_weights_bit_exact(K, shape, bits):
    out, ref, mmax = head_case(shape, bits)
    assert (mmax <= 127) == (bits[0] == 2) and ref.any()
    assert ("int8", 16) in out if bits[0] == 2 else ("int8", 16) not in out
    for key, y in out.items():
        assert y.shape == ref.shape == (shape[0], shape[2])
        np.testing.assert_array_equal(y.view(np.int32), ref.view(np.int32), err_msg=repr(key))


def test_wide_blob_needs_the_keyword(K):
    from shiftedscalequantization_amd._capi import SSQError
    rng = np.random.default_rng(1)
    _, _, _, wide, _ = scaled_fc(K, rng, 10, 40, 4)
    hi = torch.zeros(2, 48, dtype=torch.int8, device="cuda")
    sp = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(SSQError, match="K30"):
        K.qlinear_pooled(hi, hi.clone(), sp, wide, torch.ones(10, device="cuda"), 4)
    y = K.qlinear_pooled(hi, hi.clone(), sp, wide, torch.ones(10, device="cuda"), 4, 8.0, wide_all=True)
    assert tuple(y.shape) == (2, 10)


@pytest.mark.parametrize("Ci", [2048, 2176])
@pytest.mark.parametrize("at", ["top", "bottom"])
def test_extremes_past_2_to_the_40(K, at, Ci):
    """HW = 126, every stored code at 127 (or -128) with z_a at the other end of the 8-bit range
    (the plane sums P_s at their two ends), every m = +-16319 (W2 codes one step around z = 1,
    k = 16319); one channel all +, one all -, the rest mixed.  At Ci = 2048 that is the largest sum
    the contract allows there, |I| = 2048 * 126 * 255 * 16319 = 2^39.97 (8-bit codes cannot reach 2^40
    at 2048 channels); at Ci = 2176 |I| passes 2^40."""
    N, Co, HW = 2, 8, 126
    rng = np.random.default_rng(5)
    sign = rng.integers(0, 2, (Co, Ci)) * 2 - 1
    sign[0], sign[1] = 1, -1
    zw = np.ones(Co, np.int64)
    qw = (1 + sign).reshape(Co, Ci, 1, 1)
    k = np.full(Co * Ci, 16319)
    m = perci_operand(qw, zw, k).reshape(Co, Ci)
    assert set(np.unique(m)) == {-16319, 16319}
    base = np.linspace(0.5, 1.5, Co).astype(F32)
    wscale = (base[:, None] * (F32(16319) / F32(1024))) * np.ones((Co, Ci), F32)
    _, packed = encode_perci(K, qw, zw, wscale, 2)
    prep = K.qweight_prepare(packed, (Co, Ci), dev(zw), 2, 0, kfac=torch.from_numpy(k), wide=True)
    assert prep.wide and int(prep.bad.item()) == 0
    qa, za = (np.full((N, Ci) + PLANES[HW], 255), 0) if at == "top" else \
        (np.zeros((N, Ci) + PLANES[HW], np.int64), 255)
    sh = head_scale_ref(F32(1.0), base, 1024, HW)
    ref, I = ref_head(qa, za, m, sh)
    assert np.abs(I).max() == Ci * 126 * 255 * 16319 > (2 ** 40 if Ci > 2048 else 2 ** 39)
    assert np.any(I.astype(F32).astype(np.int64) != I)
    digits = pooled_digits(K, qa, 0)
    h = host(digits[0]).astype(np.int64)
    assert (h == ((127 * 126 + 64) >> 7 if at == "top" else -126)).all()
    for tile in (16, 64):
        y = run_fc(K, digits, prep, sh, HW, za, 8, False, tile)
        np.testing.assert_array_equal(y.view(np.int32), ref.view(np.int32))


def test_head_from_codes_end_to_end(K):
    """act_encode -> K29 -> K30 (wide) from an fp32 activation on its grid against the host
    restatement of the whole head, and against the decoded head in fp64 within
    10 * 2^-24 * sum_c mean_hw|x_hat| |W_hat|: the plain head's 8 units (it counts 6
    roundings) plus the 2 the grid adds to the decoded weight (fp32(k / L), fp32(base * .));
    the kernel's own count does not change, L * HW being one exact divisor."""
    rng = np.random.default_rng(23)
    N, Ci, Co, HW, wb, ab = 5, 130, 70, 49, 4, 8
    qa, za = rng.integers(0, 256, (N, Ci) + PLANES[HW]), 117
    da = F32(0.0371)
    xhat = (qa - za).astype(F32) * da
    codes, nb = K.act_encode(dev(xhat), float(da), float(za), ab, False)
    assert int(nb.item()) == 0
    qw, zw, wscale = draw_perci_weight(rng, (Co, Ci, 1, 1), wb)
    L, base, k = K.perci_grid(torch.from_numpy(wscale), Co, Ci, K.QWIDE_MAX)
    m = perci_operand(qw, zw, k.numpy()).reshape(Co, Ci)
    assert np.abs(m).max() > 127
    what, packed = encode_perci(K, qw, zw, wscale, wb)
    prep = K.qweight_prepare_scaled(packed, (Co, Ci), dev(zw), wb, 0, kfac=k, wide=True)
    assert prep.wide and int(prep.bad.item()) == 0
    sh = head_scale_ref(da, base.numpy(), L, HW)
    s0 = dev(F32(da) * base.numpy())
    np.testing.assert_array_equal(host(K.head_scale(s0, L * HW)).view(np.int32), sh.view(np.int32))
    ref, _ = ref_head(qa, za, m, sh)
    y = host(K.qlinear_pooled(*K.avgpool_codes(codes), prep, K.head_scale(s0, L * HW), HW, float(za),
                              ab, False, wide_all=True))
    np.testing.assert_array_equal(y.view(np.int32), ref.view(np.int32))
    x64, w64 = xhat.astype(np.float64), what.reshape(Co, Ci).astype(np.float64)
    ref64 = x64.reshape(N, Ci, -1).mean(-1) @ w64.T
    A = np.abs(x64).reshape(N, Ci, -1).mean(-1) @ np.abs(w64).T
    err = np.abs(y.astype(np.float64) - ref64)
    worst = float((err[A > 0] / A[A > 0]).max())
    parity_log({"test": "qlinear_pooled_wide_vs_fp64", "shape": [N, Ci, Co, HW],
                "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 10.0})
    assert np.all(err <= 10 * 2.0 ** -24 * A)
