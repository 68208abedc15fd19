"""Grouped / depthwise integer inference kernels on the device (K24 ssq_qweight_prepare_grouped,
K25 / K26 ssq_qconv_i8_grouped_fwd): the conv equals the host grouped integer reference
fp32(I) * s bit for bit over groups that share a 16-B chunk, start mid-chunk, span several k
steps and channel tiles, over depthwise planes with chunk tails and 1x1 .. 7x7 taps, at 2..8
bits symmetric or not, at the accumulator extremes and with per-group identity weights (group
isolation, lane map); it stays within the derived fp32 bound of the decoded path's grouped
convolution; and the wrappers refuse mismatched groups."""
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_qinfer_gpu import ALWAYS, ROTATE, dev, host, parity_log
from test_qinfer_grouped_host import grouped_centred_sum, grouped_ref_output
from test_qinfer_host import qrange

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


# (N, C, H, W, Co, R, stride, pad, G)
GROUPED = {
    "g2_one_chunk": (2, 16, 5, 5, 16, 3, 1, 1, 2),
    "cig24_s2": (2, 72, 6, 6, 72, 3, 2, 1, 3),
    "cig40_cog20": (2, 160, 5, 7, 80, 3, 1, 1, 4),
    "cig48_g9": (1, 432, 4, 4, 432, 3, 1, 1, 9),
    "cig56_s2": (1, 112, 4, 4, 112, 3, 2, 1, 2),
    "1x1_cog65": (1, 48, 3, 3, 130, 1, 1, 0, 2),
    "multiplier2": (1, 6, 5, 5, 12, 3, 1, 1, 6),
}
DEPTHWISE = {
    "dw_c5": (2, 5, 6, 7, 5, 3, 1, 1, 5),
    "dw_c40_s2": (3, 40, 9, 9, 40, 3, 2, 1, 40),
    "dw_c960": (1, 960, 7, 7, 960, 3, 1, 1, 960),
    "dw_5x5": (1, 16, 8, 8, 16, 5, 1, 2, 16),
    "dw_7x7": (1, 17, 9, 9, 17, 7, 2, 3, 17),
    "dw_1x1": (1, 33, 3, 3, 33, 1, 1, 0, 33),
}
SHAPES = {**GROUPED, **DEPTHWISE}
KIND = {**{n: "grouped" for n in GROUPED}, **{n: "depthwise" for n in DEPTHWISE}}
# every shape meets 8/8 and 2/2, both symmetries; the other widths rotate over the shapes
CASES = [(name, bits) for i, name in enumerate(SHAPES)
         for bits in ALWAYS + [ROTATE[i % len(ROTATE)], ROTATE[(i + 3) % len(ROTATE)]]]


def encode_weight(K, qw, zw, d1, wb, wsym, groups):
    """Integer codes -> W_hat = (q - zp) * d1 -> the export's packed codes -> K24."""
    wlo, whi = qrange(wb, wsym)
    what = (qw - zw.reshape(-1, 1, 1, 1)).astype(np.float32) * d1.reshape(-1, 1, 1, 1)
    packed, bad = K.pack_encode(dev(what), dev(zw), dev(d1), False, None, wb, wlo, whi)
    assert bad == 0
    prep = K.qweight_prepare(packed, qw.shape, dev(zw), wb, wlo, groups=groups)
    assert int(prep.bad.item()) == 0 and prep.groups == groups
    return what, prep


@functools.lru_cache(maxsize=None)
def run_case(name, bits):
    """Device output and host references of one case, computed once for both tests."""
    from shiftedscalequantization_amd import kernels as K
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES[name]
    wb, wsym, ab, asym = bits
    rng = np.random.default_rng(zlib.crc32(repr((name, bits)).encode()))
    alo, ahi = qrange(ab, asym)
    wlo, whi = qrange(wb, wsym)
    qa = rng.integers(alo, ahi + 1, (N, Cc, H, W))
    za = int(rng.integers(alo, ahi + 1))
    qw = rng.integers(wlo, whi + 1, (Co, Cc // G, R, R))
    zw = rng.integers(wlo, whi + 1, Co)
    da = np.float32(rng.uniform(0.01, 0.2))
    d1 = rng.uniform(1e-3, 2e-2, Co).astype(np.float32)
    xhat = (qa - za).astype(np.float32) * da
    what, prep = encode_weight(K, qw, zw, d1, wb, wsym, G)
    kind = K.qconv_kind(prep)
    scale = da * d1                                     # fp32(delta_a * d1[co])
    assert scale.dtype == np.float32
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = K.qconv(dev(xhat), prep, dev(scale), stride, pad, groups=G, act_zp=float(za),
                act_bits=ab, act_sym=asym, act_delta=float(da), bad=bad)
    ref = grouped_ref_output(qa, za, qw, zw, scale, stride, pad, G)
    xt, wt = torch.from_numpy(xhat).double(), torch.from_numpy(what).double()
    ref64 = F.conv2d(xt, wt, stride=stride, padding=pad, groups=G).numpy()
    A = F.conv2d(xt.abs(), wt.abs(), stride=stride, padding=pad, groups=G).numpy()
    out = host(y)
    assert out.shape == ref.shape
    return out, ref, ref64, A, int(bad.item()), kind


@pytest.mark.parametrize("name,bits", CASES)
def test_qconv_grouped_bit_exact(K, name, bits):
    out, ref, _, _, bad, kind = run_case(name, bits)
    assert bad == 0 and kind == KIND[name]
    np.testing.assert_array_equal(out.view(np.int32), ref.view(np.int32))


def test_cases_cover_every_width():
    assert {b[0] for _, b in CASES} >= {2, 3, 4, 8} and {b[2] for _, b in CASES} >= {2, 4, 8}
    for name in SHAPES:
        assert set(ALWAYS) <= {b for n, b in CASES if n == name}


@pytest.mark.parametrize("name", list(SHAPES))
def test_qconv_grouped_within_fp32_bound_of_decoded_path(K, name):
    """|y - conv64(x_hat, W_hat)| <= 2^-21 * conv64(|x_hat|, |W_hat|) elementwise, the bound of
    test_qinfer_gpu.py: it counts roundings per term and does not depend on grouping."""
    worst = 0.0
    for n, bits in CASES:
        if n != name:
            continue
        out, _, ref64, A, _, _ = run_case(n, bits)
        err = np.abs(out.astype(np.float64) - ref64)
        assert np.all(err <= 2.0 ** -21 * A), (n, bits, float((err / np.maximum(A, 1e-300)).max()))
        nz = A > 0
        if nz.any():
            worst = max(worst, float((err[nz] / A[nz]).max()))
    parity_log({"test": "qconv_grouped_vs_fp64", "shape": name, "kind": KIND[name],
                "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 8.0})


# ---------------------------------------------------------------- extremes, identity
def _run_codes(K, qa, za, qw, zw, scale, stride, pad, groups, ab=8, asym=False, wb=8, wsym=False):
    """Straight from integer codes (delta = 1 so x_hat = q - z exactly)."""
    what, prep = encode_weight(K, qw, zw, np.ones(qw.shape[0], np.float32), wb, wsym, groups)
    xhat = (qa - za).astype(np.float32)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = K.qconv(dev(xhat), prep, dev(scale), stride, pad, groups=groups, act_zp=float(za),
                act_bits=ab, act_sym=asym, act_delta=1.0, bad=bad)
    assert int(bad.item()) == 0
    return host(y)


def test_group_isolation_identity_weights_lane_map(K):
    """q_w - z_w = delta(co_local, ci_local) inside every group, asymmetric random activation
    codes: the output is (q_a - z_a)[n, co] * s[co], so a read from the wrong group or a wrong
    row / column map shows."""
    rng = np.random.default_rng(17)
    N, Cc, H, W, G = 2, 72, 3, 5, 3
    Cig = Cc // G
    zw = rng.integers(0, 255, Cc)
    eye = np.tile(np.eye(Cig, dtype=np.int64), (G, 1))              # (Co, Cig)
    qw = (zw.reshape(-1, 1) + eye).reshape(Cc, Cig, 1, 1)
    qa = rng.integers(0, 256, (N, Cc, H, W))
    za = 37
    scale = rng.uniform(0.5, 2.0, Cc).astype(np.float32)
    out = _run_codes(K, qa, za, qw, zw, scale, 1, 0, G)
    want = (qa - za).astype(np.float32) * scale.reshape(1, -1, 1, 1)
    np.testing.assert_array_equal(out.view(np.int32), want.view(np.int32))


def test_qconv_grouped_extremes_k1440(K):
    N, Cc, H, W, Co, R, G = 2, 320, 4, 4, 64, 3, 2
    Cig = Cc // G
    scale = np.linspace(0.5, 1.5, Co).astype(np.float32)
    # all codes at the top, zero points at the bottom: |I| = 1440 * 255^2 > 2^24, the
    # conversion rounds
    qa, qw = np.full((N, Cc, H, W), 255), np.full((Co, Cig, R, R), 255)
    zw = np.zeros(Co, np.int64)
    I = grouped_centred_sum(qa, 0, qw, zw, 1, 1, G)
    assert I.max() == 1440 * 255 * 255 > 2 ** 24
    ref = grouped_ref_output(qa, 0, qw, zw, scale, 1, 1, G)
    np.testing.assert_array_equal(_run_codes(K, qa, 0, qw, zw, scale, 1, 1, G).view(np.int32),
                                  ref.view(np.int32))
    # near the top with odd sums: fp32(I) itself rounds
    rng = np.random.default_rng(11)
    qa, qw = rng.integers(253, 256, (N, Cc, H, W)), rng.integers(253, 256, (Co, Cig, R, R))
    I = grouped_centred_sum(qa, 0, qw, zw, 1, 1, G)
    assert I.max() > 2 ** 24 and np.any(I.astype(np.float32).astype(np.int64) != I)
    ref = grouped_ref_output(qa, 0, qw, zw, scale, 1, 1, G)
    np.testing.assert_array_equal(_run_codes(K, qa, 0, qw, zw, scale, 1, 1, G).view(np.int32),
                                  ref.view(np.int32))
    # mirrored: all codes at the bottom, zero points at the top
    qa, qw = np.zeros((N, Cc, H, W), np.int64), np.zeros((Co, Cig, R, R), np.int64)
    zw = np.full(Co, 255)
    ref = grouped_ref_output(qa, 255, qw, zw, scale, 1, 1, G)
    assert ref.max() == np.float32(1440 * 255 * 255) * scale.max()
    np.testing.assert_array_equal(_run_codes(K, qa, 255, qw, zw, scale, 1, 1, G).view(np.int32),
                                  ref.view(np.int32))
    # alternating-sign centred weights against a constant input: I = 0 in the interior
    qa = np.full((N, Cc, H, W), 255)
    sign = np.where(np.arange(Cig) % 2 == 0, 1, -1).reshape(1, Cig, 1, 1)
    zw = np.full(Co, 128)
    qw = 128 + 127 * sign * np.ones((Co, Cig, R, R), np.int64)
    ref = grouped_ref_output(qa, 0, qw, zw, scale, 1, 1, G)
    assert not grouped_centred_sum(qa, 0, qw, zw, 1, 1, G).any()
    out = _run_codes(K, qa, 0, qw, zw, scale, 1, 1, G)
    np.testing.assert_array_equal(out.view(np.int32), ref.view(np.int32))
    assert not out.any()


def test_qconv_depthwise_extremes_7x7(K):
    """All codes 255, zero points 0 at 7x7: the largest depthwise |I| = 49 * 255^2, and its
    mirror image (codes 0, zero points 255)."""
    N, Cc, H, W, R = 1, 20, 9, 9, 7
    scale = np.linspace(0.5, 1.5, Cc).astype(np.float32)
    qa, qw = np.full((N, Cc, H, W), 255), np.full((Cc, 1, R, R), 255)
    zw = np.zeros(Cc, np.int64)
    assert grouped_centred_sum(qa, 0, qw, zw, 1, 3, Cc).max() == 49 * 255 * 255
    ref = grouped_ref_output(qa, 0, qw, zw, scale, 1, 3, Cc)
    np.testing.assert_array_equal(_run_codes(K, qa, 0, qw, zw, scale, 1, 3, Cc).view(np.int32),
                                  ref.view(np.int32))
    qa, qw = np.zeros((N, Cc, H, W), np.int64), np.zeros((Cc, 1, R, R), np.int64)
    zw = np.full(Cc, 255)
    ref = grouped_ref_output(qa, 255, qw, zw, scale, 1, 3, Cc)
    np.testing.assert_array_equal(_run_codes(K, qa, 255, qw, zw, scale, 1, 3, Cc).view(np.int32),
                                  ref.view(np.int32))


# ---------------------------------------------------------------- wrappers
def test_wrappers_check_groups_and_channels(K):
    from shiftedscalequantization_amd._capi import SSQError
    rng = np.random.default_rng(3)
    qa = rng.integers(0, 16, (1, 32, 4, 4))
    qw, zw = rng.integers(0, 4, (8, 16, 3, 3)), rng.integers(0, 4, 8)
    scale = np.ones(8, np.float32)
    _, prep_g = encode_weight(K, qw, zw, np.ones(8, np.float32), 2, False, 2)
    codes, _ = K.act_encode(dev((qa - 5).astype(np.float32)), 1.0, 5.0, 4, False)
    y = K.qconv(codes, prep_g, dev(scale), 1, 1, groups=2, act_zp=5.0, act_bits=4)
    ref = grouped_ref_output(qa, 5, qw, zw, scale, 1, 1, 2)
    np.testing.assert_array_equal(host(y).view(np.int32), ref.view(np.int32))
    # groups different from the prepared weight's, both directions
    with pytest.raises(SSQError, match="groups"):
        K.qconv(codes, prep_g, dev(scale), 1, 1, act_zp=5.0, act_bits=4)
    with pytest.raises(SSQError, match="groups"):
        K.qconv(codes, prep_g, dev(scale), 1, 1, groups=4, act_zp=5.0, act_bits=4)
    packed, _ = K.pack_encode(dev((qw - zw.reshape(-1, 1, 1, 1)).astype(np.float32)), dev(zw),
                              dev(np.ones(8, np.float32)), False, None, 2, 0, 3)
    prep_1 = K.qweight_prepare(packed, qw.shape, dev(zw), 2, 0)
    assert prep_1.groups == 1 and K.qconv_kind(prep_1) == "dense"
    codes16, _ = K.act_encode(dev((qa[:, :16] - 5).astype(np.float32)), 1.0, 5.0, 4, False)
    with pytest.raises(SSQError, match="groups"):
        K.qconv(codes16, prep_1, dev(scale), 1, 1, groups=2, act_zp=5.0, act_bits=4)
    # codes whose channel count is not Cig * groups
    with pytest.raises(SSQError, match="do not match"):
        K.qconv(codes16, prep_g, dev(scale), 1, 1, groups=2, act_zp=5.0, act_bits=4)
    with pytest.raises(SSQError, match="zero point"):
        K.qconv(codes, prep_g, dev(scale), 1, 1, groups=2, act_zp=4.5, act_bits=4)
    # a weight zero point that is no integer code is counted by K24, once per channel
    assert int(K.qweight_prepare(packed, qw.shape, dev(zw + 0.5), 2, 0, groups=2).bad.item()) == 8
    dw = rng.integers(0, 4, (20, 1, 3, 3))
    pdw, _ = K.pack_encode(dev(dw.astype(np.float32)), dev(np.zeros(20)), dev(np.ones(20, np.float32)),
                           False, None, 2, 0, 3)
    assert int(K.qweight_prepare(pdw, dw.shape, dev(np.full(20, 0.5)), 2, 0, groups=20).bad.item()) == 20
