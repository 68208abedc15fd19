"""Integer inference kernels on the device (K21 ssq_act_encode, K22 ssq_qweight_prepare, K23
ssq_qconv_i8_fwd): the activation codes are the quantizer's own and off-grid inputs are
counted; the conv equals the host integer reference fp32(I) * s bit for bit over shapes that
hit the K tail, the Co tail, spatial padding and several K steps, at 2..8 bits symmetric or
not, at the accumulator extremes and with identity weights (lane map); and it stays within
the derived fp32 bound of the decoded path's convolution."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_qinfer_host import centred_sum, qrange, ref_output

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def host(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def parity_log(rec):
    """Print the figure and append it to $SSQ_PARITY_LOG (jsonl) when set."""
    print(json.dumps(rec))
    path = os.environ.get("SSQ_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def stored_to_codes(stored, n_bits, sym, C):
    """act_encode's int8 NHWC (channel-padded) -> integer codes in NCHW / (N, C) order."""
    q = host(stored).astype(np.int64) + (qrange(n_bits, sym)[0] + 128)
    return np.moveaxis(q[..., :C], -1, 1)


# ---------------------------------------------------------------- 1. act_encode
@pytest.mark.parametrize("n_bits", [2, 4, 8])
@pytest.mark.parametrize("sym", [False, True])
def test_act_encode_matches_quantizer(K, n_bits, sym):
    g = torch.Generator().manual_seed(100 + n_bits + sym)
    x = (torch.randn(3, 5, 3, 7, generator=g) * 1.5 + (0.0 if sym else 0.7)).cuda()
    # ('mse': a symmetric quantizer's zero point is 0; 'max' puts it at 2^(n_bits-1))
    d, z, _ = K.scale_init(x, n_bits, sym, False, "mse")
    y, codes = K.fake_quant_fwd(x, d, z, n_bits, sym, codes=True)
    want = host(codes.view(torch.int8) if sym else codes).astype(np.int64)
    delta, zp = float(d), float(z)
    lo, hi = qrange(n_bits, sym)
    stored, bad = K.act_encode(y, delta, zp, n_bits, sym)
    assert stored.dtype == torch.int8 and tuple(stored.shape) == (3, 3, 7, 16)    # NHWC, C -> 16
    np.testing.assert_array_equal(stored_to_codes(stored, n_bits, sym, 5), want)
    assert not host(stored)[..., 5:].any()
    assert int(bad.item()) == 0
    # NHWC order spelled out on one element of the non-square plane
    assert int(host(stored)[2, 1, 6, 4]) + lo + 128 == want[2, 4, 1, 6]
    # off the grid by a thousandth of a step: counted, same codes
    off = y + 1e-3 * delta
    stored2, bad2 = K.act_encode(off, delta, zp, n_bits, sym)
    moved = int((host(off).view(np.int32) != host(y).view(np.int32)).sum())
    assert moved > 0 and int(bad2.item()) == moved
    np.testing.assert_array_equal(host(stored2), host(stored))
    # NaN / +-inf: counted, stored as qmin; the counter adds up across calls
    z3 = y.clone()
    z3[0, 0, 0, 0], z3[1, 2, 1, 3], z3[2, 4, 2, 6] = float("nan"), float("inf"), float("-inf")
    stored3, _ = K.act_encode(z3, delta, zp, n_bits, sym, bad=bad2)
    assert int(bad2.item()) == moved + 3
    q3 = stored_to_codes(stored3, n_bits, sym, 5)
    assert q3[0, 0, 0, 0] == lo and q3[1, 2, 1, 3] == lo and q3[2, 4, 2, 6] == lo
    mask = np.ones(want.shape, bool)
    mask[0, 0, 0, 0] = mask[1, 2, 1, 3] = mask[2, 4, 2, 6] = False
    np.testing.assert_array_equal(q3[mask], want[mask])
    # a linear layer's (N, C) input
    stored4, bad4 = K.act_encode(y[:, :, 1, 2].contiguous(), delta, zp, n_bits, sym)
    assert tuple(stored4.shape) == (3, 16) and int(bad4.item()) == 0
    np.testing.assert_array_equal(stored_to_codes(stored4, n_bits, sym, 5), want[:, :, 1, 2])


def test_act_encode_symmetric_max_zero_point(K):
    """The 'max' initialisation of a symmetric quantizer puts the zero point at 2^(n_bits-1),
    above qmax: encodable while it fits the int8 pad value (4 bits), refused at 8 bits."""
    from shiftedscalequantization_amd._capi import SSQError
    x = torch.randn(2, 5, 3, 7, generator=torch.Generator().manual_seed(8)).cuda()
    d, z, _ = K.scale_init(x, 4, True, False, "max")
    assert float(z) == 8.0
    y, codes = K.fake_quant_fwd(x, d, z, 4, True, codes=True)
    stored, bad = K.act_encode(y, float(d), float(z), 4, True)
    np.testing.assert_array_equal(stored_to_codes(stored, 4, True, 5),
                                  host(codes.view(torch.int8)).astype(np.int64))
    assert int(bad.item()) == 0
    d, z, _ = K.scale_init(x, 8, True, False, "max")
    assert float(z) == 128.0
    with pytest.raises(SSQError, match="zero point"):
        K.act_encode(x, float(d), float(z), 8, True)


# ---------------------------------------------------------------- 2./5. qconv
# (N, Ci, H, W, Co, R, stride, pad); H = None: a linear (N, Ci) -> (N, Co)
SHAPES = {
    "k27": (2, 3, 5, 5, 5, 3, 1, 1),
    "k180_tails": (3, 20, 9, 9, 33, 3, 2, 1),
    "exact_tiles": (2, 64, 8, 8, 16, 1, 1, 0),
    "ci130_s2": (1, 130, 7, 7, 17, 1, 2, 0),
    "nonsquare": (2, 16, 6, 10, 48, 3, 1, 1),
    "k1440": (2, 160, 4, 4, 32, 3, 1, 1),
    "7x7": (1, 8, 9, 9, 4, 7, 2, 3),
    "linear": (5, 70, None, None, 10, 1, 1, 0),
}
# (weight bits, weight sym, act bits, act sym): every shape meets 8/8 and 2/2, both
# symmetries; the other widths rotate over the shapes
ALWAYS = [(8, False, 8, False), (8, True, 8, True), (2, False, 2, False), (2, True, 2, True)]
ROTATE = [(3, False, 4, True), (4, True, 4, False), (3, True, 8, False), (4, False, 2, True),
          (8, False, 4, False), (2, False, 8, True), (1, False, 4, False), (5, True, 3, True)]
CASES = [(name, bits) for i, name in enumerate(SHAPES)
         for bits in ALWAYS + [ROTATE[i % len(ROTATE)], ROTATE[(i + 3) % len(ROTATE)]]]


def encode_weight(K, qw, zw, d1, wb, wsym):
    """Integer codes -> W_hat = (q - zp) * d1 -> the export's packed codes -> K22."""
    wlo, whi = qrange(wb, wsym)
    what = ((qw - zw.reshape((-1,) + (1,) * (qw.ndim - 1))).astype(np.float32)
            * d1.reshape((-1,) + (1,) * (qw.ndim - 1)))
    packed, bad = K.pack_encode(dev(what), dev(zw), dev(d1), False, None, wb, wlo, whi)
    assert bad == 0
    prep = K.qweight_prepare(packed, qw.shape, dev(zw), wb, wlo)
    assert int(prep.bad.item()) == 0
    return what, prep


@functools.lru_cache(maxsize=None)
def run_case(name, bits):
    """Device output and host references of one case, computed once for tests 2 and 5."""
    from shiftedscalequantization_amd import kernels as K
    N, Ci, H, W, Co, R, stride, pad = SHAPES[name]
    wb, wsym, ab, asym = bits
    linear = H is None
    rng = np.random.default_rng(zlib.crc32(repr((name, bits)).encode()))
    alo, ahi = qrange(ab, asym)
    wlo, whi = qrange(wb, wsym)
    xs = (N, Ci) if linear else (N, Ci, H, W)
    ws = (Co, Ci) if linear else (Co, Ci, R, R)
    qa = rng.integers(alo, ahi + 1, xs)
    za = int(rng.integers(alo, ahi + 1))
    qw = rng.integers(wlo, whi + 1, ws)
    zw = rng.integers(wlo, whi + 1, Co)
    da = np.float32(rng.uniform(0.01, 0.2))
    d1 = rng.uniform(1e-3, 2e-2, Co).astype(np.float32)
    xhat = (qa - za).astype(np.float32) * da
    what, prep = encode_weight(K, qw, zw, d1, wb, wsym)
    scale = da * d1                                     # fp32(delta_a * d1[co])
    assert scale.dtype == np.float32
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = K.qconv(dev(xhat), prep, dev(scale), stride, pad, act_zp=float(za), act_bits=ab,
                act_sym=asym, act_delta=float(da), bad=bad)
    q4 = (lambda a: a.reshape(a.shape + (1, 1))) if linear else (lambda a: a)
    ref = ref_output(q4(qa), za, q4(qw), zw, scale, stride, pad)
    xt, wt = torch.from_numpy(q4(xhat)).double(), torch.from_numpy(q4(what)).double()
    ref64 = F.conv2d(xt, wt, stride=stride, padding=pad).numpy()
    A = F.conv2d(xt.abs(), wt.abs(), stride=stride, padding=pad).numpy()
    out = host(y)
    assert out.shape == ((N, Co) if linear else ref.shape)
    return out.reshape(ref.shape), ref, ref64, A, int(bad.item())


@pytest.mark.parametrize("name,bits", CASES)
def test_qconv_bit_exact(K, name, bits):
    out, ref, _, _, bad = run_case(name, bits)
    assert bad == 0
    np.testing.assert_array_equal(out.view(np.int32), ref.view(np.int32))


def test_cases_cover_every_width():
    assert {b[0] for _, b in CASES} >= {2, 3, 4, 8} and {b[2] for _, b in CASES} >= {2, 4, 8}
    for name in SHAPES:
        assert {(8, False, 8, False), (2, False, 2, False)} <= {b for n, b in CASES if n == name}


@pytest.mark.parametrize("name", list(SHAPES))
def test_qconv_within_fp32_bound_of_decoded_path(K, name):
    """|y - conv64(x_hat, W_hat)| <= 2^-21 * conv64(|x_hat|, |W_hat|) elementwise: one rounding
    each in x_hat and W_hat, at most three in the integer epilogue (convert, delta_a * d1,
    product) = 5 * 2^-24 * A; 8 * 2^-24 covers the second-order terms."""
    worst = 0.0
    for n, bits in CASES:
        if n != name:
            continue
        out, _, ref64, A, _ = run_case(n, bits)
        err = np.abs(out.astype(np.float64) - ref64)
        assert np.all(err <= 2.0 ** -21 * A), (n, bits, float((err / np.maximum(A, 1e-300)).max()))
        nz = A > 0
        if nz.any():
            worst = max(worst, float((err[nz] / A[nz]).max()))
    parity_log({"test": "qconv_vs_fp64", "shape": name, "worst_err_over_A_in_2^-24": worst * 2 ** 24,
                "bound_in_2^-24": 8.0})


# ---------------------------------------------------------------- 3. extremes
def _run_codes(K, qa, za, qw, zw, scale, stride, pad, ab=8, asym=False, wb=8, wsym=False):
    """Straight from integer codes (delta = 1 so x_hat = q - z exactly)."""
    what, prep = encode_weight(K, qw, zw, np.ones(qw.shape[0], np.float32), wb, wsym)
    xhat = (qa - za).astype(np.float32)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = K.qconv(dev(xhat), prep, dev(scale), stride, pad, act_zp=float(za), act_bits=ab,
                act_sym=asym, act_delta=1.0, bad=bad)
    assert int(bad.item()) == 0
    return host(y)


def test_qconv_extremes_k1440(K):
    N, Ci, H, W, Co, R = 2, 160, 4, 4, 32, 3
    scale = np.linspace(0.5, 1.5, Co).astype(np.float32)
    # all codes at the top, zero points at the bottom: |I| = 1440 * 255^2 > 2^24, the
    # conversion rounds
    qa, qw = np.full((N, Ci, H, W), 255), np.full((Co, Ci, R, R), 255)
    zw = np.zeros(Co, np.int64)
    ref = ref_output(qa, 0, qw, zw, scale, 1, 1)
    I = centred_sum(qa, 0, qw, zw, 1, 1)
    assert I.max() > 2 ** 24
    np.testing.assert_array_equal(_run_codes(K, qa, 0, qw, zw, scale, 1, 1).view(np.int32),
                                  ref.view(np.int32))
    # near the top with odd sums: fp32(I) itself rounds
    rng = np.random.default_rng(11)
    qa, qw = rng.integers(253, 256, (N, Ci, H, W)), rng.integers(253, 256, (Co, Ci, R, R))
    I = centred_sum(qa, 0, qw, zw, 1, 1)
    assert I.max() > 2 ** 24 and np.any(I.astype(np.float32).astype(np.int64) != I)
    ref = ref_output(qa, 0, qw, zw, scale, 1, 1)
    np.testing.assert_array_equal(_run_codes(K, qa, 0, qw, zw, scale, 1, 1).view(np.int32),
                                  ref.view(np.int32))
    # all codes at the bottom, zero points at the top
    qa, qw = np.zeros((N, Ci, H, W), np.int64), np.zeros((Co, Ci, R, R), np.int64)
    zw = np.full(Co, 255)
    ref = ref_output(qa, 255, qw, zw, scale, 1, 1)
    assert ref.max() == np.float32(1440 * 255 * 255) * scale.max()
    np.testing.assert_array_equal(_run_codes(K, qa, 255, qw, zw, scale, 1, 1).view(np.int32),
                                  ref.view(np.int32))
    # alternating-sign centred weights against a constant input: I = 0 in the interior
    qa = np.full((N, Ci, H, W), 255)
    sign = np.where(np.arange(Ci) % 2 == 0, 1, -1).reshape(1, Ci, 1, 1)
    zw = np.full(Co, 128)
    qw = 128 + 127 * sign * np.ones((Co, Ci, R, R), np.int64)
    ref = ref_output(qa, 0, qw, zw, scale, 1, 1)
    assert not centred_sum(qa, 0, qw, zw, 1, 1).any()
    out = _run_codes(K, qa, 0, qw, zw, scale, 1, 1)
    np.testing.assert_array_equal(out.view(np.int32), ref.view(np.int32))
    assert not out.any()


# ---------------------------------------------------------------- 4. identity weights
def test_qconv_identity_weights_lane_map(K):
    """q_w - z_w = delta(co, ci) with asymmetric random activation codes: the output is
    (q_a - z_a) * s[co], so a row / column swap or a wrong lane map shows."""
    rng = np.random.default_rng(7)
    Cc = 32
    zw = rng.integers(0, 255, Cc)
    qw = (zw.reshape(-1, 1) + np.eye(Cc, dtype=np.int64)).reshape(Cc, Cc, 1, 1)
    qa = rng.integers(0, 256, (2, Cc, 3, 5))
    za = 37
    scale = rng.uniform(0.5, 2.0, Cc).astype(np.float32)
    out = _run_codes(K, qa, za, qw, zw, scale, 1, 0)
    want = (qa - za).astype(np.float32) * scale.reshape(1, -1, 1, 1)
    np.testing.assert_array_equal(out.view(np.int32), want.view(np.int32))


def test_qconv_takes_codes_and_checks_arguments(K):
    from shiftedscalequantization_amd._capi import SSQError
    rng = np.random.default_rng(3)
    qa, qw = rng.integers(0, 16, (1, 8, 4, 4)), rng.integers(0, 4, (4, 8, 3, 3))
    zw, scale = rng.integers(0, 4, 4), np.ones(4, np.float32)
    what, prep = encode_weight(K, qw, zw, np.ones(4, np.float32), 2, False)
    codes, bad = K.act_encode(dev((qa - 5).astype(np.float32)), 1.0, 5.0, 4, False)
    y = K.qconv(codes, prep, dev(scale), 1, 1, act_zp=5.0, act_bits=4)
    ref = ref_output(qa, 5, qw, zw, scale, 1, 1)
    np.testing.assert_array_equal(host(y).view(np.int32), ref.view(np.int32))
    with pytest.raises(SSQError, match="groups"):
        K.qconv(codes, prep, dev(scale), 1, 1, groups=2, act_zp=5.0, act_bits=4)
    with pytest.raises(SSQError, match="zero point"):
        K.qconv(codes, prep, dev(scale), 1, 1, act_zp=4.5, act_bits=4)
    # a weight zero point that is no integer code is counted by K22
    packed, _ = K.pack_encode(dev(what), dev(zw), dev(np.ones(4, np.float32)), False, None, 2, 0, 3)
    assert int(K.qweight_prepare(packed, qw.shape, dev(zw + 0.5), 2, 0).bad.item()) == 4
