"""Integer inference of column-scaled weights on the device (ssq_qweight_prepare_colscale,
ssq_qweight_prepare_grouped_colscale, the CENTRED instantiations of K23): codes, zero points and
the integer column factors k are built directly (no search), and y.view(int32) must EQUAL the
host int64 reference fp32(I) * s[co], I = sum (q_a - z_a)(q_w - z_w[co]) k[j],
s[co] = fp32(fp32(delta_a * d1[co]) / fp32(L)).  Shapes: batch 2 on a 9x7 plane (M = 126, no
tile multiple): 3x3 at stride 1 and 2 with Ci = 24 (padded to 32) and Co = 72 (crosses the 64
tile), 1x1, 7x7 on Ci = 3, a linear, depthwise 3x3, grouped g = 3.  Weights W2 / L = 32,
W3 / L = 16, W4 / L = 8 with asymmetric per-channel zero points; activations at 4 and 8 bits,
symmetric and not.  Then the accumulator extreme, the int8 range refusal, bit identity of the
shift-and-correct and centred instantiations on one blob (fp32, codes, both residual forms),
the emitted codes against qconv -> K13 -> act_encode, and the 9 * 2^-24 bound against the
decoded path's fp64 convolution."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_qinfer_carry_gpu import fp32_epilogue, pick_quantizer
from test_qinfer_colscale_host import (centred_operand, colscale_scale, colscale_sum,
                                       ref_output)
from test_qinfer_host import qrange

pytestmark = pytest.mark.gpu
F32 = np.float32


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


# (N, C, H, W, Co, R, stride, pad, groups); H = None: a linear (N, C) -> (N, Co)
SHAPES = {
    "3x3_s1": (2, 24, 9, 7, 72, 3, 1, 1, 1),
    "3x3_s2": (2, 24, 9, 7, 72, 3, 2, 1, 1),
    "1x1": (2, 40, 9, 7, 16, 1, 1, 0, 1),
    "7x7": (2, 3, 9, 7, 8, 7, 1, 3, 1),
    "linear": (5, 100, None, None, 10, 1, 1, 0, 1),
    "dw3x3": (2, 24, 9, 7, 24, 3, 1, 1, 24),
    "g3": (2, 24, 9, 7, 72, 3, 1, 1, 3),
}
FIRST = "3x3_s1"
WEIGHTS = [(2, 32), (3, 16), (4, 8)]                            # (n_bits_w, L)
ACTS = [(4, False), (4, True), (8, False), (8, True)]           # (n_bits_a, sym)
CASES = [(n, w, a) for n in SHAPES for w in WEIGHTS for a in ACTS]


def encode_colscale(K, qw, zw, d1, k, L, wb, groups=1):
    """Integer codes -> W_hat = ((q - zp) * d1) * fp32(k / L) -> the export's packed codes ->
    the column-scaled prepare.  qw is (Co, Cig, R, S) (a linear's (Co, Ci, 1, 1))."""
    whi = 2 ** wb - 1
    c = (k.astype(F32) / F32(L)).reshape((1,) + qw.shape[1:])
    what = ((qw - zw.reshape(-1, 1, 1, 1)).astype(F32) * d1.reshape(-1, 1, 1, 1)) * c
    assert what.dtype == F32
    packed, bad = K.pack_encode(dev(what), dev(zw), dev(d1), False, dev(c.reshape(-1)), wb, 0, whi)
    assert bad == 0
    return what, packed


def draw_weight(rng, ws, wb, L):
    """Codes over the whole range, asymmetric per-channel zero points inside it, k in 1..L with
    a column at each end."""
    whi = 2 ** wb - 1
    qw = rng.integers(0, whi + 1, ws)
    zw = rng.integers(0, whi + 1, ws[0])
    zw[0], zw[-1] = 0, whi
    k = rng.integers(1, L + 1, int(np.prod(ws[1:])))
    k[0], k[-1] = 1, L
    return qw, zw, k


@functools.lru_cache(maxsize=None)
def run_case(name, wform, aform):
    """Device output and host references of one case, computed once for the bit-exact and the
    bound tests."""
    from shiftedscalequantization_amd import kernels as K
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES[name]
    wb, L = wform
    ab, asym = aform
    linear = H is None
    rng = np.random.default_rng(zlib.crc32(repr((name, wform, aform)).encode()))
    alo, ahi = qrange(ab, asym)
    xs = (N, Cc, 1, 1) if linear else (N, Cc, H, W)
    qa = rng.integers(alo, ahi + 1, xs)
    za = int(rng.integers(alo, ahi + 1))
    qw, zw, k = draw_weight(rng, (Co, Cc // G, R, R), wb, L)
    assert np.abs(centred_operand(qw, zw, k)).max() <= 127
    da = F32(rng.uniform(0.01, 0.2))
    d1 = rng.uniform(1e-3, 2e-2, Co).astype(F32)
    xhat = (qa - za).astype(F32) * da
    what, packed = encode_colscale(K, qw, zw, d1, k, L, wb, G)
    wshape = (Co, Cc) if linear else qw.shape
    prep = K.qweight_prepare(packed, wshape, dev(zw), wb, 0, groups=G, kcol=torch.from_numpy(k))
    assert prep.centred and int(prep.bad.item()) == 0
    scale = colscale_scale(da, d1, L)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    x = dev(xhat.reshape(N, Cc) if linear else xhat)
    y = K.qconv(x, prep, dev(scale), stride, pad, groups=G, act_zp=float(za), act_bits=ab,
                act_sym=asym, act_delta=float(da), bad=bad)
    ref = ref_output(qa, za, qw, zw, k, scale, stride, pad, G)
    xt, wt = torch.from_numpy(xhat).double(), torch.from_numpy(what).double()
    ref64 = F.conv2d(xt, wt, stride=stride, padding=pad, groups=G).numpy()
    A = F.conv2d(xt.abs(), wt.abs(), stride=stride, padding=pad, groups=G).numpy()
    out = host(y)
    assert out.shape == ((N, Co) if linear else ref.shape)
    return out.reshape(ref.shape), ref, ref64, A, int(bad.item())


@pytest.mark.parametrize("name,wform,aform", CASES)
def test_colscale_bit_exact(K, name, wform, aform):
    out, ref, _, _, bad = run_case(name, wform, aform)
    assert bad == 0
    assert ref.any()
    np.testing.assert_array_equal(out.view(np.int32), ref.view(np.int32))


@pytest.mark.parametrize("name", list(SHAPES))
def test_colscale_within_fp32_bound_of_decoded_path(K, name):
    """|y - conv64(x_hat, W_hat)| <= 9 * 2^-24 * conv64(|x_hat|, |W_hat|) elementwise: one
    rounding in x_hat, three in W_hat ((q - z) * d1, * c, c = fp32(k / L) itself), four in the
    integer epilogue (fp32(I), delta_a * d1, / L, the product); the ninth unit covers the
    second-order terms."""
    worst = 0.0
    for n, wform, aform in CASES:
        if n != name:
            continue
        out, _, ref64, A, _ = run_case(n, wform, aform)
        err = np.abs(out.astype(np.float64) - ref64)
        nz = A > 0
        ratio = float((err[nz] / A[nz]).max()) if nz.any() else 0.0
        print({"case": (n, wform, aform), "err_over_A_in_2^-24": ratio * 2 ** 24})
        assert np.all(err <= 9 * 2.0 ** -24 * A), (n, wform, aform, ratio * 2 ** 24)
        worst = max(worst, ratio)
    parity_log({"test": "colscale_qconv_vs_fp64", "shape": name,
                "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 9.0})


def test_cases_cover_the_forms():
    assert {(n, w) for n, w, _ in CASES} == {(n, w) for n in SHAPES for w in WEIGHTS}
    assert {a for _, _, a in CASES} == set(ACTS)
    for wb, L in WEIGHTS:
        assert (2 ** wb - 1) * L <= 127 < (2 ** wb - 1) * 2 * L


# ---------------------------------------------------------------- accumulator extreme
def test_accumulator_extreme(K):
    """Ci = 512, 3x3 on a 3x3 plane: every m = +-127 ((q - z) = +-1, k = 127), every activation
    at qmax with z_a = qmin: |I| = 4608 * 255 * 127 > 2^24 in the centre, the conversion rounds;
    one channel all +, one all -, one all + but a single tap, the rest mixed."""
    N, Ci, Co = 1, 512, 8
    rng = np.random.default_rng(5)
    sign = rng.integers(0, 2, (Co, Ci, 3, 3)) * 2 - 1
    sign[0], sign[1], sign[2] = 1, -1, 1
    sign[2, 0, 1, 1] = -1                                       # 2 * odd * 32385: fp32(I) rounds
    zw = np.ones(Co, np.int64)
    qw = 1 + sign                                               # W2 codes 0 / 2 around z = 1
    k = np.full(Ci * 9, 127)
    m = centred_operand(qw, zw, k)
    assert set(np.unique(m)) == {-127, 127}
    qa = np.full((N, Ci, 3, 3), 255)
    d1 = np.linspace(0.5, 1.5, Co).astype(F32)
    what, packed = encode_colscale(K, qw, zw, d1, k, 127, 2)
    prep = K.qweight_prepare(packed, qw.shape, dev(zw), 2, 0, kcol=torch.from_numpy(k))
    assert int(prep.bad.item()) == 0
    scale = colscale_scale(F32(1.0), d1, 127)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = K.qconv(dev(qa.astype(F32)), prep, dev(scale), 1, 1, act_zp=0.0, act_bits=8,
                act_delta=1.0, bad=bad)
    I = colscale_sum(qa, 0, qw, zw, k, 1, 1)
    assert I.max() == 4608 * 255 * 127 > 2 ** 24 and I.min() == -I.max()
    assert np.any(I.astype(F32).astype(np.int64) != I)
    ref = ref_output(qa, 0, qw, zw, k, scale, 1, 1)
    assert int(bad.item()) == 0
    np.testing.assert_array_equal(host(y).view(np.int32), ref.view(np.int32))


# ---------------------------------------------------------------- range refusal
@pytest.mark.parametrize("name", ["3x3_s1", "dw3x3", "g3"])
def test_prepare_counts_elements_that_leave_int8(K, name):
    """W4 with L = 16: (q - z) * k reaches 15 * 16 = 240; the prepare counts every real element
    with |m| > 127, and none when the same codes meet L = 8."""
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES[name]
    rng = np.random.default_rng(17)
    ws = (Co, Cc // G, R, R)
    qw, zw, k = draw_weight(rng, ws, 4, 16)
    over = int((np.abs(centred_operand(qw, zw, k)) > 127).sum())
    assert over > 0
    d1 = np.full(Co, 0.01, F32)
    _, packed = encode_colscale(K, qw, zw, d1, k, 16, 4, G)
    prep = K.qweight_prepare(packed, ws, dev(zw), 4, 0, groups=G, kcol=torch.from_numpy(k))
    assert int(prep.bad.item()) == over
    k8 = np.minimum(k, 8)
    _, packed = encode_colscale(K, qw, zw, d1, k8, 8, 4, G)
    prep = K.qweight_prepare(packed, ws, dev(zw), 4, 0, groups=G, kcol=torch.from_numpy(k8))
    assert int(prep.bad.item()) == 0
    # a zero point that is no integer code is still counted, once per channel
    prep = K.qweight_prepare(packed, ws, dev(zw + 0.5), 4, 0, groups=G, kcol=torch.from_numpy(k8))
    assert int(prep.bad.item()) >= Co


def test_wrapper_refuses_bad_kcol(K):
    from shiftedscalequantization_amd._capi import SSQError
    packed = torch.zeros(64, dtype=torch.uint8, device="cuda")
    zp = torch.zeros(4, device="cuda")
    for kcol in (torch.ones(7, dtype=torch.int32), torch.zeros(8, dtype=torch.int32),
                 torch.full((8,), 128, dtype=torch.int32), torch.ones(8)):
        with pytest.raises(SSQError, match="kcol"):
            K.qweight_prepare(packed, (4, 8, 1, 1), zp, 4, 0, kcol=kcol)


# ---------------------------------------------------------------- one blob, two instantiations
def first_layer(K, seed, ab=4, asym=False):
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES[FIRST]
    rng = np.random.default_rng(seed)
    alo, ahi = qrange(ab, asym)
    qa = rng.integers(alo, ahi + 1, (N, Cc, H, W))
    za = int(rng.integers(alo, ahi + 1))
    qw, zw, k = draw_weight(rng, (Co, Cc, R, R), 2, 32)
    da = F32(0.125)
    d1 = rng.uniform(1e-3, 2e-2, Co).astype(F32)
    _, packed = encode_colscale(K, qw, zw, d1, k, 32, 2)
    prep = K.qweight_prepare(packed, qw.shape, dev(zw), 2, 0, kcol=torch.from_numpy(k))
    assert prep.centred and int(prep.bad.item()) == 0
    codes, nb = K.act_encode(dev((qa - za).astype(F32) * da), float(da), float(za), ab, asym)
    assert int(nb.item()) == 0
    scale = colscale_scale(da, d1, 32)
    kw = dict(act_zp=float(za), act_bits=ab, act_sym=asym)
    return rng, prep, codes, scale, kw, (qa, za, qw, zw, k)


@pytest.mark.parametrize("residual", ["none", "fp32", "codes"])
def test_sa_and_centred_instantiations_are_bit_identical(K, monkeypatch, residual):
    """The same centred blob through the shift-and-correct kernels (cwz = 0 in the blob) and
    through the CENTRED ones: identical bytes, for the fp32 output and for emitted codes with
    and without a residual in both residual forms."""
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES[FIRST]
    rng, prep, codes, scale, kw, ints = first_layer(K, 41)
    bias = dev(rng.normal(0, 0.05, Co).astype(F32))
    gamma, phi = dev(rng.uniform(0.5, 1.5, Co).astype(F32)), dev(rng.normal(0, 0.05, Co).astype(F32))
    ref = ref_output(*ints, scale, stride, pad)
    d, z = pick_quantizer(ref, 4, False)
    dims = ref.shape
    res = None
    if residual == "fp32":
        res = dev(rng.normal(0, float(ref.std()), dims).astype(F32))
    elif residual == "codes":
        rc = dev(rng.integers(-128, 128, (N, dims[2], dims[3], 80)), torch.int8)
        rc[..., Co:] = 0
        res = K.carried(rc, dims, float(ref.std()) / 64, 131.0, 8, False)
    outs = {}
    for centred in (False, True):
        monkeypatch.setattr(K, "QCONV_CENTRED", centred)
        want = "ssq_qconv_i8_centred_fwd" if centred else "ssq_qconv_i8_fwd"
        assert K._qconv_fn(prep, 1, "fwd") == want
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        y = K.qconv(codes, prep, dev(scale), stride, pad, **kw)
        c = K.qconv_codes(codes, prep, dev(scale), stride, pad, bias=bias, gamma=gamma, phi=phi,
                          relu=1, out_delta=float(d), out_zp=float(z), out_bits=4, bad=bad,
                          residual=res, **kw)
        assert int(bad.item()) == 0
        outs[centred] = (host(y), host(c))
    np.testing.assert_array_equal(outs[True][0].view(np.int32), ref.view(np.int32))
    np.testing.assert_array_equal(outs[False][0].view(np.int32), outs[True][0].view(np.int32))
    assert outs[True][1].dtype == np.int8 and outs[True][1].any()
    np.testing.assert_array_equal(outs[False][1], outs[True][1])


@pytest.mark.parametrize("aform", ACTS)
def test_centred_emitted_codes_equal_the_uncarried_route(K, aform):
    """The centred code-emitting kernel on the first shape, bias and affine on, ReLU: the bytes
    act_encode derives from the K13 epilogue of qconv's fp32 output, nothing off the grid."""
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES[FIRST]
    rng, prep, codes, scale, kw, ints = first_layer(K, 43, *aform)
    assert K.QCONV_CENTRED and K._qconv_fn(prep, 1, "codes_fwd") == "ssq_qconv_i8_centred_codes_fwd"
    bias = rng.normal(0, 0.05, Co).astype(F32)
    gamma, phi = rng.uniform(0.5, 1.5, Co).astype(F32), rng.normal(0, 0.05, Co).astype(F32)
    ref = ref_output(*ints, scale, stride, pad)
    t = np.maximum((ref + bias.reshape(1, -1, 1, 1)) * gamma.reshape(1, -1, 1, 1)
                   + phi.reshape(1, -1, 1, 1), 0)
    for ob, osym in ((4, False), (8, True)):
        d, z = pick_quantizer(t, ob, osym)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        fused = K.qconv_codes(codes, prep, dev(scale), stride, pad, bias=dev(bias), gamma=dev(gamma),
                              phi=dev(phi), relu=1, out_delta=float(d), out_zp=float(z),
                              out_bits=ob, out_sym=osym, bad=bad, **kw)
        y = K.qconv(codes, prep, dev(scale), stride, pad, **kw)
        yq = fp32_epilogue(K, y, dev(bias), dev(gamma), dev(phi), 1, d, z, ob, osym)
        plain, bad_b = K.act_encode(yq, float(d), float(z), ob, osym)
        assert int(bad.item()) == 0 and int(bad_b.item()) == 0
        got = host(fused)
        lo, hi = qrange(ob, osym)
        real = got[..., :Co].astype(np.int64) + lo + 128
        assert (real == lo).any() and (real == hi).any() and ((real > lo) & (real < hi)).any()
        assert not got[..., Co:].any()
        np.testing.assert_array_equal(got, host(plain))


def test_existing_consumers_run_a_centred_blob(K):
    """K26 (grouped) and K25 (depthwise) emit codes from a column-scaled blob through their
    unchanged kernels: equal to their own fp32 output -> K13 -> act_encode."""
    for name in ("g3", "dw3x3"):
        N, Cc, H, W, Co, R, stride, pad, G = SHAPES[name]
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        qa, za = rng.integers(0, 16, (N, Cc, H, W)), 5
        qw, zw, k = draw_weight(rng, (Co, Cc // G, R, R), 3, 16)
        d1 = rng.uniform(1e-3, 2e-2, Co).astype(F32)
        _, packed = encode_colscale(K, qw, zw, d1, k, 16, 3, G)
        prep = K.qweight_prepare(packed, qw.shape, dev(zw), 3, 0, groups=G, kcol=torch.from_numpy(k))
        assert int(prep.bad.item()) == 0
        scale = colscale_scale(F32(0.125), d1, 16)
        codes, _ = K.act_encode(dev((qa - za).astype(F32) * F32(0.125)), 0.125, float(za), 4, False)
        kw = dict(groups=G, act_zp=float(za), act_bits=4)
        ref = ref_output(qa, za, qw, zw, k, scale, stride, pad, G)
        d, z = pick_quantizer(np.maximum(ref, 0), 4, False)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        fused = K.qconv_codes(codes, prep, dev(scale), stride, pad, relu=1, out_delta=float(d),
                              out_zp=float(z), out_bits=4, bad=bad, **kw)
        y = K.qconv(codes, prep, dev(scale), stride, pad, **kw)
        np.testing.assert_array_equal(host(y).view(np.int32), ref.view(np.int32))
        yq = fp32_epilogue(K, y, None, None, None, 1, d, z, 4, False)
        plain, bad_b = K.act_encode(yq, float(d), float(z), 4, False)
        assert int(bad.item()) == 0 and int(bad_b.item()) == 0
        np.testing.assert_array_equal(host(fused), host(plain))
