"""The two-digit weight operand on the device (ssq_qweight_prepare_wide, K23's WIDE
instantiations): a scaled weight whose centred integer m = (q - z) * k leaves int8 runs as
m = 128 h + l on two int8 planes.  y.view(int32) must EQUAL the host int64 reference
fp32(I) * s[co] for W4 / L32 and W8 / L32 per-(co, ci) scales and for a W4 column scale at
L = 1024, on a 3x3 (Ci = 70, Co = 72, batch 2, plane 9x7: K, channel and pixel tails) and a 1x1
(one k step); the code-emitting form and both residual forms must equal the uncarried route
(the fp32 form -> the K13 epilogue -> act_encode).  Then the accumulator extremes (every
m = +-16319 against activations at qmax and at qmin, K = 4608, |I| > 2^31), bit identity with the
centred int8 instantiation on a blob both hold (SSQ_QCONV_WIDE=1), the prepare's count, and the
wrapper's refusals (split-K, K26, K30)."""
import functools
import types
import zlib

import numpy as np
import pytest
import torch

from test_qinfer_carry_gpu import pick_quantizer
from test_qinfer_colscale_gpu import encode_colscale
from test_qinfer_colscale_host import centred_operand
from test_qinfer_host import qrange
from test_qinfer_perci_gpu import SHAPES, dev, draw_perci_weight, encode_perci, host
from test_qinfer_perci_host import (grid_scale, operand_sum, perci_operand, predicate, ref_output,
                                    wide_sum)

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


WEIGHTS = ["perci_w4_l32", "perci_w8_l32", "col_w4_l1024"]
FORMS = ["fp32", "codes", "res_fp32", "res_codes"]
NAMES = ["3x3_s1", "1x1"]


def draw_wide_weight(K, rng, ws, wform):
    """(wb, qw, zw, W_hat, packed, m, L, base[co], prepare keywords) of one weight form, its grid
    found from the stored floats."""
    Co, Ci = ws[:2]
    if wform.startswith("perci"):
        wb = 4 if "w4" in wform else 8
        qw, zw, wscale = draw_perci_weight(rng, ws, wb)
        assert K.perci_grid(torch.from_numpy(wscale), Co, Ci, 127)[0] == 32
        L, base, k = K.perci_grid(torch.from_numpy(wscale), Co, Ci, K.QWIDE_MAX)
        predicate(wscale, L, base, k, K.QWIDE_MAX)
        what, packed = encode_perci(K, qw, zw, wscale, wb)
        return wb, qw, zw, what, packed, perci_operand(qw, zw, k.numpy()), L, base.numpy(), dict(kfac=k)
    wb, whi = 4, 15
    qw = rng.integers(0, whi + 1, ws)
    zw = rng.integers(0, whi + 1, Co)
    zw[0], zw[-1] = 0, whi
    k = rng.integers(1, 1025, int(np.prod(ws[1:])))
    k[0], k[-1] = 1, 1024
    d1 = rng.uniform(1e-3, 2e-2, Co).astype(F32)
    what, packed = encode_colscale(K, qw, zw, d1, k, 1024, wb)
    c = torch.from_numpy(k.astype(F32) / F32(1024))
    assert K.colscale_grid(c) is None
    L, kk = K.colscale_grid(c, K.QWIDE_MAX_L, K.QWIDE_MAX)
    assert L == 1024 and np.array_equal(kk.numpy(), k)
    return wb, qw, zw, what, packed, centred_operand(qw, zw, k), L, d1, dict(kcol=kk)


@functools.lru_cache(maxsize=None)
def layer(name, wform):
    """One wide layer: the prepared blob, the encoded input and the host reference."""
    from shiftedscalequantization_amd import kernels as K
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(repr((name, wform)).encode()))
    ab, asym = (8, False) if "w8" in wform else (4, True)
    alo, ahi = qrange(ab, asym)
    qa = rng.integers(alo, ahi + 1, (N, Cc, H, W))
    za = int(rng.integers(alo, ahi + 1))
    wb, qw, zw, what, packed, m, L, base, kw = draw_wide_weight(K, rng, (Co, Cc, R, R), wform)
    assert 127 < np.abs(m).max() <= K.QWIDE_MAX
    # the int8 blob does not hold it (where its factors fit at all)
    if max(int(v.max()) for v in kw.values()) <= 127:
        narrow = K.qweight_prepare(packed, qw.shape, dev(zw), wb, 0, **kw)
        assert int(narrow.bad.item()) == int((np.abs(m) > 127).sum())
    prep = K.qweight_prepare_scaled(packed, qw.shape, dev(zw), wb, 0, wide=True, **kw)
    assert prep.wide and prep.centred and int(prep.bad.item()) == 0
    da = F32(rng.uniform(0.01, 0.2))
    codes, nb = K.act_encode(dev((qa - za).astype(F32) * da), float(da), float(za), ab, asym)
    assert int(nb.item()) == 0
    scale = grid_scale(da, base, L)
    I = operand_sum(qa, za, m, stride, pad)
    np.testing.assert_array_equal(I, wide_sum(qa, za, m, stride, pad, alo))
    return types.SimpleNamespace(prep=prep, codes=codes, scale=scale, ref=ref_output(I, scale),
                                 kw=dict(act_zp=float(za), act_bits=ab, act_sym=asym), rng=rng,
                                 geo=(stride, pad), Co=Co)


def emitted_and_uncarried(K, Ly, form, prep=None):
    """(the code-emitting kernel's bytes, the uncarried route's) for `form` on layer `Ly`."""
    prep = Ly.prep if prep is None else prep
    stride, pad = Ly.geo
    Co, rng = Ly.Co, np.random.default_rng(7)
    bias = dev(rng.normal(0, 0.05, Co).astype(F32))
    gamma, phi = dev(rng.uniform(0.5, 1.5, Co).astype(F32)), dev(rng.normal(0, 0.05, Co).astype(F32))
    dims = Ly.ref.shape
    res = res_plain = None
    if form == "res_fp32":
        res = res_plain = dev(rng.normal(0, float(Ly.ref.std()), dims).astype(F32))
    elif form == "res_codes":
        rc = dev(rng.integers(-128, 128, (dims[0], dims[2], dims[3], -(-Co // 16) * 16)), torch.int8)
        rc[..., Co:] = 0
        rq = (float(Ly.ref.std()) / 64, 131.0, 8, False)
        res, res_plain = K.carried(rc, dims, *rq), K.act_decode(rc, Co, *rq)
    d, z = pick_quantizer(np.maximum(Ly.ref, 0), 4, False)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    fused = K.qconv_codes(Ly.codes, prep, dev(Ly.scale), stride, pad, bias=bias, gamma=gamma,
                          phi=phi, relu=1, out_delta=float(d), out_zp=float(z), out_bits=4, bad=bad,
                          residual=res, **Ly.kw)
    y = K.qconv(Ly.codes, prep, dev(Ly.scale), stride, pad, **Ly.kw)
    q = types.SimpleNamespace(delta=dev(np.array([d], F32)), zero_point=dev(np.array([z], F32)),
                              n_bits=4, sym=False)
    with torch.no_grad():
        yq = K.epilogue(y, bias, gamma, phi, res_plain, 1, q)
    plain, bad_b = K.act_encode(yq, float(d), float(z), 4, False)
    assert int(bad.item()) == 0 and int(bad_b.item()) == 0
    return host(fused), host(plain)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wform", WEIGHTS)
@pytest.mark.parametrize("name", NAMES)
def test_wide_bit_exact(K, name, wform, form):
    Ly = layer(name, wform)
    stride, pad = Ly.geo
    if form == "fp32":
        assert K._qconv_fn(Ly.prep, 1, "fwd") == "ssq_qconv_i8_wide_fwd"
        y = K.qconv(Ly.codes, Ly.prep, dev(Ly.scale), stride, pad, **Ly.kw)
        assert Ly.ref.any()
        np.testing.assert_array_equal(host(y).view(np.int32), Ly.ref.view(np.int32))
        return
    got, want = emitted_and_uncarried(K, Ly, form)
    real = got[..., :Ly.Co].astype(np.int64) + 128
    assert (real == 0).any() and (real == 15).any() and ((real > 0) & (real < 15)).any()
    assert not got[..., Ly.Co:].any()
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------- accumulator extremes
@pytest.mark.parametrize("at", ["qmax", "qmin"])
def test_accumulator_extremes(K, at):
    """Ci = 512, 3x3 on a 3x3 plane (K = 4608): every m = +-16319 ((q - z) = +-1, k = 16319), every
    activation at qmax with z_a = qmin, or at qmin with z_a = qmax: |I| = 4608 * 255 * 16319
    passes 2^31 in the centre and the conversion rounds; one channel all +, one all -, one all +
    but a single tap, the rest mixed."""
    N, Ci, Co = 1, 512, 8
    rng = np.random.default_rng(5)
    sign = rng.integers(0, 2, (Co, Ci, 3, 3)) * 2 - 1
    sign[0], sign[1], sign[2] = 1, -1, 1
    sign[2, 0, 1, 1] = -1
    zw = np.ones(Co, np.int64)
    qw = 1 + sign                                               # W2 codes 0 / 2 around z = 1
    k = np.full(Ci * 9, 16319)
    m = centred_operand(qw, zw, k)
    assert set(np.unique(m)) == {-16319, 16319}
    qa, za = (np.full((N, Ci, 3, 3), 255), 0) if at == "qmax" else (np.zeros((N, Ci, 3, 3), np.int64), 255)
    d1 = np.linspace(0.5, 1.5, Co).astype(F32)
    _, packed = encode_colscale(K, qw, zw, d1, k, 1024, 2)
    prep = K.qweight_prepare(packed, qw.shape, dev(zw), 2, 0, kcol=torch.from_numpy(k), wide=True)
    assert prep.wide and int(prep.bad.item()) == 0
    scale = grid_scale(F32(1.0), d1, 1024)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = K.qconv(dev((qa - za).astype(F32)), prep, dev(scale), 1, 1, act_zp=float(za), act_bits=8,
                act_delta=1.0, bad=bad)
    I = operand_sum(qa, za, m, 1, 1)
    assert np.abs(I).max() == 4608 * 255 * 16319 > 2 ** 31 and I.min() == -I.max()
    assert np.any(I.astype(F32).astype(np.int64) != I)
    np.testing.assert_array_equal(I, wide_sum(qa, za, m, 1, 1, 0))
    assert int(bad.item()) == 0
    np.testing.assert_array_equal(host(y).view(np.int32), ref_output(I, scale).view(np.int32))


# ---------------------------------------------------------------- one weight, two operands
@pytest.mark.parametrize("form", FORMS)
def test_wide_knob_is_bit_identical_to_the_centred_int8_form(K, monkeypatch, form):
    """A W2 / L32 per-(co, ci) weight (|m| <= 99) under SSQ_QCONV_WIDE=1 takes the wide blob and
    gives the centred int8 instantiation's bytes in all four forms; under auto it stays int8."""
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES["3x3_s1"]
    rng = np.random.default_rng(41)
    qw, zw, wscale = draw_perci_weight(rng, (Co, Cc, R, R), 2)
    L, base, k = K.perci_grid(torch.from_numpy(wscale), Co, Cc, 127)
    m = perci_operand(qw, zw, k.numpy())
    assert np.abs(m).max() <= 127
    _, packed = encode_perci(K, qw, zw, wscale, 2)
    preps = {}
    for knob in ("auto", "1"):
        monkeypatch.setattr(K, "QCONV_WIDE", knob)
        preps[knob] = K.qweight_prepare_scaled(packed, qw.shape, dev(zw), 2, 0, kfac=k, wide=True)
        assert int(preps[knob].bad.item()) == 0 and preps[knob].centred
    assert not preps["auto"].wide and preps["1"].wide
    assert K._qconv_fn(preps["auto"], 1, "fwd") == "ssq_qconv_i8_centred_fwd"
    assert preps["1"].blob.numel() > preps["auto"].blob.numel()
    qa, za = rng.integers(0, 16, (N, Cc, H, W)), 6
    da = F32(0.125)
    codes, _ = K.act_encode(dev((qa - za).astype(F32) * da), float(da), float(za), 4, False)
    scale = grid_scale(da, base.numpy(), L)
    ref = ref_output(operand_sum(qa, za, m, stride, pad), scale)
    Ly = types.SimpleNamespace(codes=codes, scale=scale, ref=ref, geo=(stride, pad), Co=Co,
                               kw=dict(act_zp=float(za), act_bits=4, act_sym=False))
    if form == "fp32":
        ys = [host(K.qconv(codes, preps[kn], dev(scale), stride, pad, **Ly.kw)) for kn in ("auto", "1")]
        np.testing.assert_array_equal(ys[0].view(np.int32), ref.view(np.int32))
        np.testing.assert_array_equal(ys[1].view(np.int32), ys[0].view(np.int32))
        return
    narrow, _ = emitted_and_uncarried(K, Ly, form, preps["auto"])
    wide, _ = emitted_and_uncarried(K, Ly, form, preps["1"])
    assert narrow.any()
    np.testing.assert_array_equal(wide, narrow)


def test_wide_prepare_counts_what_leaves_two_digits(K):
    """k = 16319 against W4 codes: every |q - z| >= 2 leaves the wide range and is counted; a
    factor above 16319 is refused by the wrapper."""
    from shiftedscalequantization_amd._capi import SSQError
    rng = np.random.default_rng(9)
    ws = (8, 16, 1, 1)
    qw, zw = rng.integers(0, 16, ws), rng.integers(0, 16, 8)
    k = np.full(16, 16319)
    over = int((np.abs(centred_operand(qw, zw, k)) > 16319).sum())
    assert over > 0
    _, packed = encode_colscale(K, qw, zw, np.full(8, 0.01, F32), k, 1024, 4)
    prep = K.qweight_prepare(packed, ws, dev(zw), 4, 0, kcol=torch.from_numpy(k), wide=True)
    assert int(prep.bad.item()) == over
    with pytest.raises(SSQError, match="16319"):
        K.qweight_prepare(packed, ws, dev(zw), 4, 0, kcol=torch.from_numpy(k + 1), wide=True)
    with pytest.raises(SSQError, match="kcol or kfac"):
        K.qweight_prepare(packed, ws, dev(zw), 4, 0, wide=True)


# ---------------------------------------------------------------- refusals
def test_wrapper_refuses_a_wide_blob_where_no_kernel_reads_it(K):
    from shiftedscalequantization_amd._capi import SSQError
    Ly = layer("3x3_s1", "perci_w4_l32")
    stride, pad = Ly.geo
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(SSQError, match="no split-K form"):
        K.qconv(Ly.codes, Ly.prep, dev(Ly.scale), stride, pad, splits=2, **Ly.kw)
    with pytest.raises(SSQError, match="no split-K form"):
        K.qconv_codes(Ly.codes, Ly.prep, dev(Ly.scale), stride, pad, out_delta=0.1, bad=bad,
                      splits=2, **Ly.kw)
    packed = torch.zeros(256, dtype=torch.uint8, device="cuda")
    with pytest.raises(SSQError, match="K26"):
        K.qweight_prepare(packed, (6, 4, 3, 3), torch.zeros(6, device="cuda"), 4, 0, groups=3,
                          kfac=torch.ones(24, dtype=torch.int32), wide=True)
    fc = K.qweight_prepare(packed, (10, 32), torch.zeros(10, device="cuda"), 4, 0,
                           kfac=torch.full((320,), 200, dtype=torch.int32), wide=True)
    assert fc.wide
    hi = torch.zeros(2, 32, dtype=torch.int8, device="cuda")
    sp = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(SSQError, match="K30"):
        K.qlinear_pooled(hi, hi.clone(), sp, fc, torch.ones(10, device="cuda"), 4)
    # a grouped weight whose grid leaves int8 has no blob at all
    assert K.qweight_prepare_scaled(packed, (6, 4, 3, 3), torch.zeros(6, device="cuda"), 4, 0, groups=3,
                                    kfac=torch.full((24,), 200, dtype=torch.int32), wide=True) is None
