"""The integer convs (K23 dense, K25 depthwise, K26 grouped) and their code-emitting epilogues
on non-square planes with R x S kernels (the Q_* lists of tests/test_conv_rect_host.py): 1x3 /
3x1 / 7x1 / 5x7 / 2x3 kernels, padding wider than the kernel (output columns made only of padded
taps, which the kernels fill with the activation zero point -- drawn non-zero here) and stride 3.
Outputs equal the host integer reference bit for bit, codes byte for byte."""
import functools
import types
import zlib

import numpy as np
import pytest
import torch

from test_conv_rect_host import Q_DENSE, Q_KINDS, out_hw
from test_qinfer_carry_gpu import VARIED, pick_quantizer
from test_qinfer_carry_host import cpad, ref_codes, stored
from test_qinfer_gpu import dev, encode_weight, host, parity_log
from test_qinfer_grouped_gpu import encode_weight as encode_weight_grouped
from test_qinfer_grouped_host import grouped_ref_output
from test_qinfer_host import qrange, ref_output
from test_qinfer_tail_host import decode_res, ref_codes_res

pytestmark = pytest.mark.gpu
F32 = np.float32

# (weight bits, weight sym, act bits, act sym): 8/8 asymmetric and 2/2 symmetric on every case,
# 4/4 on the first case of each kernel
EVERY = [(8, False, 8, False), (2, True, 2, True)]
SOME = (4, False, 4, False)
CASES = [(kind, cfg, bits) for kind, cases in Q_KINDS.items() for i, cfg in enumerate(cases)
         for bits in EVERY + ([SOME] if i == 0 else [])]
# the code-emitting epilogues: per kernel one case with H < W and one with H > W, both R != S
CODES_CASES = [(kind, cfg) for kind, cases in Q_KINDS.items() for cfg in cases[:2]]
# (out bits, out sym, act, bias, affine), from the carry tests' list
EPILOGUES = [VARIED[0], VARIED[1], VARIED[7]]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def make_layer(K, rng, cfg, bits, unit_weight_delta=False):
    """Seeded integer codes of one rectangular layer with a non-zero activation zero point,
    its prepared weight and fp32 input x_hat = (q - z) * delta."""
    N, Cc, H, W, Co, R, S, stride, pad, G = cfg
    wb, wsym, ab, asym = bits
    alo, ahi = qrange(ab, asym)
    wlo, whi = qrange(wb, wsym)
    L = types.SimpleNamespace(cfg=cfg, ab=ab, asym=asym)
    L.qa = rng.integers(alo, ahi + 1, (N, Cc, H, W))
    L.za = int(rng.choice([v for v in range(alo, ahi + 1) if v != 0]))
    L.qw = rng.integers(wlo, whi + 1, (Co, Cc // G, R, S))
    L.zw = rng.integers(wlo, whi + 1, Co)
    L.da = F32(rng.uniform(0.01, 0.2))
    L.d1 = np.ones(Co, F32) if unit_weight_delta else rng.uniform(1e-3, 2e-2, Co).astype(F32)
    if G == 1:
        _, L.prep = encode_weight(K, L.qw, L.zw, L.d1, wb, wsym)
    else:
        _, L.prep = encode_weight_grouped(K, L.qw, L.zw, L.d1, wb, wsym, G)
    L.xhat = (L.qa - L.za).astype(F32) * L.da
    return L


def reference(L, scale):
    N, Cc, H, W, Co, R, S, stride, pad, G = L.cfg
    if G == 1:
        return ref_output(L.qa, L.za, L.qw, L.zw, scale, stride, pad)
    return grouped_ref_output(L.qa, L.za, L.qw, L.zw, scale, stride, pad, G)


@functools.lru_cache(maxsize=None)
def run_case(kind, cfg, bits):
    from shiftedscalequantization_amd import kernels as K
    N, Cc, H, W, Co, R, S, stride, pad, G = cfg
    rng = np.random.default_rng(zlib.crc32(repr((kind, cfg, bits)).encode()))
    L = make_layer(K, rng, cfg, bits)
    scale = L.da * L.d1                                 # fp32(delta_a * d1[co])
    assert scale.dtype == F32 and L.za != 0
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = K.qconv(dev(L.xhat), L.prep, dev(scale), stride, pad, groups=G, act_zp=float(L.za),
                act_bits=L.ab, act_sym=L.asym, act_delta=float(L.da), bad=bad)
    return host(y), reference(L, scale), int(bad.item()), K.qconv_kind(L.prep)


@pytest.mark.parametrize("kind,cfg,bits", CASES)
def test_qconv_rect_bit_exact(K, kind, cfg, bits):
    out, ref, bad, got_kind = run_case(kind, cfg, bits)
    N, Cc, H, W, Co, R, S, stride, pad, G = cfg
    assert got_kind == kind and bad == 0
    assert out.shape == ref.shape == (N, Co) + out_hw(H, W, R, S, stride, pad)
    differ = int((out.view(np.int32) != ref.view(np.int32)).sum())
    parity_log({"test": "qconv_rect", "kind": kind, "case": list(cfg), "bits": list(bits),
                "differing_outputs": differ, "worst_err_over_bound": 0.0 if differ == 0 else None})
    np.testing.assert_array_equal(out.view(np.int32), ref.view(np.int32))


def test_cases_cover_the_issue():
    for kind, cases in Q_KINDS.items():
        for cfg in cases:
            mine = {b for k, c, b in CASES if (k, c) == (kind, cfg)}
            assert set(EVERY) <= mine, (kind, cfg)
        assert any(b == SOME for k, _, b in CASES if k == kind)
        mine = [c for k, c in CODES_CASES if k == kind]
        assert any(c[2] < c[3] for c in mine) and any(c[2] > c[3] for c in mine)
        assert all(c[5] != c[6] for c in mine)
    # padding wider than the kernel: whole output columns (rows) made only of padded taps
    assert any(c[8] >= c[5] or c[8] >= c[6] for c in Q_DENSE)


# ---------------------------------------------------------------- code-emitting epilogues
def _epilogue_params(rng, Co, case):
    ob, osym, act, use_bias, use_affine = case
    bias = rng.normal(0, 1.0, Co).astype(F32) if use_bias else None
    gamma = rng.uniform(0.5, 1.5, Co).astype(F32) if use_affine else None
    phi = rng.normal(0, 0.5, Co).astype(F32) if use_affine else None
    return bias, gamma, phi


def _codes_layer(K, rng, cfg):
    """A 4/4-bit layer whose raw outputs span a few units, so ReLU6's upper edge is met."""
    L = make_layer(K, rng, cfg, (4, False, 4, False), unit_weight_delta=True)
    I = reference(L, np.ones(cfg[4], F32))
    L.scale = (F32(4.0 / max(float(I.std()), 1.0)) * rng.uniform(0.5, 1.5, cfg[4])).astype(F32)
    L.codes, bad = K.act_encode(dev(L.xhat), float(L.da), float(L.za), L.ab, L.asym)
    assert int(bad.item()) == 0
    return L


def _fused(K, L, bias, gamma, phi, act, d, z, ob, osym, residual=None):
    N, Cc, H, W, Co, R, S, stride, pad, G = L.cfg
    tb = lambda v: None if v is None else dev(v)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = K.qconv_codes(L.codes, L.prep, dev(L.scale), stride, pad, groups=G, act_zp=float(L.za),
                        act_bits=L.ab, act_sym=L.asym, bias=tb(bias), gamma=tb(gamma), phi=tb(phi),
                        relu=act, out_delta=float(d), out_zp=float(z), out_bits=ob, out_sym=osym,
                        bad=bad, residual=residual)
    return host(out), int(bad.item())


@pytest.mark.parametrize("case", EPILOGUES)
@pytest.mark.parametrize("kind,cfg", CODES_CASES)
def test_qconv_codes_rect_equal_host_reference(K, kind, cfg, case):
    """qconv_codes (dense, depthwise, grouped) on rectangular cases: the int8 codes of the
    numpy epilogue reference, byte for byte."""
    N, Cc, H, W, Co, R, S, stride, pad, G = cfg
    ob, osym, act = case[:3]
    rng = np.random.default_rng(zlib.crc32(repr((kind, cfg, case)).encode()))
    L = _codes_layer(K, rng, cfg)
    assert K.qconv_kind(L.prep) == kind
    bias, gamma, phi = _epilogue_params(rng, Co, case)
    args = (L.qa, L.za, L.qw, L.zw, L.scale, stride, pad, bias, gamma, phi, act)
    d, z = pick_quantizer(ref_codes(*args, 1.0, 0.0, 8, False, G)[2], ob, osym)
    ref, ref_bad, _ = ref_codes(*args, d, z, ob, osym, G)
    fused, bad = _fused(K, L, bias, gamma, phi, act, d, z, ob, osym)
    lo, hi = qrange(ob, osym)
    real = ref[..., :Co].astype(np.int64) + (lo + 128)
    assert (real == lo).any() and (real == hi).any() and ((real > lo) & (real < hi)).any()
    assert ref_bad == 0 and bad == 0
    OH, OW = out_hw(H, W, R, S, stride, pad)
    assert fused.dtype == np.int8 and fused.shape == ref.shape == (N, OH, OW, cpad(Co))
    differ = int((fused != ref).sum())
    parity_log({"test": "qconv_codes_rect", "kind": kind, "case": list(cfg), "epilogue": list(case),
                "differing_codes": differ, "worst_err_over_bound": 0.0 if differ == 0 else None})
    assert np.array_equal(fused, ref), "fused codes differ from the host reference"


@pytest.mark.parametrize("case", EPILOGUES[:2])
@pytest.mark.parametrize("res_kind", ["fp32", "codes"])
@pytest.mark.parametrize("cfg", Q_DENSE[:2])
def test_qconv_codes_residual_rect_equal_host_reference(K, cfg, res_kind, case):
    """The dense residual form (a block tail) on the rectangular cases, with the residual as an
    fp32 tensor and as carried codes of another quantizer."""
    N, Cc, H, W, Co, R, S, stride, pad, G = cfg
    ob, osym, act = case[:3]
    rng = np.random.default_rng(zlib.crc32(repr((cfg, case, res_kind)).encode()))
    L = _codes_layer(K, rng, cfg)
    bias, gamma, phi = _epilogue_params(rng, Co, case)
    conv = (L.qa, L.za, L.qw, L.zw, L.scale, stride, pad, bias, gamma, phi)
    dims = (N, Co) + out_hw(H, W, R, S, stride, pad)
    spread = float(ref_codes(*conv, 0, 1.0, 0.0, 8, False)[2].std()) * 2.0 + 0.5
    if res_kind == "fp32":
        res = rng.normal(0, 0.5 * spread, dims).astype(F32)
        residual = dev(res)
    else:
        rb, rsym, rz = 8, False, 131.0
        rlo, rhi = qrange(rb, rsym)
        rd = F32(spread / (rhi - rlo))
        rcodes = stored(rng.integers(rlo, rhi + 1, dims).astype(F32), rb, rsym)
        res = decode_res(rcodes, Co, rd, rz, rb, rsym)
        residual = K.carried(dev(rcodes, torch.int8), dims, float(rd), rz, rb, rsym)
    t = ref_codes_res(*conv, act, 1.0, 0.0, 8, False, res)[2]
    d, z = pick_quantizer(t, ob, osym)
    ref, ref_bad, _ = ref_codes_res(*conv, act, d, z, ob, osym, res)
    fused, bad = _fused(K, L, bias, gamma, phi, act, d, z, ob, osym, residual=residual)
    assert ref_bad == 0 and bad == 0 and fused.shape == ref.shape
    differ = int((fused != ref).sum())
    parity_log({"test": "qconv_codes_res_rect", "kind": "dense_" + res_kind, "case": list(cfg),
                "epilogue": list(case), "differing_codes": differ,
                "worst_err_over_bound": 0.0 if differ == 0 else None})
    assert np.array_equal(fused, ref), "fused codes differ from the host reference"
