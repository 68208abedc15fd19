"""Carried int8 codes between integer layers (csrc/qinfer_epi.h), host side: the numpy float32
restatement of the code-emitting epilogue the GPU tests compare against (`ref_codes`) agrees
with the oracle's UniformAffineQuantizer, the new ABI is declared, exported and bound and
refuses bad output quantizers without a GPU, --int_infer_carry implies --int_infer, and every
block type declares its interior chain.  The reference lives here (test_qinfer_carry_gpu.py
imports it)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_qinfer_grouped_host import grouped_ref_output
from test_qinfer_host import qrange, ref_output

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssq_qconv_i8_codes_fwd", "ssq_qconv_i8_grouped_codes_fwd", "ssq_act_decode")
F32 = np.float32


# ---------------------------------------------------------------- numpy reference
def cpad(c):
    return (c + 15) // 16 * 16


def ref_pre_quant(y, bias, gamma, phi, act):
    """The K13 epilogue before the act quantizer on the conv's fp32 output y (N, Co, OH, OW):
    bias add, gamma * . + phi as two fp32 roundings, act 0 identity / 1 ReLU / 2 ReLU6 (NaN
    stays NaN, as torch.clamp)."""
    col = lambda v: np.asarray(v, F32).reshape(1, -1, 1, 1)
    t = np.asarray(y, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        if bias is not None:
            t = t + col(bias)
        if gamma is not None:
            t = (t * col(gamma)).astype(F32) + col(phi)
        if act >= 1:
            t = np.where(t < 0, F32(0), t)
        if act == 2:
            t = np.where(t > 6, F32(6), t)
    assert t.dtype == F32
    return t


def quant_codes(t, d_out, z_out, n_bits, sym):
    """round_ste(t / d) + z, clamped: (q as float32 with NaN kept, NaN count)."""
    lo, hi = qrange(n_bits, sym)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tq = (np.asarray(t, F32) / F32(d_out)).astype(F32)
        r = np.rint(tq)
        v = ((r - tq) + tq) + F32(z_out)          # round_ste: NaN at an infinite t / d
        q = np.clip(v, F32(lo), F32(hi))          # NaN stays NaN
    return q.astype(F32), int(np.isnan(q).sum())


def stored(q, n_bits, sym):
    """q (N, C, H, W; NaN -> qmin) -> K21's stored form: NHWC int8 q - (qmin + 128), channels
    zero-padded to a multiple of 16."""
    lo, _ = qrange(n_bits, sym)
    q = np.where(np.isnan(q), F32(lo), q)
    N, Cc, H, W = q.shape
    out = np.zeros((N, H, W, cpad(Cc)), np.int8)
    out[..., :Cc] = np.moveaxis(q.astype(np.int64) - (lo + 128), 1, -1).astype(np.int8)
    return out


def ref_codes(qa, za, qw, zw, scale, stride, pad, bias, gamma, phi, act, d_out, z_out, n_bits,
              sym, groups=1):
    """The code-emitting kernels' contract: (int8 NHWC codes, channel-padded; NaN count; the
    epilogue's pre-quantizer value t)."""
    if groups == 1:
        y = ref_output(qa, za, qw, zw, scale, stride, pad)
    else:
        y = grouped_ref_output(qa, za, qw, zw, scale, stride, pad, groups)
    t = ref_pre_quant(y, bias, gamma, phi, act)
    q, nbad = quant_codes(t, d_out, z_out, n_bits, sym)
    return stored(q, n_bits, sym), nbad, t


@pytest.mark.parametrize("n_bits,sym", [(2, False), (4, False), (4, True), (8, False), (8, True)])
def test_ref_codes_match_the_oracle_quantizer(n_bits, sym):
    """ref_codes's codes are the oracle UniformAffineQuantizer's codes of ref_codes's own
    pre-quantizer value, clamp edges, interior and ties included."""
    from oracle import ssq_ref as R
    rng = np.random.default_rng(40 + n_bits + sym)
    lo, hi = qrange(n_bits, sym)
    qa = rng.integers(0, 16, (2, 6, 5, 5))
    qw = rng.integers(0, 4, (7, 6, 3, 3))
    zw = rng.integers(0, 4, 7)
    scale = rng.uniform(0.01, 0.03, 7).astype(F32)
    bias = rng.normal(0, 0.5, 7).astype(F32)
    gamma, phi = rng.uniform(0.8, 1.2, 7).astype(F32), rng.normal(0, 0.1, 7).astype(F32)
    t = ref_pre_quant(ref_output(qa, 5, qw, zw, scale, 1, 1), bias, gamma, phi, 0)
    d_out = F32((np.percentile(t, 90) - np.percentile(t, 10)) / (hi - lo))
    z_out = float(np.clip(np.rint(lo - np.percentile(t, 10) / d_out), lo, hi))
    codes, nbad, t2 = ref_codes(qa, 5, qw, zw, scale, 1, 1, bias, gamma, phi, 0, d_out, z_out,
                                n_bits, sym)
    assert nbad == 0 and np.array_equal(t.view(np.int32), t2.view(np.int32))
    _, want = R.fake_quant(t, d_out, z_out, n_bits, sym)
    got = np.moveaxis(codes[..., :7].astype(np.int64) + (lo + 128), -1, 1)
    assert {lo, hi} <= set(np.unique(want)) and len(np.unique(want)) > 2   # both edges, interior
    np.testing.assert_array_equal(got, want)
    assert not codes[..., 7:].any()


def test_ref_codes_round_half_even_and_nan():
    t = np.array([0.5, 1.5, 2.5, -0.5, -1.5, np.nan, np.inf, -np.inf], F32).reshape(1, 8, 1, 1)
    q, nbad = quant_codes(t, 1.0, 0.0, 8, True)
    # inf / d is infinite: round_ste gives NaN there, as the quantizer does
    assert nbad == 3
    np.testing.assert_array_equal(q.reshape(-1)[:5], [0, 2, 2, -0.0, -2])
    s = stored(q, 8, True)
    assert s.shape == (1, 1, 1, 16) and s.dtype == np.int8
    np.testing.assert_array_equal(s.reshape(-1)[:8], [0, 2, 2, 0, -2, -128, -128, -128])


# ---------------------------------------------------------------- ABI
def test_new_symbols_declared_exported_and_bound():
    from shiftedscalequantization_amd import _capi
    src = open(os.path.join(ROOT, "include", "ssq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _capi.load()
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, src)
        assert m, s
        assert hasattr(lib, s), s
        assert s in _capi.SIGNATURES, s
        # one ctypes argument per declared parameter
        assert len(_capi.SIGNATURES[s][1]) == m.group(1).count(",") + 1, s
    from shiftedscalequantization_amd.build import HEADERS
    assert "qinfer_epi.h" in HEADERS
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert s in doc, s


def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


def _codes_fwd(lib, grouped=False, codes=True, bias=None, gamma=None, phi=None, act=1, d=0.1,
               z=0.0, qmin=0, qmax=15, out=True, bad=True, in_zp=0.0, groups=None):
    f = _fake
    fn = lib.ssq_qconv_i8_grouped_codes_fwd if grouped else lib.ssq_qconv_i8_codes_fwd
    groups = (2 if grouped else 1) if groups is None else groups
    return fn(f() if codes else None, f(), f(), 1, 16, 4, 4, 16, 3, 3, 1, 1, groups, in_zp, 0, 255,
              bias, gamma, phi, act, d, z, qmin, qmax, f() if out else None,
              f() if bad else None, None)


@pytest.mark.parametrize("grouped", [False, True])
def test_codes_entry_points_refuse_bad_arguments_without_gpu(grouped):
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    err = lib.ssq_last_error
    f = _fake
    assert _codes_fwd(lib, grouped, out=False) == -1 and b"null" in err()
    assert _codes_fwd(lib, grouped, bad=False) == -1 and b"null" in err()
    assert _codes_fwd(lib, grouped, codes=False) == -1 and b"null" in err()
    assert _codes_fwd(lib, grouped, gamma=f()) == -1 and b"gamma and phi" in err()
    assert _codes_fwd(lib, grouped, phi=f()) == -1 and b"gamma and phi" in err()
    assert _codes_fwd(lib, grouped, act=3) == -1 and b"activation" in err()
    assert _codes_fwd(lib, grouped, z=0.5) == -1 and b"output zero point" in err()
    assert _codes_fwd(lib, grouped, z=256.0) == -1 and b"output zero point" in err()
    assert _codes_fwd(lib, grouped, z=-1.0) == -1 and b"output zero point" in err()
    assert _codes_fwd(lib, grouped, z=float("nan")) == -1 and b"output zero point" in err()
    assert _codes_fwd(lib, grouped, qmin=0, qmax=256) == -1 and b"8-bit" in err()
    assert _codes_fwd(lib, grouped, qmin=3, qmax=3) == -1 and b"8-bit" in err()
    for d in (0.0, -1.0, float("inf"), float("nan")):
        assert _codes_fwd(lib, grouped, d=d) == -1 and b"delta" in err()
    # the input side keeps the fp32 entry point's checks
    assert _codes_fwd(lib, grouped, in_zp=0.5) == -1 and b"zero point" in err()
    assert _codes_fwd(lib, grouped, groups=1 if grouped else 2) == -1 and b"groups" in err()


def test_act_decode_refuses_bad_arguments_without_gpu():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    err = lib.ssq_last_error
    f = _fake
    dec = lib.ssq_act_decode
    assert dec(None, 1, 4, 2, 2, 0.1, 0.0, 0, f(), None) == -1 and b"null" in err()
    assert dec(f(), 1, 4, 2, 2, 0.1, 0.0, 0, None, None) == -1 and b"null" in err()
    assert dec(f(), 1, 0, 2, 2, 0.1, 0.0, 0, f(), None) == -1 and b"geometry" in err()
    assert dec(f(), 1, 4, 2, 2, 0.0, 0.0, 0, f(), None) == -1 and b"delta" in err()
    assert dec(f(), 1, 4, 2, 2, 0.1, 0.5, 0, f(), None) == -1 and b"zero point" in err()
    assert dec(f(), 1, 4, 2, 2, 0.1, 0.0, -129, f(), None) == -1 and b"qmin" in err()
    assert dec(f(), 1 << 20, 64, 8, 8, 0.1, 0.0, 0, f(), None) == -1 and b"2^31" in err()


def test_wrappers_refuse_without_gpu():
    import torch
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    prep = K.QPrepared(None, (4, 2, 3, 3), None)
    x = torch.zeros(1, 2, 4, 4)
    with pytest.raises(SSQError, match="out_delta and bad"):
        K.qconv_codes(x, prep, torch.ones(4))
    with pytest.raises(SSQError, match="gamma and phi"):
        K.qconv_codes(x, prep, torch.ones(4), gamma=torch.ones(4), out_delta=0.1,
                      bad=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(SSQError, match="conv layers only"):
        K.qconv_codes(x, K.QPrepared(None, (4, 2), None), torch.ones(4), out_delta=0.1,
                      bad=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(SSQError):
        K.act_decode(torch.zeros(1, 2, 2, 16), 4, 0.1, 0.0, 4)            # not int8
    with pytest.raises(SSQError):
        K.act_decode(torch.zeros(1, 2, 2, 16, dtype=torch.int8), 4, 0.1, 0.0, 4)   # a CPU tensor
    cc = K.CarriedCodes((1, 4, 2, 2), 0.1, 3.0, 4, False)
    assert cc.quantizer() == (0.1, 3.0, 4, False) and cc.shape == (1, 4, 2, 2)
    # a plain tensor passes through materialize_epi untouched
    assert K.materialize_epi(x) is x


# ---------------------------------------------------------------- CLI, block structure
def test_cli_int_infer_carry_implies_int_infer():
    from shiftedscalequantization_amd.cli import parse_args
    a = parse_args(["--int_infer_carry"])
    assert a.int_infer_carry and a.int_infer and not a.int_infer_grouped
    a = parse_args(["--int_infer_carry", "--int_infer_grouped"])
    assert a.int_infer_carry and a.int_infer and a.int_infer_grouped
    a = parse_args(["--int_infer"])
    assert a.int_infer and not a.int_infer_carry
    assert not parse_args([]).int_infer_carry


@pytest.mark.parametrize("arch,block,n_pairs", [
    ("resnet18", "QuantBasicBlock", {1}), ("resnet50", "QuantBottleneck", {2}),
    ("regnetx_600m", "QuantResBottleneckBlock", {2}), ("mobilenetv2", "QuantInvertedResidual", {1, 2})])
def test_interior_chain_of_every_block_type(arch, block, n_pairs):
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd.quant import QuantModule
    from shiftedscalequantization_amd.quant.quant_block import BaseQuantBlock
    qnn = D.build_qnn(arch, 2, 4, device="cpu")
    blocks = [m for m in qnn.modules() if isinstance(m, BaseQuantBlock)]
    assert blocks and {type(b).__name__ for b in blocks} == {block}
    assert {len(b.interior_chain()) for b in blocks} == n_pairs
    for b in blocks:
        chain = b.interior_chain()
        convs = list(b.conv) if block == "QuantInvertedResidual" else [b.conv1, b.conv2] + (
            [] if block == "QuantBasicBlock" else [b.conv3])
        assert chain == list(zip(convs[:-1], convs[1:]))
        for prod, cons in chain:
            assert isinstance(prod, QuantModule) and isinstance(cons, QuantModule)
            # a producer owns an act quantizer; the block's last conv (the tail) never produces
            assert not prod.disable_act_quant and prod is not convs[-1]
            assert getattr(b, "downsample", None) not in (prod, cons)
    assert BaseQuantBlock.interior_chain(blocks[0]) == []
