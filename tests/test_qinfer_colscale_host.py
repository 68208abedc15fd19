"""Integer inference of column-scaled weights, host side: the grid rule of
kernels.colscale_grid (the smallest L <= 127 with k[j] = rint(c[j] * L) >= 1 and fp32(k[j] / L)
== c[j] bit for bit), the new ABI (declared, exported, bound, argument errors without a GPU),
the --int_infer_colscale flag, and the numpy integer reference the GPU tests compare against
(test_qinfer_colscale_gpu.py imports it)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from test_qinfer_host import conv_i64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssq_qweight_prepare_colscale", "ssq_qweight_prepare_grouped_colscale",
       "ssq_qconv_i8_centred_fwd", "ssq_qconv_i8_centred_codes_fwd",
       "ssq_qconv_i8_centred_codes_res_fwd")
F32 = np.float32


# ---------------------------------------------------------------- numpy integer reference
def centred_operand(qw, zw, k):
    """m[co, j] = (q_w - z_w[co]) * k[j], j = (ci, r, s); qw (Co, Cig, R, S), k (Cig*R*S,)."""
    qw = np.asarray(qw, np.int64)
    w = qw - np.asarray(zw, np.int64).reshape(-1, 1, 1, 1)
    return w * np.asarray(k, np.int64).reshape((1,) + qw.shape[1:])


def colscale_sum(qa, za, qw, zw, k, stride, pad, groups=1):
    """I = sum_j (q_a - z_a) m[co, j] over co's group; a zero-padded tap contributes 0."""
    a = np.asarray(qa, np.int64) - int(za)
    m = centred_operand(qw, zw, k)
    Co, Cig = m.shape[:2]
    Cog = Co // groups
    outs = [conv_i64(a[:, g * Cig:(g + 1) * Cig], m[g * Cog:(g + 1) * Cog], stride, pad)
            for g in range(groups)]
    return np.concatenate(outs, axis=1)


def colscale_scale(da, d1, L):
    """s[co] = fp32(fp32(delta_a * d1[co]) / fp32(L))."""
    s = F32(da) * np.asarray(d1, F32)
    assert s.dtype == F32
    return s / F32(L)


def ref_output(qa, za, qw, zw, k, scale, stride, pad, groups=1):
    """The contract: fp32(I) * s[co] -- one conversion, one fp32 product."""
    I = colscale_sum(qa, za, qw, zw, k, stride, pad, groups)
    return I.astype(F32) * np.asarray(scale, F32).reshape(1, -1, 1, 1)


def test_reference_centred_identity():
    """The kernel's route restated: D = sum a_s m with the pad constant on padded taps, then
    I = D + az * T[co]."""
    rng = np.random.default_rng(3)
    qa, za, alo = rng.integers(0, 16, (2, 5, 6, 4)), 6, 0
    qw, zw, k = rng.integers(0, 4, (7, 5, 3, 3)), rng.integers(0, 4, 7), rng.integers(1, 33, 45)
    m = centred_operand(qw, zw, k)
    ca = alo + 128
    D = conv_i64(qa - ca, m, 1, 1, fill=za - ca)
    T = m.reshape(7, -1).sum(1)
    np.testing.assert_array_equal(D + (ca - za) * T.reshape(1, -1, 1, 1),
                                  colscale_sum(qa, za, qw, zw, k, 1, 1))


# ---------------------------------------------------------------- the grid rule
@pytest.mark.parametrize("level", [1, 2, 3, 4, 8, 32, 127])
def test_grid_of_a_searched_scale(level):
    from shiftedscalequantization_amd import kernels as K
    rng = np.random.default_rng(level)
    k = rng.integers(1, level + 1, 300)
    k[0], k[-1] = 1, level
    c = torch.from_numpy(k.astype(F32) / F32(level))
    L, kk = K.colscale_grid(c)
    assert kk.dtype == torch.int32 and tuple(kk.shape) == (300,)
    kk = kk.numpy().astype(np.int64)
    # L divides level, k is the same fraction, and it reproduces c bit for bit
    assert 1 <= L <= level and level % L == 0
    np.testing.assert_array_equal(kk * (level // L), k)
    np.testing.assert_array_equal((kk.astype(F32) / F32(L)).view(np.int32), c.numpy().view(np.int32))
    # the smallest such L: k[0] = 1 of `level` has no smaller denominator
    assert L == level
    # any shape is flattened
    assert K.colscale_grid(c.reshape(1, 3, 10, 10))[0] == L


def test_grid_is_the_smallest_denominator():
    from shiftedscalequantization_amd import kernels as K
    L, k = K.colscale_grid(torch.tensor([1.0, 0.5, 0.5, 1.0]))      # level 4 found {2, 4} / 4
    assert L == 2 and k.tolist() == [2, 1, 1, 2]
    L, k = K.colscale_grid(torch.ones(1, 5, 3, 3))
    assert L == 1 and k.tolist() == [1] * 45
    L, k = K.colscale_grid(torch.tensor([0.75, 0.25]))
    assert L == 4 and k.tolist() == [3, 1]


def test_grid_refusals():
    from shiftedscalequantization_amd import kernels as K
    g = torch.Generator().manual_seed(1)
    assert K.colscale_grid(torch.rand(64, generator=g) + 0.5) is None
    assert K.colscale_grid(torch.tensor([1.0, 1.0 / 128.0])) is None        # needs L = 128
    assert K.colscale_grid(torch.tensor([1.0, 127.0 / 128.0])) is None
    assert K.colscale_grid(torch.tensor([1.0, 0.0])) is None
    assert K.colscale_grid(torch.tensor([1.0, -0.5])) is None
    assert K.colscale_grid(torch.tensor([1.0, float("nan")])) is None
    assert K.colscale_grid(torch.tensor([1.0, float("inf")])) is None
    # one ulp off a grid point is off the grid
    c = np.array([1.0, 0.75], F32)
    c[1] = np.nextafter(c[1], F32(1))
    assert K.colscale_grid(torch.from_numpy(c)) is None
    assert K.colscale_grid(torch.tensor([1.0, 1.0 / 127.0]))[0] == 127


# ---------------------------------------------------------------- ABI
def test_new_symbols_declared_exported_and_bound():
    from shiftedscalequantization_amd import _capi
    src = open(os.path.join(ROOT, "include", "ssq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _capi.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, src), s
        assert hasattr(lib, s), s
        assert s in _capi.SIGNATURES, s
    # the centred convs take their plain twins' arguments
    for form in ("fwd", "codes_fwd", "codes_res_fwd"):
        assert _capi.SIGNATURES[f"ssq_qconv_i8_centred_{form}"] == _capi.SIGNATURES[f"ssq_qconv_i8_{form}"]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(s in doc for s in NEW)


def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


def test_argument_errors_without_gpu():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    f = _fake
    prep = lib.ssq_qweight_prepare_colscale
    assert prep(f(), f(), None, 8, 8, 1, 1, 4, 0, f(), f(), None) == -1
    assert b"null" in lib.ssq_last_error()
    assert prep(f(), f(), f(), 8, 65537, 1, 1, 4, 0, f(), f(), None) == -1
    assert b"65536" in lib.ssq_last_error()
    assert prep(f(), f(), f(), 8, 8, 1, 1, 9, 0, f(), f(), None) == -1
    gprep = lib.ssq_qweight_prepare_grouped_colscale
    assert gprep(f(), f(), None, 8, 1, 3, 3, 8, 4, 0, f(), f(), None) == -1
    assert b"null" in lib.ssq_last_error()
    assert gprep(f(), f(), f(), 8, 8, 3, 3, 1, 4, 0, f(), f(), None) == -1
    assert b"groups" in lib.ssq_last_error()
    assert gprep(f(), f(), f(), 9, 4, 3, 3, 2, 4, 0, f(), f(), None) == -1
    conv = lib.ssq_qconv_i8_centred_fwd
    args = lambda **kw: [kw.get(n, v) for n, v in (("Nb", 1), ("Ci", 8), ("H", 4), ("W", 4), ("Co", 8),
                                                   ("R", 1), ("S", 1), ("stride", 1), ("pad", 0),
                                                   ("groups", 1), ("zp", 0.0), ("qmin", 0),
                                                   ("qmax", 255))]
    assert conv(None, f(), f(), *args(), f(), None) == -1 and b"null" in lib.ssq_last_error()
    assert conv(f(), f(), f(), *args(groups=2), f(), None) == -1 and b"groups" in lib.ssq_last_error()
    assert conv(f(), f(), f(), *args(zp=0.5), f(), None) == -1 and b"zero point" in lib.ssq_last_error()
    assert conv(f(), f(), f(), *args(Ci=65537), f(), None) == -1 and b"65536" in lib.ssq_last_error()


def test_wrapper_checks_kcol():
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    with pytest.raises(SSQError):       # CPU tensors are refused before anything else
        K.qweight_prepare(torch.zeros(16, dtype=torch.uint8), (4, 4, 1, 1), torch.zeros(4), 4, 0,
                          kcol=torch.ones(4, dtype=torch.int32))
    assert K.QPrepared(None, (4, 4, 1, 1), None).centred is False
    assert K.QPrepared(None, (4, 4, 1, 1), None, centred=True).centred is True


def test_knob_routes_a_centred_blob(monkeypatch):
    from shiftedscalequantization_amd import kernels as K
    plain = K.QPrepared(None, (4, 4, 1, 1), None)
    centred = K.QPrepared(None, (4, 4, 1, 1), None, centred=True)
    grouped = K.QPrepared(None, (4, 1, 3, 3), None, groups=4, centred=True)
    for form in ("fwd", "codes_fwd", "codes_res_fwd"):
        monkeypatch.setattr(K, "QCONV_CENTRED", True)
        assert K._qconv_fn(plain, 1, form) == f"ssq_qconv_i8_{form}"
        assert K._qconv_fn(centred, 1, form) == f"ssq_qconv_i8_centred_{form}"
        monkeypatch.setattr(K, "QCONV_CENTRED", False)
        assert K._qconv_fn(centred, 1, form) == f"ssq_qconv_i8_{form}"
    assert K._qconv_fn(grouped, 4, "fwd") == "ssq_qconv_i8_grouped_fwd"


# ---------------------------------------------------------------- driver flag
def test_cli_flag_implications():
    from shiftedscalequantization_amd.cli import parse_args
    a = parse_args([])
    assert not a.int_infer_colscale and not a.int_infer
    a = parse_args(["--int_infer_colscale"])
    assert a.int_infer_colscale and a.int_infer
    assert not (a.int_infer_grouped or a.int_infer_carry or a.int_infer_carry_head)
    a = parse_args(["--int_infer_colscale", "--int_infer_carry_stem", "--int_infer_grouped",
                    "--test", "True"])
    assert a.int_infer_colscale and a.int_infer_carry_blocks and a.int_infer_carry
    assert a.int_infer_grouped and a.int_infer and a.test
    a = parse_args(["--int_infer_carry_head"])
    assert a.int_infer and not a.int_infer_colscale


def test_planner_signature_and_default():
    import inspect
    from shiftedscalequantization_amd.quant import enable_integer_inference
    p = inspect.signature(enable_integer_inference).parameters
    assert p["colscale"].default is False
