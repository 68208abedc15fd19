"""Integer inference (K21-K23, csrc/qinfer.hip), host side: the ABI is declared, exported and
bound, argument errors come back without a GPU, the prepared-weight size query is sane, and
the numpy integer reference the GPU tests compare against satisfies the kernel's
shift-and-correct identity.  The reference lives here (test_qinfer_gpu.py imports it)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssq_qinfer_cpad", "ssq_qweight_prepared_bytes", "ssq_act_encode", "ssq_qweight_prepare",
       "ssq_qconv_i8_fwd")


# ---------------------------------------------------------------- numpy integer reference
def qrange(n_bits, sym):
    n = 2 ** n_bits
    return (-(n // 2), n // 2 - 1) if sym else (0, n - 1)


def conv_i64(a, w, stride, pad, fill=0):
    """int64 cross-correlation of a (N, C, H, W) with w (Co, C, R, S); the border is `fill`."""
    a, w = np.asarray(a, np.int64), np.asarray(w, np.int64)
    N, Cc, H, W = a.shape
    Co, _, R, S = w.shape
    ap = np.full((N, Cc, H + 2 * pad, W + 2 * pad), fill, np.int64)
    ap[:, :, pad:pad + H, pad:pad + W] = a
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    out = np.zeros((N, Co, OH, OW), np.int64)
    for r in range(R):
        for s in range(S):
            patch = ap[:, :, r:r + stride * (OH - 1) + 1:stride, s:s + stride * (OW - 1) + 1:stride]
            out += np.einsum("nchw,oc->nohw", patch, w[:, :, r, s])
    return out


def centred_sum(qa, za, qw, zw, stride, pad):
    """I = sum (q_a - z_a)(q_w - z_w[co]); a zero-padded tap contributes (q_a - z_a) = 0."""
    a = np.asarray(qa, np.int64) - int(za)
    w = np.asarray(qw, np.int64) - np.asarray(zw, np.int64).reshape(-1, 1, 1, 1)
    return conv_i64(a, w, stride, pad)


def ref_output(qa, za, qw, zw, scale, stride, pad):
    """The kernel's contract: fp32(I) * s[co] -- one conversion, one fp32 product."""
    I = centred_sum(qa, za, qw, zw, stride, pad)
    return I.astype(np.float32) * np.asarray(scale, np.float32).reshape(1, -1, 1, 1)


def shifted_sum(qa, za, a_qmin, qw, zw, w_qmin, stride, pad):
    """The kernel's route restated: int8 operands shifted by qmin + 128, padded taps holding
    z_a - ca, the cross terms restored from the window sum SA and the per-channel T."""
    ca, cw = a_qmin + 128, w_qmin + 128
    a_s = np.asarray(qa, np.int64) - ca
    w_s = np.asarray(qw, np.int64) - cw
    assert a_s.min() >= -128 and a_s.max() <= 127 and w_s.min() >= -128 and w_s.max() <= 127
    assert -128 <= int(za) - ca <= 127
    D = conv_i64(a_s, w_s, stride, pad, fill=int(za) - ca)
    SA = conv_i64(a_s, np.ones((1,) + w_s.shape[1:], np.int64), stride, pad, fill=int(za) - ca)
    cwz = cw - np.asarray(zw, np.int64)
    K = int(np.prod(w_s.shape[1:]))
    T = w_s.reshape(w_s.shape[0], -1).sum(1) + K * cwz
    return D + cwz.reshape(1, -1, 1, 1) * SA + (ca - int(za)) * T.reshape(1, -1, 1, 1)


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
    from shiftedscalequantization_amd.build import SOURCES
    assert "qinfer.hip" in SOURCES


def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


def _qconv(lib, codes, prep, scale, y, Nb=1, Ci=8, H=4, W=4, Co=8, R=1, S=1, stride=1, pad=0,
           groups=1, zp=0.0, qmin=0, qmax=255):
    return lib.ssq_qconv_i8_fwd(codes, prep, scale, Nb, Ci, H, W, Co, R, S, stride, pad, groups, zp,
                                qmin, qmax, y, None)


def test_argument_errors_without_gpu():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    f = _fake
    assert _qconv(lib, None, f(), f(), f()) == -1 and b"null" in lib.ssq_last_error()
    assert _qconv(lib, f(), f(), f(), None) == -1 and b"null" in lib.ssq_last_error()
    assert _qconv(lib, f(), f(), f(), f(), groups=2, Ci=8) == -1 and b"groups" in lib.ssq_last_error()
    assert _qconv(lib, f(), f(), f(), f(), Ci=65537) == -1 and b"65536" in lib.ssq_last_error()
    assert _qconv(lib, f(), f(), f(), f(), Ci=8192, R=3, S=3, H=8, W=8) == -1
    assert b"65536" in lib.ssq_last_error()
    assert _qconv(lib, f(), f(), f(), f(), zp=0.5) == -1 and b"zero point" in lib.ssq_last_error()
    assert _qconv(lib, f(), f(), f(), f(), zp=256.0, qmin=0, qmax=255) == -1
    assert b"zero point" in lib.ssq_last_error()
    assert _qconv(lib, f(), f(), f(), f(), zp=-9.0, qmin=-8, qmax=7) == -1
    assert b"zero point" in lib.ssq_last_error()
    assert _qconv(lib, f(), f(), f(), f(), zp=128.0, qmin=-128, qmax=127) == -1
    assert b"zero point" in lib.ssq_last_error()
    assert _qconv(lib, f(), f(), f(), f(), R=9, S=9, H=16, W=16) == -1
    # K21 / K22
    assert lib.ssq_act_encode(None, 1, 4, 2, 2, 0.1, 0.0, 0, 15, f(), f(), None) == -1
    assert b"null" in lib.ssq_last_error()
    assert lib.ssq_act_encode(f(), 1, 4, 2, 2, 0.1, 1.5, 0, 15, f(), f(), None) == -1
    assert b"zero point" in lib.ssq_last_error()
    assert lib.ssq_act_encode(f(), 1, 4, 2, 2, 0.1, 0.0, 0, 256, f(), f(), None) == -1
    assert lib.ssq_qweight_prepare(None, f(), 8, 8, 1, 1, 4, 0, f(), f(), None) == -1
    assert b"null" in lib.ssq_last_error()
    assert lib.ssq_qweight_prepare(f(), f(), 8, 65537, 1, 1, 4, 0, f(), f(), None) == -1
    assert b"65536" in lib.ssq_last_error()
    assert lib.ssq_qweight_prepare(f(), f(), 8, 8, 1, 1, 9, 0, f(), f(), None) == -1


def test_wrappers_refuse_cpu_tensors():
    import torch
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    with pytest.raises(SSQError):
        K.act_encode(torch.zeros(1, 4, 2, 2), 0.1, 0.0, 4)
    with pytest.raises(SSQError):
        K.qweight_prepare(torch.zeros(16, dtype=torch.uint8), (4, 4, 1, 1), torch.zeros(4), 4, 0)


def test_prepared_bytes_positive_and_monotone():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    q = lib.ssq_qweight_prepared_bytes
    assert q(1, 1, 1, 1) > 0 and q(0, 1, 1, 1) == 0
    for Ci, R in ((3, 3), (64, 1), (130, 1), (160, 3), (8, 7)):
        sizes = [q(Co, Ci, R, R) for Co in range(1, 200)]
        assert all(b >= a > 0 for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        assert sizes[0] >= Ci * R * R      # at least the int8 weights of one channel
    for Co in (1, 17, 64):
        sizes = [q(Co, Ci, 3, 3) for Ci in range(1, 300)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        sizes = [q(Co, 16, R, R) for R in range(1, 8)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert [lib.ssq_qinfer_cpad(c) for c in (1, 16, 17, 130)] == [16, 16, 32, 144]


@pytest.mark.parametrize("a_sym", [False, True])
@pytest.mark.parametrize("w_sym", [False, True])
@pytest.mark.parametrize("geo", [(2, 3, 5, 5, 5, 3, 1, 1), (1, 8, 9, 9, 4, 7, 2, 3),
                                 (2, 20, 4, 6, 7, 1, 2, 0)])
def test_reference_shift_and_correct_identity_8_8(geo, w_sym, a_sym):
    N, Ci, H, W, Co, R, stride, pad = geo
    rng = np.random.default_rng(hash((geo, w_sym, a_sym)) & 0xffff)
    alo, ahi = qrange(8, a_sym)
    wlo, whi = qrange(8, w_sym)
    for za in (alo, ahi, int(rng.integers(alo, ahi + 1))):
        qa = rng.integers(alo, ahi + 1, (N, Ci, H, W))
        qw = rng.integers(wlo, whi + 1, (Co, Ci, R, R))
        zw = rng.integers(wlo, whi + 1, Co)
        zw[0], zw[-1] = wlo, whi
        np.testing.assert_array_equal(shifted_sum(qa, za, alo, qw, zw, wlo, stride, pad),
                                      centred_sum(qa, za, qw, zw, stride, pad))


def test_reference_extremes():
    qa = np.full((1, 160, 4, 4), 255)
    qw = np.full((2, 160, 3, 3), 255)
    I = centred_sum(qa, 0, qw, np.zeros(2), 1, 1)
    assert I.max() == 1440 * 255 * 255 > 2 ** 24
    np.testing.assert_array_equal(shifted_sum(qa, 0, 0, qw, np.zeros(2), 0, 1, 1), I)
    y = ref_output(qa, 0, qw, np.zeros(2), np.ones(2, np.float32), 1, 1)
    assert y.dtype == np.float32 and y.max() == np.float32(1440 * 255 * 255)
