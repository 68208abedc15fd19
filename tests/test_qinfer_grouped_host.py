"""Grouped / depthwise integer inference (K24-K26, csrc/qinfer_grouped.hip), host side: the
numpy grouped integer reference the GPU tests compare against equals a float64 grouped
convolution exactly, the new ABI is declared, exported and bound, argument errors come back
without a GPU, and the size query and the kernel-choice rule are sane.  The reference lives
here (test_qinfer_grouped_gpu.py imports it)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_qinfer_host import centred_sum, qrange

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssq_qconv_grouped_kind", "ssq_qweight_prepared_bytes_grouped",
       "ssq_qweight_prepare_grouped", "ssq_qconv_i8_grouped_fwd")


# ---------------------------------------------------------------- numpy grouped reference
def grouped_centred_sum(qa, za, qw, zw, stride, pad, groups):
    """I of a grouped conv: test_qinfer_host.centred_sum per group, channels concatenated.
    qa (N, C, H, W), qw (Co, C / groups, R, S), zw (Co,)."""
    qa, qw, zw = np.asarray(qa), np.asarray(qw), np.asarray(zw)
    Cig, Cog = qa.shape[1] // groups, qw.shape[0] // groups
    assert qw.shape[1] == Cig and Cig * groups == qa.shape[1] and Cog * groups == qw.shape[0]
    return np.concatenate(
        [centred_sum(qa[:, g * Cig:(g + 1) * Cig], za, qw[g * Cog:(g + 1) * Cog],
                     zw[g * Cog:(g + 1) * Cog], stride, pad) for g in range(groups)], axis=1)


def grouped_ref_output(qa, za, qw, zw, scale, stride, pad, groups):
    """The kernels' contract: fp32(I) * s[co] -- one conversion, one fp32 product."""
    I = grouped_centred_sum(qa, za, qw, zw, stride, pad, groups)
    return I.astype(np.float32) * np.asarray(scale, np.float32).reshape(1, -1, 1, 1)


@pytest.mark.parametrize("geo", [(2, 8, 8, 3, 1, 1), (3, 24, 24, 3, 2, 1), (4, 40, 20, 3, 1, 1),
                                 (6, 1, 2, 3, 2, 1), (5, 1, 1, 5, 1, 2), (3, 24, 24, 1, 1, 0)])
def test_grouped_reference_equals_float64_conv(geo):
    G, Cig, Cog, R, stride, pad = geo
    rng = np.random.default_rng(G * 1000 + Cig * 10 + R)
    qa = rng.integers(0, 256, (2, G * Cig, 6, 7))
    qw = rng.integers(0, 256, (G * Cog, Cig, R, R))
    zw = rng.integers(0, 256, G * Cog)
    za = int(rng.integers(0, 256))
    I = grouped_centred_sum(qa, za, qw, zw, stride, pad, G)
    # |I| < 2^53: the float64 convolution of the centred integers is exact
    x = torch.from_numpy((qa - za).astype(np.float64))
    w = torch.from_numpy((qw - zw.reshape(-1, 1, 1, 1)).astype(np.float64))
    want = F.conv2d(x, w, stride=stride, padding=pad, groups=G).numpy()
    assert I.shape == want.shape and I.dtype == np.int64
    np.testing.assert_array_equal(I.astype(np.float64), want)


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
    assert "qinfer_grouped.hip" in SOURCES
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert s in doc, s


def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


def _qconv(lib, codes, prep, scale, y, Nb=1, Cc=16, H=4, W=4, Co=16, R=3, S=3, stride=1, pad=1,
           groups=2, zp=0.0, qmin=0, qmax=255):
    return lib.ssq_qconv_i8_grouped_fwd(codes, prep, scale, Nb, Cc, H, W, Co, R, S, stride, pad,
                                        groups, zp, qmin, qmax, y, None)


def _prep(lib, packed, zp, prepared, bad, Co=16, Cig=8, R=3, S=3, groups=2, n_bits=4, qmin=0):
    return lib.ssq_qweight_prepare_grouped(packed, zp, Co, Cig, R, S, groups, n_bits, qmin,
                                           prepared, bad, None)


def test_argument_errors_without_gpu():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    f = _fake
    err = lib.ssq_last_error
    assert _qconv(lib, None, f(), f(), f()) == -1 and b"null" in err()
    assert _qconv(lib, f(), f(), f(), None) == -1 and b"null" in err()
    assert _qconv(lib, f(), f(), f(), f(), groups=1) == -1
    assert b"groups" in err() and b"ssq_qconv_i8_fwd" in err()
    assert _qconv(lib, f(), f(), f(), f(), Cc=10, groups=4) == -1
    assert b"C = 10" in err() and b"groups" in err()
    assert _qconv(lib, f(), f(), f(), f(), Co=18, groups=4) == -1
    assert b"Co = 18" in err() and b"groups" in err()
    assert _qconv(lib, f(), f(), f(), f(), Cc=2 * 8192, Co=2, H=8, W=8) == -1 and b"65536" in err()
    assert _qconv(lib, f(), f(), f(), f(), Cc=2 * 65537, Co=2, R=1, S=1, pad=0) == -1
    assert b"65536" in err()
    assert _qconv(lib, f(), f(), f(), f(), R=9, S=9, H=16, W=16) == -1 and b"R = 9" in err()
    assert _qconv(lib, f(), f(), f(), f(), zp=0.5) == -1 and b"zero point" in err()
    assert _qconv(lib, f(), f(), f(), f(), zp=256.0) == -1 and b"zero point" in err()
    assert _qconv(lib, f(), f(), f(), f(), Nb=1 << 20, Cc=64, Co=64, H=8, W=8) == -1
    assert b"2^31" in err()
    # the depthwise route takes the same checks
    assert _qconv(lib, f(), f(), f(), f(), Cc=16, Co=16, groups=16, zp=0.5) == -1
    assert b"zero point" in err()
    assert _qconv(lib, f(), f(), f(), f(), Cc=16, Co=16, groups=16, R=8, S=8, H=16, W=16) == -1
    # K24
    assert _prep(lib, None, f(), f(), f()) == -1 and b"null" in err()
    assert _prep(lib, f(), f(), f(), None) == -1 and b"null" in err()
    assert _prep(lib, f(), f(), f(), f(), groups=1) == -1
    assert b"groups" in err() and b"ssq_qweight_prepare" in err()
    assert _prep(lib, f(), f(), f(), f(), Co=17) == -1 and b"Co = 17" in err()
    assert _prep(lib, f(), f(), f(), f(), Cig=8192) == -1 and b"65536" in err()
    assert _prep(lib, f(), f(), f(), f(), R=9) == -1 and b"R = 9" in err()
    assert _prep(lib, f(), f(), f(), f(), n_bits=9) == -1


def test_wrappers_check_groups_without_gpu():
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    with pytest.raises(SSQError):
        K.qweight_prepare(torch.zeros(64, dtype=torch.uint8), (4, 2, 3, 3), torch.zeros(4), 4, 0,
                          groups=2)                        # a CPU tensor
    assert K.QPrepared(None, (4, 2, 3, 3), None).groups == 1
    assert K.qconv_kind(K.QPrepared(None, (4, 2, 3, 3), None)) == "dense"
    assert K.qconv_kind(K.QPrepared(None, (8, 1, 3, 3), None, groups=8)) == "depthwise"
    assert K.qconv_kind(K.QPrepared(None, (8, 2, 3, 3), None, groups=2)) == "grouped"
    with pytest.raises(SSQError):
        K.qconv_kind(K.QPrepared(None, (9, 2, 3, 3), None, groups=2))


def test_prepared_bytes_grouped_positive_and_monotone():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    q = lib.ssq_qweight_prepared_bytes_grouped
    assert q(16, 8, 3, 3, 2) > 0 and q(5, 1, 3, 3, 5) > 0
    # invalid geometry
    assert q(16, 8, 3, 3, 1) == 0 and q(16, 8, 3, 3, 0) == 0 and q(17, 8, 3, 3, 2) == 0
    assert q(0, 8, 3, 3, 2) == 0 and q(16, 0, 3, 3, 2) == 0 and q(16, 8, 0, 3, 2) == 0
    assert q(16, 8, 9, 9, 2) == 0
    # grouped: monotone in Co at a fixed (groups, Cig, R)
    for G, Cig, R in ((2, 8, 3), (3, 24, 3), (4, 40, 3), (9, 48, 3), (2, 56, 3), (6, 1, 3),
                      (2, 24, 1), (2, 3, 7)):
        sizes = [q(G * Cog, Cig, R, R, G) for Cog in range(1, 140)]
        assert all(b >= a > 0 for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        for Cog, b in zip(range(1, 140), sizes):
            assert b >= G * Cog * Cig * R * R       # at least the int8 weights
    # depthwise: Co = C = groups move together
    for R in (1, 3, 5, 7):
        sizes = [q(Cc, 1, R, R, Cc) for Cc in range(2, 200)]
        assert all(b >= a > 0 for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        for Cc, b in zip(range(2, 200), sizes):
            assert b >= Cc * R * R


def test_grouped_kind():
    from shiftedscalequantization_amd import _capi
    kind = _capi.load().ssq_qconv_grouped_kind
    for Cc in (2, 5, 16, 960):
        assert kind(Cc, 1, Cc) == 1
    assert kind(16, 8, 2) == 2 and kind(12, 1, 6) == 2      # channel multiplier 2: not depthwise
    assert kind(432, 48, 9) == 2 and kind(2, 8, 2) == 2
    assert kind(16, 8, 1) == 0 and kind(16, 8, 0) == 0 and kind(17, 8, 2) == 0
    assert kind(0, 8, 2) == 0 and kind(16, 0, 2) == 0 and kind(16, 8, -2) == 0


def test_cli_int_infer_grouped_implies_int_infer():
    from shiftedscalequantization_amd.cli import parse_args
    a = parse_args(["--int_infer_grouped"])
    assert a.int_infer_grouped and a.int_infer
    a = parse_args(["--int_infer"])
    assert a.int_infer and not a.int_infer_grouped
    a = parse_args([])
    assert not a.int_infer and not a.int_infer_grouped
