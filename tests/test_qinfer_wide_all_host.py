"""The wide operand on the grouped kernels and the pooled fc, without a device: the two-plane
grouped layout's size against a Python restatement, the new entry points' declarations and
argument refusals (each -1 with ssq_last_error set, before any launch), the wrappers' routing of
the marked blobs, and the keyword / flag defaults."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssq_qweight_prepared_bytes_grouped_wide", "ssq_qweight_prepare_grouped_wide",
       "ssq_qconv_i8_grouped_wide_fwd", "ssq_qconv_i8_grouped_wide_codes_fwd",
       "ssq_qlinear_pooled_wide_fwd")


def rup(v, m):
    return -(-v // m) * m


def grouped_bytes(Co, Cig, R, S, G, planes):
    """GLayout restated: `planes` digit planes of [G * Cogp][Kp] int8 rows, the 0/1 rows [G][Kp],
    cwz[Co] and T[Co] (int32); Kp covers R * S taps of the widest 16-aligned channel window."""
    Cogp = rup(Co // G, 16)
    Wc = max(rup((g + 1) * Cig, 16) - g * Cig // 16 * 16 for g in range(min(G, 16)))
    Kp = rup(R * S * Wc, 64)
    return planes * G * Cogp * Kp + G * Kp + 8 * Co, G * Cogp * Kp


@pytest.mark.parametrize("G,Cig,Cog,R", [(3, 24, 8, 3), (2, 64, 8, 3), (24, 24, 24, 3), (3, 24, 8, 1)])
def test_two_plane_layout_sizes(G, Cig, Cog, R):
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    Co = G * Cog
    wide, plane = grouped_bytes(Co, Cig, R, R, G, 2)
    narrow, _ = grouped_bytes(Co, Cig, R, R, G, 1)
    assert lib.ssq_qweight_prepared_bytes_grouped(Co, Cig, R, R, G) == narrow
    assert lib.ssq_qweight_prepared_bytes_grouped_wide(Co, Cig, R, R, G) == wide == narrow + plane
    # the LDS tile of the wide instantiation: 64 pixel rows + 2 x 64 weight rows of 80 bytes
    assert (64 + 2 * 64) * 80 == 15360


def test_depthwise_layout_is_the_int32_blob_and_bad_geometry_is_zero():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    q = lib.ssq_qweight_prepared_bytes_grouped_wide
    assert q(20, 1, 3, 3, 20) == lib.ssq_qweight_prepared_bytes_grouped(20, 1, 3, 3, 20) == 9 * 32 * 4
    assert q(24, 8, 8, 3, 3) == 0 and q(24, 8, 3, 3, 1) == 0 and q(25, 8, 3, 3, 3) == 0


def test_new_symbols_declared_exported_and_bound():
    from shiftedscalequantization_amd import _capi
    src = open(os.path.join(ROOT, "include", "ssq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _capi.load()
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % s, src)
        assert m and hasattr(lib, s) and s in _capi.SIGNATURES, s
        assert len(_capi.SIGNATURES[s][1]) == m.group(1).count(",") + 1, s
    S = _capi.SIGNATURES
    assert S["ssq_qconv_i8_grouped_wide_fwd"] == S["ssq_qconv_i8_grouped_fwd"]
    assert S["ssq_qconv_i8_grouped_wide_codes_fwd"] == S["ssq_qconv_i8_grouped_codes_fwd"]
    assert S["ssq_qlinear_pooled_wide_fwd"] == S["ssq_qlinear_pooled_fwd"]
    assert set(re.findall(r"\b(ssq_\w+)\s*\(", src)) == set(S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(s in doc for s in NEW)


def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


def test_argument_errors_without_gpu():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    f = _fake
    err = lib.ssq_last_error

    def prep(packed=True, zp=True, kfac=True, per_ci=0, Co=24, Cig=8, R=3, S=3, groups=3, n_bits=4,
             prepared=True, bad=True):
        p = lambda on: f() if on else None
        return lib.ssq_qweight_prepare_grouped_wide(p(packed), p(zp), p(kfac), per_ci, Co, Cig, R, S,
                                                    groups, n_bits, 0, p(prepared), p(bad), None)
    for name in ("packed", "zp", "kfac", "prepared", "bad"):
        assert prep(**{name: False}) == -1 and b"null" in err(), name
    assert prep(groups=1, Co=24, Cig=24) == -1 and b"groups" in err()
    assert prep(per_ci=1, Co=20, Cig=1, groups=20) == -1 and b"depthwise" in err()
    assert prep(R=8) == -1 and b"[1, 7]" in err()
    assert prep(Cig=65537, R=1, S=1) == -1 and b"65536" in err()
    assert prep(Cig=8192, R=3, S=3) == -1 and b"65536" in err()      # K = 73728
    assert prep(Co=25) == -1 and b"divisible" in err()
    assert prep(n_bits=9) == -1

    def conv(fn, tail, codes=True, prepared=True, scale=True, Nb=1, Cc=24, H=4, W=4, Co=24, R=3, S=3,
             stride=1, pad=1, groups=3, zp=0.0):
        p = lambda on: f() if on else None
        return fn(p(codes), p(prepared), p(scale), Nb, Cc, H, W, Co, R, S, stride, pad, groups, zp, 0,
                  255, *tail)
    fwd, cod = lib.ssq_qconv_i8_grouped_wide_fwd, lib.ssq_qconv_i8_grouped_wide_codes_fwd
    epi = (None, None, None, 1, 0.1, 0.0, 0, 15)
    for fn, tail in ((fwd, (f(), None)), (cod, (*epi, f(), f(), None))):
        for name in ("codes", "prepared", "scale"):
            assert conv(fn, tail, **{name: False}) == -1 and b"null" in err(), name
        assert conv(fn, tail, groups=1) == -1 and b"groups" in err()
        assert conv(fn, tail, R=8) == -1 and b"[1, 7]" in err()
        assert conv(fn, tail, Cc=3 * 8192) == -1 and b"65536" in err()
        assert conv(fn, tail, zp=0.5) == -1 and b"zero point" in err()
        assert conv(fn, tail, Cc=25) == -1 and b"divisible" in err()
    assert conv(fwd, (None, None)) == -1 and b"null" in err()
    assert conv(cod, (*epi, None, f(), None)) == -1
    assert conv(cod, (*epi, f(), None, None)) == -1

    def fc(hi=True, lo=True, sp=True, prepared=True, sh=True, y=True, N=2, Ci=16, Co=10, HW=49, zp=0.0):
        p = lambda on: f() if on else None
        return lib.ssq_qlinear_pooled_wide_fwd(p(hi), p(lo), p(sp), p(prepared), p(sh), N, Ci, Co, HW,
                                               zp, 0, 255, p(y), None)
    for name in ("hi", "lo", "sp", "prepared", "sh", "y"):
        assert fc(**{name: False}) == -1 and b"null" in err(), name
    assert fc(HW=127) == -1 and b"126" in err()
    assert fc(HW=0) == -1
    assert fc(Ci=65537) == -1 and b"65536" in err()
    assert fc(zp=0.5) == -1 and b"zero point" in err()
    assert fc(N=0) == -1


def test_wrapper_routes_the_marked_blobs(monkeypatch):
    """A grouped wide blob carries a mark of its own (QPrepared.wide_all): with it the grouped wide
    entry points, without it today's refusal; no residual form, no split-K form."""
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    marked = K.QPrepared(None, (4, 2, 3, 3), None, groups=2, centred=True, wide=True, wide_all=True)
    bare = K.QPrepared(None, (4, 2, 3, 3), None, groups=2, centred=True, wide=True)
    assert marked.wide_all and not bare.wide_all
    assert not K.QPrepared(None, (4, 4, 1, 1), None, centred=True, wide=True).wide_all
    for centred in (True, False):
        monkeypatch.setattr(K, "QCONV_CENTRED", centred)
        assert K._qconv_fn(marked, 2, "fwd") == "ssq_qconv_i8_grouped_wide_fwd"
        assert K._qconv_fn(marked, 2, "codes_fwd") == "ssq_qconv_i8_grouped_wide_codes_fwd"
    with pytest.raises(SSQError, match="K26"):
        K._qconv_fn(bare, 2, "fwd")
    with pytest.raises(SSQError, match="residual"):
        K._qconv_fn(marked, 2, "codes_res_fwd")
    with pytest.raises(SSQError, match="groups == 1"):
        K._qconv_split("qconv", marked, 2, "fwd", 2, None, torch.zeros(1, 4, 4, 16, dtype=torch.int8), 1, 0)
    for fn in (K.qweight_prepare, K.qweight_prepare_scaled, K.qlinear_pooled):
        assert inspect.signature(fn).parameters["wide_all"].default is False


def test_keyword_defaults_to_off_and_the_flag_implies_wide():
    from shiftedscalequantization_amd.cli import parse_args
    from shiftedscalequantization_amd.quant import enable_integer_inference
    assert inspect.signature(enable_integer_inference).parameters["wide_all"].default is False
    a = parse_args([])
    assert not a.int_infer_wide_all and not a.int_infer_wide and not a.int_infer
    a = parse_args(["--int_infer_wide"])
    assert a.int_infer_wide and not a.int_infer_wide_all
    a = parse_args(["--int_infer_wide_all"])
    assert a.int_infer_wide_all and a.int_infer_wide and a.int_infer
    assert not a.int_infer_per_ci and not a.int_infer_grouped
