"""The shared act-quantizer argument check (csrc/qinfer_check.h, qquant_ok) through each of the
seven places that apply it, without a GPU: a bad zero point, a bad code range and, where the
entry point has a delta, a bad delta each return -1 with the entry point's own name in
ssq_last_error().  The pointers are non-null and never dereferenced: the checks return before
any launch."""
import ctypes as C

import pytest


def _fake():
    return C.c_void_p(256)


def _q(d=0.1, z=0.0, qmin=0, qmax=255):
    return dict(d=d, z=z, qmin=qmin, qmax=qmax)


def act_encode(lib, d, z, qmin, qmax):
    f = _fake
    return lib.ssq_act_encode(f(), 1, 4, 2, 2, d, z, qmin, qmax, f(), f(), None)


def act_decode(lib, d, z, qmin, qmax):      # no qmax: its range check bounds qmin
    f = _fake
    return lib.ssq_act_decode(f(), 1, 4, 2, 2, d, z, qmin, f(), None)


def qconv(lib, d, z, qmin, qmax):           # no delta
    f = _fake
    return lib.ssq_qconv_i8_fwd(f(), f(), f(), 1, 16, 4, 4, 16, 3, 3, 1, 1, 1, z, qmin, qmax, f(), None)


def qconv_grouped(lib, d, z, qmin, qmax):   # no delta
    f = _fake
    return lib.ssq_qconv_i8_grouped_fwd(f(), f(), f(), 1, 16, 4, 4, 16, 3, 3, 1, 1, 2, z, qmin, qmax,
                                        f(), None)


def epilogue_codes(lib, d, z, qmin, qmax):  # the output quantizer
    f = _fake
    return lib.ssq_epilogue_codes_fwd(f(), None, None, None, 1, 16, 4, 4, 1, d, z, qmin, qmax, f(),
                                      f(), None)


def codes_res(lib, d, z, qmin, qmax):       # the residual codes' quantizer
    f = _fake
    return lib.ssq_qconv_i8_codes_res_fwd(f(), f(), f(), 1, 16, 4, 4, 16, 3, 3, 1, 1, 1, 0.0, 0, 255,
                                          None, None, None, 1, 0.1, 0.0, 0, 15, f(), f(), None, f(),
                                          d, z, qmin, qmax, None)


def qlinear_pooled(lib, d, z, qmin, qmax):  # no delta
    f = _fake
    return lib.ssq_qlinear_pooled_fwd(f(), f(), f(), f(), f(), 2, 16, 10, 49, z, qmin, qmax, f(), None)


# (entry point, caller, has a delta, has a qmax)
SITES = [("ssq_act_encode", act_encode, True, True),
         ("ssq_act_decode", act_decode, True, False),
         ("ssq_qconv_i8_fwd", qconv, False, True),
         ("ssq_qconv_i8_grouped_fwd", qconv_grouped, False, True),
         ("ssq_epilogue_codes_fwd", epilogue_codes, True, True),
         ("ssq_qconv_i8_codes_res_fwd", codes_res, True, True),
         ("ssq_qlinear_pooled_fwd", qlinear_pooled, False, True)]


@pytest.mark.parametrize("name,fn,has_delta,has_qmax", SITES, ids=[s[0] for s in SITES])
def test_quantizer_check_at_every_site(name, fn, has_delta, has_qmax):
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()

    def refused(word, **kw):
        assert fn(lib, **_q(**kw)) == -1
        msg = lib.ssq_last_error()
        assert name.encode() in msg and word in msg, msg

    for z in (0.5, 256.0, -1.0, float("nan")):
        refused(b"zero point", z=z)
    refused(b"zero point", z=-9.0, qmin=-8, qmax=7)
    if has_qmax:
        refused(b"8-bit", qmin=0, qmax=256)
        refused(b"8-bit", qmin=3, qmax=3)
    else:
        refused(b"qmin", qmin=-129, z=-129.0)
        refused(b"qmin", qmin=1, z=1.0)
    for d in (0.0, -1.0, float("inf"), float("nan")):
        if has_delta:
            refused(b"delta", d=d)
    # the range check comes before the delta's, the delta's before the zero point's
    if has_delta and has_qmax:
        refused(b"8-bit", qmin=0, qmax=256, d=0.0, z=0.5)
        refused(b"delta", d=0.0, z=0.5)
