"""Fused stem (K31, csrc/qinfer_stemconv.hip), host side.

`chain_conv` restates the kernel's contract on the host: every output is the fp32 fma chain
acc_{k+1} = fmaf(x_k, w[co, k], acc_k) from +0 over (ci, r, s) in the weight's memory order, a
padded tap entering as +0.  The fma is vectorised: the float64 product of two float32 is exact
(48 bits), TwoSum gives the exact error of the float64 sum, and rounding that sum to odd before
the float32 conversion makes the double rounding harmless (53 >= 2 * 24 + 2).  It is checked
against libm's fmaf, and the conv against a float64 conv within the chain's a-priori bound.  The
GPU tests import it.  Then the ABI, the flags and the planning of CPU-built models."""
import ctypes as C
import ctypes.util
import inspect
import os
import re

import numpy as np
import pytest
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssq_stem_weight_prepared_bytes", "ssq_stem_weight_prepare", "ssq_stem_conv_fwd",
       "ssq_stem_conv_codes_fwd")
F32 = np.float32


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c), elementwise with broadcasting."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                   # exact
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)               # TwoSum: p + c = s + e exactly
        fin = np.isfinite(s)
        e = np.where(fin, e, 0.0)
        even = (s.view(np.int64) & 1) == 0
        odd = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
        s = np.where(fin & (e != 0) & even, odd, s)  # round to odd
        return s.astype(F32)


def chain_conv(x, w, stride=1, pad=0):
    """K31's contract: x (N, Ci, H, W), w (Co, Ci, R, S) float32 -> y (N, Co, OH, OW) float32."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    N, Ci, H, W = x.shape
    Co, _, R, S = w.shape
    OH, OW = (H + 2 * ph - R) // sh + 1, (W + 2 * pw - S) // sw + 1
    xp = np.zeros((N, Ci, H + 2 * ph, W + 2 * pw), F32)
    xp[:, :, ph:ph + H, pw:pw + W] = x
    acc = np.zeros((N, Co, OH, OW), F32)
    for ci in range(Ci):
        for r in range(R):
            for s in range(S):
                xs = xp[:, ci, r:r + sh * (OH - 1) + 1:sh, s:s + sw * (OW - 1) + 1:sw]
                acc = fma32(xs[:, None], w[None, :, ci, r, s, None, None], acc)
    return acc


def conv64(x, w, stride=1, pad=0):
    """The same conv in float64 (of float64 casts of the operands)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    N, Ci, H, W = x.shape
    Co, _, R, S = w.shape
    OH, OW = (H + 2 * ph - R) // sh + 1, (W + 2 * pw - S) // sw + 1
    xp = np.zeros((N, Ci, H + 2 * ph, W + 2 * pw))
    xp[:, :, ph:ph + H, pw:pw + W] = x
    acc = np.zeros((N, Co, OH, OW))
    for ci in range(Ci):
        for r in range(R):
            for s in range(S):
                xs = xp[:, ci, r:r + sh * (OH - 1) + 1:sh, s:s + sw * (OW - 1) + 1:sw]
                acc += xs[:, None] * w[None, :, ci, r, s, None, None]
    return acc


# ---------------------------------------------------------------- the host fma
def _libm_fmaf():
    lib = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lib.fmaf.restype = C.c_float
    lib.fmaf.argtypes = [C.c_float] * 3
    return lib.fmaf


def _triples():
    rng = np.random.default_rng(31)
    n = 40000
    u = lambda: rng.standard_normal(n).astype(F32)
    wide = lambda: (rng.standard_normal(n) * np.exp2(rng.integers(-60, 60, n))).astype(F32)
    parts = [(u(), u(), u()), (wide(), wide(), wide())]
    # cancellations: c = -fl32(a * b), so the result is the product's rounding error alone
    a, b = u(), u()
    parts.append((a, b, -(a * b)))
    # exact ties: a * b = m + 1/2 ulp-of-the-sum patterns.  a = 1 + 2^-12 * i, b = 1 + 2^-12 * j
    # have a 24-bit-plus product whose tail 2^-24 * i * j meets the half-way point of c's grid
    i, j = rng.integers(1, 4096, n), rng.integers(1, 4096, n)
    a, b = (1 + i * 2.0 ** -12).astype(F32), (1 + j * 2.0 ** -12).astype(F32)
    parts.append((a, b, rng.integers(-8, 8, n).astype(F32)))
    # half-way cases by construction: a * b = 2^-24 (an exact half ulp of c in [1, 2)), c odd / even
    k = rng.integers(0, 1 << 23, n)
    c = (1 + k * 2.0 ** -23).astype(F32)
    half = np.full(n, 2.0 ** -12, F32)
    parts.append((half, half, c))
    parts.append((half, -half, c))
    # subnormal results and signed zeros
    tiny = (rng.standard_normal(n) * 2.0 ** -75).astype(F32)
    parts.append((tiny, tiny, np.where(rng.random(n) < 0.5, F32(0.0), F32(-0.0)).astype(F32)))
    parts.append((tiny, (rng.standard_normal(n) * 2.0 ** -70).astype(F32),
                  (rng.standard_normal(n) * 2.0 ** -149).astype(F32)))
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.4e38, 1e-45], F32)
    g = np.stack(np.meshgrid(specials, specials, specials, indexing="ij"), -1).reshape(-1, 3)
    parts.append((g[:, 0], g[:, 1], g[:, 2]))
    return [np.concatenate([p[i] for p in parts]) for i in range(3)]


def test_fma32_equals_libm_fmaf():
    fmaf = _libm_fmaf()
    a, b, c = _triples()
    assert a.size >= 100000
    got = fma32(a, b, c)
    want = np.array([fmaf(float(p), float(q), float(r)) for p, q, r in zip(a, b, c)], F32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))
    # the ties were real: the fma differs from the two-rounding form somewhere
    with np.errstate(all="ignore"):
        two = ((a * b).astype(F32) + c).astype(F32)
    assert (two[~nan] != want[~nan]).sum() > 1000


CONVS = [((2, 3, 18, 20), 64, (7, 7), 2, 3), ((1, 3, 9, 11), 32, (3, 3), 2, 1),
         ((3, 3, 5, 5), 16, (5, 3), (1, 2), (2, 0)), ((2, 4, 7, 9), 16, (3, 3), 1, 0)]


@pytest.mark.parametrize("xs,Co,ker,stride,pad", CONVS)
def test_chain_conv_within_the_chain_bound_of_a_float64_conv(xs, Co, ker, stride, pad):
    rng = np.random.default_rng(5)
    x = rng.standard_normal(xs).astype(F32)
    w = rng.standard_normal((Co, xs[1]) + ker).astype(F32)
    y = chain_conv(x, w, stride, pad)
    ref = conv64(x, w, stride, pad)
    K = xs[1] * ker[0] * ker[1]
    u = K * 2.0 ** -24
    bound = u / (1 - u) * conv64(np.abs(x), np.abs(w), stride, pad)
    assert y.dtype == F32 and y.shape == ref.shape
    err = np.abs(y.astype(np.float64) - ref)
    assert (err <= bound).all() and err.max() > 0


def test_chain_conv_is_an_fmaf_loop():
    """One output per border class, spelled out with libm's fmaf in (ci, r, s) order."""
    fmaf = _libm_fmaf()
    rng = np.random.default_rng(9)
    x = rng.standard_normal((1, 3, 6, 7)).astype(F32)
    w = rng.standard_normal((2, 3, 5, 3)).astype(F32)
    (sh, sw), (ph, pw) = (1, 2), (2, 1)
    y = chain_conv(x, w, (sh, sw), (ph, pw))
    for oh, ow in ((0, 0), (2, 1), (y.shape[2] - 1, y.shape[3] - 1)):
        for co in range(2):
            acc = 0.0
            for ci in range(3):
                for r in range(5):
                    for s in range(3):
                        h, v = oh * sh + r - ph, ow * sw + s - pw
                        xv = float(x[0, ci, h, v]) if 0 <= h < 6 and 0 <= v < 7 else 0.0
                        acc = fmaf(xv, float(w[co, ci, r, s]), acc)
            assert F32(acc).view(np.int32) == y[0, co, oh, ow].view(np.int32)


# ---------------------------------------------------------------- ABI
def test_new_symbols_declared_exported_and_bound():
    from shiftedscalequantization_amd import _capi
    from shiftedscalequantization_amd.build import SOURCES
    src = open(os.path.join(ROOT, "include", "ssq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _capi.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, src)
        assert m and hasattr(lib, s) and s in _capi.SIGNATURES, s
        assert len(_capi.SIGNATURES[s][1]) == m.group(1).count(",") + 1, s
        assert s in doc, s
    assert "qinfer_stemconv.hip" in SOURCES


def test_prepared_bytes_is_zero_for_a_refused_geometry():
    from shiftedscalequantization_amd import _capi
    nbytes = _capi.load().ssq_stem_weight_prepared_bytes
    assert nbytes(64, 3, 7, 7) >= 147 * 64 * 4 and nbytes(64, 3, 7, 7) % 16 == 0
    assert nbytes(1, 1, 1, 1) > 0 and nbytes(72, 4, 7, 7) >= 196 * 72 * 4
    for geo in ((64, 5, 3, 3), (64, 0, 3, 3), (64, 3, 8, 3), (64, 3, 3, 8), (64, 3, 0, 3),
                (0, 3, 3, 3), (-1, 3, 3, 3)):
        assert nbytes(*geo) == 0, geo


def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


def _conv(lib, codes, x=True, blob=True, nbytes=None, y=True, bad=True, geo=(1, 3, 8, 8, 16, 3, 3),
          stride=(1, 1), pad=(1, 1), d=0.1):
    f = _fake
    if nbytes is None:
        nbytes = lib.ssq_stem_weight_prepared_bytes(geo[4], geo[1], geo[5], geo[6])
    head = (f() if x else None, f() if blob else None, nbytes, *geo, *stride, *pad)
    if codes:
        return lib.ssq_stem_conv_codes_fwd(*head, None, None, None, 1, d, 0.0, 0, 255,
                                           f() if y else None, f() if bad else None, None)
    return lib.ssq_stem_conv_fwd(*head, f() if y else None, None)


@pytest.mark.parametrize("codes", [False, True])
def test_stem_conv_refuses_bad_arguments_without_gpu(codes):
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    err = lib.ssq_last_error
    run = lambda **kw: _conv(lib, codes, **kw)
    for kw in (dict(x=False), dict(blob=False), dict(y=False)):
        assert run(**kw) == -1 and b"null" in err()
    assert run(geo=(1, 5, 8, 8, 16, 3, 3), nbytes=1 << 20) == -1 and b"stem geometry" in err()
    assert run(geo=(1, 3, 8, 8, 16, 8, 3), nbytes=1 << 20) == -1 and b"stem geometry" in err()
    assert run(geo=(1, 3, 8, 8, 16, 3, 8), nbytes=1 << 20) == -1 and b"stem geometry" in err()
    assert run(geo=(1, 3, 8, 8, 0, 3, 3), nbytes=1 << 20) == -1 and b"stem geometry" in err()
    assert run(pad=(3, 1)) == -1 and b"padding" in err()
    assert run(pad=(1, 3)) == -1 and b"padding" in err()
    assert run(pad=(-1, 1)) == -1 and b"padding" in err()
    assert run(stride=(0, 1)) == -1 and b"geometry" in err()
    assert run(geo=(0, 3, 8, 8, 16, 3, 3)) == -1 and b"geometry" in err()
    assert run(geo=(1, 3, 2, 8, 16, 7, 3), pad=(0, 1)) == -1 and b"empty output" in err()
    full = lib.ssq_stem_weight_prepared_bytes(16, 3, 3, 3)
    assert run(nbytes=full - 1) == -1 and b"prepared blob" in err()
    assert run(geo=(1 << 16, 3, 128, 128, 16, 3, 3)) == -1 and b"2^31" in err()
    if codes:
        assert run(bad=False) == -1 and b"null" in err()
        assert run(d=0.0) == -1 and b"delta" in err()
    f = _fake
    assert lib.ssq_stem_weight_prepare(None, 16, 3, 3, 3, f(), None) == -1 and b"null" in err()
    assert lib.ssq_stem_weight_prepare(f(), 16, 5, 3, 3, f(), None) == -1 and b"geometry" in err()


def test_wrappers_refuse_without_gpu():
    import torch
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    with pytest.raises(SSQError):
        K.stem_weight_prepare(torch.zeros(16, 3, 3, 3))              # a CPU tensor
    with pytest.raises(SSQError, match="stem_weight_prepare"):
        K.stem_conv(torch.zeros(1, 3, 8, 8), object())
    sw = K.StemWeight(torch.zeros(16, dtype=torch.uint8), (16, 3, 3, 3))
    with pytest.raises(SSQError, match="bad is required"):
        K.stem_conv_codes(torch.zeros(1, 3, 8, 8), sw, None, None, None, 1, 0.1, 0.0, 8, False, None)
    assert K.stem_geometry_reason(64, 3, 7, 7, 2, 3) is None
    assert K.stem_geometry_reason(32, 3, 3, 3, (2, 2), (1, 1)) is None
    assert "geometry" in K.stem_geometry_reason(64, 5, 3, 3, 1, 1)
    assert "geometry" in K.stem_geometry_reason(64, 3, 3, 3, 1, 3)
    assert "geometry" in K.stem_geometry_reason(64, 3, 3, 3, 1, 1, dilation=2)
    assert K.stem_geometry_reason(64, 2, 3, 3, 1, 1, groups=2) == "grouped conv"


# ---------------------------------------------------------------- CLI, API
def test_cli_int_infer_fused_stem_implies_the_flags_below_it():
    from shiftedscalequantization_amd.cli import parse_args
    a = parse_args(["--int_infer_fused_stem"])
    assert (a.int_infer_fused_stem and a.int_infer_carry_stem and a.int_infer_carry_blocks
            and a.int_infer_carry and a.int_infer)
    a = parse_args(["--int_infer_carry_stem"])
    assert a.int_infer_carry_stem and not a.int_infer_fused_stem
    assert not parse_args([]).int_infer_fused_stem


def test_fused_stem_is_a_keyword_with_default_false():
    from shiftedscalequantization_amd import quant as Q
    p = inspect.signature(Q.enable_integer_inference).parameters["fused_stem"]
    assert p.default is False


# ---------------------------------------------------------------- planning
def cpu_qnn(arch):
    from shiftedscalequantization_amd import drivers as D
    return D.build_qnn(arch, 2, 4, device="cpu")


@pytest.mark.parametrize("arch,geo", [("resnet18", (64, 3, 7, 7)), ("mobilenetv2", (32, 3, 3, 3)),
                                      ("regnetx_600m", (32, 3, 3, 3))])
def test_zoo_stems_are_inside_the_geometry(arch, geo):
    from shiftedscalequantization_amd.quant import stem_edges
    from shiftedscalequantization_amd.quant.integer import fused_stem_reason
    qnn = cpu_qnn(arch)
    (producer, _, _), = stem_edges(qnn)
    assert tuple(producer.weight.shape) == geo
    assert fused_stem_reason(producer) is None


def test_stems_outside_the_geometry_are_reported_with_their_reason():
    import torch
    from shiftedscalequantization_amd.quant import stem_edges
    from shiftedscalequantization_amd.quant.integer import fused_stem_reason
    qnn = cpu_qnn("resnet18")
    (producer, _, _), = stem_edges(qnn)
    w = producer.weight
    producer.weight = nn.Parameter(torch.zeros(64, 5, 7, 7))
    assert "geometry" in fused_stem_reason(producer) and "Ci 5" in fused_stem_reason(producer)
    producer.weight = nn.Parameter(torch.zeros(64, 2, 7, 7))
    producer.fwd_kwargs = dict(producer.fwd_kwargs, groups=2)
    assert fused_stem_reason(producer) == "grouped conv"
    producer.weight, producer.fwd_kwargs = w, dict(producer.fwd_kwargs, groups=1)
    assert fused_stem_reason(producer) is None


def test_shape_rule_knob(monkeypatch):
    from shiftedscalequantization_amd.quant.integer import stem_fused_takes
    geo = ((64, 3, 7, 7), (64, 3, 224, 224), (2, 2), (3, 3))
    monkeypatch.setenv("SSQ_STEM_FUSED", "1")
    assert stem_fused_takes(*geo) is True
    monkeypatch.setenv("SSQ_STEM_FUSED", "0")
    assert stem_fused_takes(*geo) is False
    monkeypatch.setenv("SSQ_STEM_FUSED", "auto")
    assert stem_fused_takes(*geo) in (True, False)


def test_report_names_fused_only_under_a_fused_plan():
    from shiftedscalequantization_amd import quant as Q
    qnn = cpu_qnn("resnet18")
    assert "fused" not in Q.stem_carry_report(qnn)
    qnn._int_fused_stem = {}              # what enable_integer_inference(fused_stem=True) leaves
    rep = Q.stem_carry_report(qnn)
    assert rep["edges"] == [] and rep["fused"] == {} and rep["unfused"] == {}
    Q.disable_integer_inference(qnn)
    assert "fused" not in Q.stem_carry_report(qnn)
