"""uint8 stem (K32, csrc/qinfer_stemu8.hip), host side.

`u8_stem_ref` restates the kernel's contract ("uint8 stem (K32)") in numpy: the two fp32
tables in their stated operation order, the integer sums through the stored shifted operands
(w_s = q - (qmin + 128), u_s = u - 128, 0 on a padded tap) and the correction identities, and the
fp32 part one float32 operation at a time (no FMA, so numpy float32 gives the kernel's bits).  Its
integer sums are checked against a direct int64 sum over the valid taps, its values against the
float64 decoded conv within the counted bound.  The GPU tests import it.  Then the ABI, the
refusals, the flag and the report's keys."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from test_qinfer_host import qrange

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssq_stem_u8_weight_prepared_bytes", "ssq_stem_u8_weight_prepare", "ssq_stem_u8_tiles",
       "ssq_stem_conv_u8_fwd", "ssq_stem_conv_u8_codes_fwd")
F32 = np.float32
MEAN, STD = (0.485, 0.456, 0.406, 0.45), (0.229, 0.224, 0.225, 0.226)


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def rounding_count(Ci):
    """The roundings between the exact value and y, as DESIGN counts them: M one, 1 / (255 std)
    two, s one, M * B one, the subtraction one, the product one, the Ci - 1 adds, the reference's
    own decode of W_hat one, second-order terms one: 11 at Ci = 3."""
    return 1 + 2 + 1 + 1 + 1 + 1 + (Ci - 1) + 1 + 1


def pack_codes(qw, qmin, n_bits):
    """Integer codes (any shape, memory order) -> the export's packed bytes: code - qmin in 2, 4 or
    8 storage bits, element i at bit i * bits, low bits first."""
    bs = 2 if n_bits <= 2 else (4 if n_bits <= 4 else 8)
    c = (np.asarray(qw, np.int64).reshape(-1) - qmin).astype(np.uint8)
    per = 8 // bs
    c = np.concatenate([c, np.zeros((-c.size) % per, np.uint8)]).reshape(-1, per)
    out = np.zeros(c.shape[0], np.uint8)
    for j in range(per):
        out |= (c[:, j] << (bs * j)).astype(np.uint8)
    return out


def windows(a, R, S, stride, pad):
    """a (N, Ci, H, W) -> (N, Ci, R, S, OH, OW): the value under every tap of every output, 0 on a
    padded tap."""
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    N, Ci, H, W = a.shape
    OH, OW = (H + 2 * ph - R) // sh + 1, (W + 2 * pw - S) // sw + 1
    ap = np.zeros((N, Ci, H + 2 * ph, W + 2 * pw), a.dtype)
    ap[:, :, ph:ph + H, pw:pw + W] = a
    out = np.zeros((N, Ci, R, S, OH, OW), a.dtype)
    for r in range(R):
        for s in range(S):
            out[:, :, r, s] = ap[:, :, r:r + sh * (OH - 1) + 1:sh, s:s + sw * (OW - 1) + 1:sw]
    return out


def direct_sums(u, qw, zw, stride, pad):
    """(A, B) as (N, Co, Ci, OH, OW) int64, the contract's definition: over the valid taps,
    B_c = sum (q_w - z_w[co]) and A_c = sum (q_w - z_w[co]) * u."""
    Co, Ci, R, S = qw.shape
    c = np.asarray(qw, np.int64) - np.asarray(zw, np.int64).reshape(-1, 1, 1, 1)
    uw = windows(np.asarray(u, np.int64), R, S, stride, pad)
    vw = windows(np.ones(u.shape, np.int64), R, S, stride, pad)
    A = np.einsum("ocrs,ncrshw->nochw", c, uw)
    B = np.einsum("ocrs,ncrshw->nochw", c, vw)
    return A, B


def shifted_sums(u, qw, zw, qmin, stride, pad):
    """(A, B) from the kernel's stored operands and its correction identities."""
    Co, Ci, R, S = qw.shape
    ws = np.asarray(qw, np.int64) - (qmin + 128)
    assert ws.min() >= -128 and ws.max() <= 127
    us = windows(np.asarray(u, np.int64) - 128, R, S, stride, pad)
    valid = windows(np.ones(u.shape, np.int64), R, S, stride, pad)
    us = us * valid                                               # u_s = 0 on a padded tap
    assert us.min() >= -128 and us.max() <= 127
    cwz = (qmin + 128 - np.asarray(zw, np.int64)).reshape(1, -1, 1, 1, 1)
    D = np.einsum("ocrs,ncrshw->nochw", ws, us)
    E = np.einsum("ocrs,ncrshw->nochw", ws, valid)
    SU = us.sum((2, 3))[:, None]                                  # (N, 1, Ci, OH, OW)
    NV = valid.sum((2, 3))[:, None]
    B = E + cwz * NV
    A = D + cwz * SU + 128 * B
    return A, B


def u8_tables_ref(mean, std, d, Co, Ci):
    """M[c] = fp32(255 * mean[c]); s[co, c] = fp32(fp32(1 / fp32(255 * std[c])) * d[co, c])."""
    mean, std = np.asarray(mean, F32)[:Ci], np.asarray(std, F32)[:Ci]
    d = np.asarray(d, F32)
    d = np.broadcast_to(d.reshape(Co, 1), (Co, Ci)) if d.size == Co else d.reshape(Co, Ci)
    M = F32(255) * mean
    inv = F32(1) / (F32(255) * std)
    s = inv.reshape(1, Ci) * d
    assert M.dtype == F32 and s.dtype == F32
    return M, np.ascontiguousarray(s)


def u8_stem_ref(u, qw, zw, qmin, d, mean, std, stride, pad):
    """K32's fp32 form: u (N, Ci, H, W) uint8, qw (Co, Ci, R, S) integer codes, zw[co] integer,
    d[co] or d[co, ci] -> y (N, Co, OH, OW) float32."""
    Co, Ci = qw.shape[:2]
    M, s = u8_tables_ref(mean, std, d, Co, Ci)
    A, B = shifted_sums(u, qw, zw, qmin, stride, pad)
    assert np.abs(A).max() < 2 ** 24 and np.abs(B).max() < 2 ** 24
    y = None
    for c in range(Ci):
        fa, fb = A[:, :, c].astype(F32), B[:, :, c].astype(F32)
        t = fa - M[c] * fb                                        # two float32 roundings
        p = t * s[None, :, c, None, None]
        y = p if y is None else y + p
        assert t.dtype == F32 and y.dtype == F32
    return y


def decoded64(u, qw, zw, d, mean, std, stride, pad):
    """(Y64, the bound's magnitude): the float64 conv of the fp32 decoded weight with
    x = (u / 255 - mean_c) / std_c in float64 from the fp32 mean, std, and
    sum |W_hat| (u + |M_c|) / (255 std_c)."""
    Co, Ci, R, S = qw.shape
    M, _ = u8_tables_ref(mean, std, np.ones(Co, F32), Co, Ci)
    d = np.asarray(d, F32)
    d = np.broadcast_to(d.reshape(Co, 1), (Co, Ci)) if d.size == Co else d.reshape(Co, Ci)
    what = ((np.asarray(qw, np.int64) - np.asarray(zw, np.int64).reshape(-1, 1, 1, 1)).astype(F32)
            * d[:, :, None, None])
    assert what.dtype == F32
    mean64 = np.asarray(mean, F32)[:Ci].astype(np.float64).reshape(1, -1, 1, 1)
    std64 = np.asarray(std, F32)[:Ci].astype(np.float64).reshape(1, -1, 1, 1)
    x = (np.asarray(u, np.float64) / 255 - mean64) / std64
    valid = windows(np.ones(u.shape), R, S, stride, pad)
    xw = windows(x, R, S, stride, pad)
    y = np.einsum("ocrs,ncrshw->nohw", what.astype(np.float64), xw)
    mag = (np.asarray(u, np.float64) + np.abs(M.astype(np.float64)).reshape(1, -1, 1, 1)) / (255 * std64)
    mw = windows(mag, R, S, stride, pad) * valid
    return y, np.einsum("ocrs,ncrshw->nohw", np.abs(what.astype(np.float64)), mw)


# name: (u shape, Co, (R, S), stride, padding): the tiling's edges (the GPU file's table)
CASES = {
    "r7": ((2, 3, 19, 37), 64, (7, 7), (2, 2), (3, 3)),
    "m3": ((2, 3, 17, 33), 72, (3, 3), (2, 2), (1, 1)),
    "s1": ((1, 4, 9, 40), 8, (3, 3), (1, 1), (1, 1)),
    "rect": ((1, 1, 12, 35), 8, (5, 3), (2, 1), (2, 0)),
}


def draw(name, n_bits=8, sym=False, per_ci=False):
    """(u, qw, zw, qmin, d) of a case: random image and codes, integer zero points in range."""
    us, Co, ker, _, _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) * 10 + n_bits + 100 * sym + 1000 * per_ci)
    lo, hi = qrange(n_bits, sym)
    u = rng.integers(0, 256, us).astype(np.uint8)
    qw = rng.integers(lo, hi + 1, (Co, us[1]) + ker)
    zw = rng.integers(lo, hi + 1, Co)
    d = rng.uniform(0.002, 0.02, (Co, us[1]) if per_ci else Co).astype(F32)
    return u, qw, zw, lo, d


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("n_bits,sym", [(8, False), (8, True), (4, False), (2, True)])
def test_shifted_sums_equal_the_direct_sums(name, n_bits, sym):
    u, qw, zw, qmin, _ = draw(name, n_bits, sym)
    _, _, _, stride, pad = CASES[name]
    A, B = shifted_sums(u, qw, zw, qmin, stride, pad)
    A0, B0 = direct_sums(u, qw, zw, stride, pad)
    assert np.array_equal(A, A0) and np.array_equal(B, B0)


def test_extremes_reach_the_bound_of_A():
    """Both code extremes with the zero point at the other end, images of all 0 and all 255:
    |A_c| reaches 49 * 255 * 255 < 2^24 at an interior pixel of a 7x7 window."""
    us, Co, ker, stride, pad = CASES["r7"]
    for q, z in ((255, 0), (0, 255)):
        qw, zw = np.full((Co, us[1]) + ker, q), np.full(Co, z)
        for fill in (0, 255):
            u = np.full(us, fill, np.uint8)
            A, B = shifted_sums(u, qw, zw, 0, stride, pad)
            A0, B0 = direct_sums(u, qw, zw, stride, pad)
            assert np.array_equal(A, A0) and np.array_equal(B, B0)
            assert np.abs(B).max() == 49 * 255
            assert np.abs(A).max() == (49 * 255 * 255 if fill else 0) < 2 ** 24
            # a corner pixel sees 4 x 4 of the 7 x 7 taps: a padded tap is x = 0, not u = 0
            assert abs(B[0, 0, 0, 0, 0]) == 16 * 255


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("per_ci", [False, True])
def test_ref_within_the_counted_bound_of_the_decoded_conv(name, per_ci):
    u, qw, zw, qmin, d = draw(name, 8, False, per_ci)
    _, _, _, stride, pad = CASES[name]
    Ci = u.shape[1]
    y = u8_stem_ref(u, qw, zw, qmin, d, MEAN, STD, stride, pad)
    y64, mag = decoded64(u, qw, zw, d, MEAN, STD, stride, pad)
    c = rounding_count(Ci)
    assert rounding_count(3) == 11 and c == 8 + Ci
    err = np.abs(y.astype(np.float64) - y64)
    worst = float((err / (2.0 ** -24 * mag)).max())
    print(f"{name} per_ci={per_ci}: worst |y - Y64| = {worst:.3f} x 2^-24 x magnitude (bound {c})")
    assert (err <= c * 2.0 ** -24 * mag).all() and err.max() > 0


def test_tables_operation_order():
    from shiftedscalequantization_amd import kernels as K
    rng = np.random.default_rng(3)
    for Co, Ci, per_ci in ((64, 3, False), (8, 4, True), (5, 1, False)):
        d = rng.uniform(1e-3, 0.05, (Co, Ci) if per_ci else Co).astype(F32)
        mean, std = rng.uniform(0.3, 0.6, Ci).astype(F32), rng.uniform(0.15, 0.3, Ci).astype(F32)
        M, s = K.stem_u8_tables(torch.tensor(mean), torch.tensor(std), torch.tensor(d), Co, Ci)
        Mr, sr = u8_tables_ref(mean, std, d, Co, Ci)
        assert M.dtype == torch.float32 and tuple(s.shape) == (Co, Ci) and s.is_contiguous()
        assert np.array_equal(M.numpy().view(np.int32), Mr.view(np.int32))
        assert np.array_equal(s.numpy().view(np.int32), sr.view(np.int32))
    # the order matters: 1 / (255 std) * d is not d / (255 std) everywhere
    d = rng.uniform(1e-3, 0.05, 4096).astype(F32)
    _, s = u8_tables_ref([0.5], [0.229], d, 4096, 1)
    other = d / (F32(255) * F32(0.229))
    assert (s[:, 0] != other).any()
    from shiftedscalequantization_amd._capi import SSQError
    with pytest.raises(SSQError, match="entries"):
        K.stem_u8_tables(torch.zeros(2), torch.ones(3), torch.ones(8), 8, 3)
    with pytest.raises(SSQError, match="scale"):
        K.stem_u8_tables(torch.zeros(3), torch.ones(3), torch.ones(9), 8, 3)


def test_pack_codes_layout():
    assert pack_codes([0, 1, 2, 3, 3], 0, 2).tolist() == [0b11100100, 0b11]
    assert pack_codes([-8, 7, 0], -8, 4).tolist() == [0xF0, 0x08]
    assert pack_codes([-128, 127], -128, 8).tolist() == [0, 255]


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
    assert "qinfer_stemu8.hip" in SOURCES


def test_prepared_bytes_and_tiles():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    nbytes = lib.ssq_stem_u8_weight_prepared_bytes
    assert nbytes(64, 3, 7, 7) == 3 * 64 * 64 + 64 * 4 + 3 * 64 * 4
    assert nbytes(72, 4, 3, 3) == 4 * 80 * 64 + 80 * 4 + 4 * 80 * 4
    for geo in ((64, 5, 3, 3), (64, 0, 3, 3), (64, 3, 8, 3), (64, 3, 3, 8), (0, 3, 3, 3)):
        assert nbytes(*geo) == 0, geo
    a, b = C.c_int64(), C.c_int64()
    tiles = lambda *g: (lib.ssq_stem_u8_tiles(*g, C.byref(a), C.byref(b)), a.value, b.value)
    # 96 x 160 under 7x7/2 pad 3: 48 x 80 outputs, 2-row tiles of 32 columns = 24 x 3 tiles; the
    # first and last tile rows and the first and last tile columns touch the border
    assert tiles(1, 3, 96, 160, 64, 7, 7, 2, 2, 3, 3, 1) == (0, 22, 50)
    # no padding: every full tile is interior; the column tail's unstored pixels reach outside
    assert tiles(1, 3, 10, 66, 16, 3, 3, 1, 1, 0, 0, 1) == (0, 8, 0)
    assert tiles(1, 3, 10, 67, 16, 3, 3, 1, 1, 0, 0, 1) == (0, 8, 4)
    assert tiles(1, 5, 10, 67, 16, 3, 3, 1, 1, 0, 0, 1)[0] == -1


def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


def _conv(lib, codes, u=True, blob=True, M=True, s=True, nbytes=None, y=True, bad=True,
          geo=(1, 3, 8, 8, 16, 3, 3), stride=(1, 1), pad=(1, 1), d=0.1):
    f = _fake
    if nbytes is None:
        nbytes = lib.ssq_stem_u8_weight_prepared_bytes(geo[4], geo[1], geo[5], geo[6])
    head = (f() if u else None, f() if blob else None, nbytes, f() if M else None,
            f() if s else None, *geo, *stride, *pad, 0)
    if codes:
        return lib.ssq_stem_conv_u8_codes_fwd(*head, None, None, None, 1, d, 0.0, 0, 255,
                                              f() if y else None, f() if bad else None, None)
    return lib.ssq_stem_conv_u8_fwd(*head, f() if y else None, None)


@pytest.mark.parametrize("codes", [False, True])
def test_stem_conv_u8_refuses_bad_arguments_without_gpu(codes):
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    err = lib.ssq_last_error
    run = lambda **kw: _conv(lib, codes, **kw)
    for kw in (dict(u=False), dict(blob=False), dict(M=False), dict(s=False), dict(y=False)):
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
    full = lib.ssq_stem_u8_weight_prepared_bytes(16, 3, 3, 3)
    assert run(nbytes=full - 1) == -1 and b"prepared blob" in err()
    assert run(geo=(1 << 16, 3, 128, 128, 16, 3, 3)) == -1 and b"2^31" in err()
    if codes:
        assert run(bad=False) == -1 and b"null" in err()
        assert run(d=0.0) == -1 and b"delta" in err()
    f = _fake
    # the blob is read as 16-byte vectors
    off = C.c_void_p(260)
    if codes:
        rc = lib.ssq_stem_conv_u8_codes_fwd(f(), off, full, f(), f(), 1, 3, 8, 8, 16, 3, 3, 1, 1, 1, 1,
                                            0, None, None, None, 1, 0.1, 0.0, 0, 255, f(), f(), None)
    else:
        rc = lib.ssq_stem_conv_u8_fwd(f(), off, full, f(), f(), 1, 3, 8, 8, 16, 3, 3, 1, 1, 1, 1, 0,
                                      f(), None)
    assert rc == -1 and b"16-byte aligned" in err()
    prep = lib.ssq_stem_u8_weight_prepare
    assert prep(f(), f(), 16, 3, 3, 3, 8, 0, off, f(), None) == -1 and b"16-byte aligned" in err()
    assert prep(None, f(), 16, 3, 3, 3, 8, 0, f(), f(), None) == -1 and b"null" in err()
    assert prep(f(), f(), 16, 3, 3, 3, 8, 0, f(), None, None) == -1 and b"null" in err()
    assert prep(f(), f(), 16, 5, 3, 3, 8, 0, f(), f(), None) == -1 and b"geometry" in err()
    assert prep(f(), f(), 16, 3, 3, 3, 9, 0, f(), f(), None) == -1 and b"n_bits" in err()
    assert prep(f(), f(), 16, 3, 3, 3, 4, -4, f(), f(), None) == -1 and b"qmin" in err()


def test_wrappers_refuse_without_gpu():
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    with pytest.raises(SSQError, match="uint8"):
        K.stem_u8_weight_prepare(torch.zeros(16), (16, 3, 3, 3), torch.zeros(16), 8, 0)
    with pytest.raises(SSQError):
        K.stem_u8_weight_prepare(torch.zeros(432, dtype=torch.uint8), (16, 3, 3, 3),
                                 torch.zeros(16), 8, 0)                  # a CPU tensor
    with pytest.raises(SSQError, match="stem_u8_weight_prepare"):
        K.stem_conv_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), object(), None, None)
    sw = K.StemU8Weight(torch.zeros(16, dtype=torch.uint8), (16, 3, 3, 3), None)
    with pytest.raises(SSQError, match="uint8"):
        K.stem_conv_u8(torch.zeros(1, 3, 8, 8), sw, torch.zeros(3), torch.zeros(16, 3))
    with pytest.raises(SSQError, match="bad is required"):
        K.stem_conv_u8_codes(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), sw, torch.zeros(3),
                             torch.zeros(16, 3), None, None, None, 1, 0.1, 0.0, 8, False, None)
    ok = K.stem_u8_geometry_reason
    assert ok(64, 3, 7, 7, 2, 3) is None and ok(32, 3, 3, 3, (2, 2), (1, 1)) is None
    assert ok(8, 1, 5, 3, (2, 1), (2, 0)) is None
    assert ok(64, 2, 3, 3, 1, 1, groups=2) == "grouped conv"
    assert "Ci = 5" in ok(64, 5, 3, 3, 1, 1)
    assert "kernel 8x3" in ok(64, 3, 8, 3, 1, 1) and "kernel 3x9" in ok(64, 3, 3, 9, 1, 1)
    assert "dilation" in ok(64, 3, 3, 3, 1, 1, dilation=2)
    assert "padding" in ok(64, 3, 3, 3, 1, 3) and "padding" in ok(64, 3, 3, 3, 1, (3, 1))


# ---------------------------------------------------------------- CLI, API
def test_cli_int_infer_u8_images_implies_nothing_but_int_infer():
    from shiftedscalequantization_amd.cli import parse_args
    a = parse_args(["--int_infer_carry_head", "--int_infer_u8_images"])
    assert a.int_infer_u8_images and a.int_infer_carry_stem and a.int_infer
    assert not a.int_infer_fused_stem
    assert not parse_args([]).int_infer_u8_images
    with pytest.raises(SystemExit):
        parse_args(["--int_infer_u8_images"])          # needs a stem edge: carry_stem / carry_head


def test_image_u8_is_a_keyword_with_default_none_and_needs_a_stem_edge():
    from shiftedscalequantization_amd import quant as Q
    p = inspect.signature(Q.enable_integer_inference).parameters["image_u8"]
    assert p.default is None
    qnn = cpu_qnn("resnet18")
    with pytest.raises(ValueError, match="stem edge"):
        Q.enable_integer_inference(qnn, torch.zeros(1, 3, 32, 32), image_u8=(MEAN[:3], STD[:3]))


# ---------------------------------------------------------------- planning
def cpu_qnn(arch):
    from shiftedscalequantization_amd import drivers as D
    return D.build_qnn(arch, 2, 4, device="cpu")


def fields(Co, zp=None, col=None, qmin=0):
    zp = torch.zeros(Co) if zp is None else zp
    return dict(zero_point=zp, col_scale=col, qmin=qmin, kind="test", per_ci=False)


@pytest.mark.parametrize("arch", ["resnet18", "mobilenetv2", "regnetx_600m"])
def test_zoo_stems_pass(arch):
    from shiftedscalequantization_amd.quant import stem_edges
    from shiftedscalequantization_amd.quant.integer import u8_stem_reason
    (producer, _, _), = stem_edges(cpu_qnn(arch))
    assert u8_stem_reason(producer) is None
    assert u8_stem_reason(producer, fields(producer.weight.shape[0])) is None


def test_every_refusal_reason():
    from shiftedscalequantization_amd.quant import stem_edges
    from shiftedscalequantization_amd.quant.integer import u8_stem_reason
    qnn = cpu_qnn("resnet18")
    (m, _, _), = stem_edges(qnn)
    w, kw = m.weight, dict(m.fwd_kwargs)
    Co = int(w.shape[0])
    # a column-scaled stem weight
    why = u8_stem_reason(m, fields(Co, col=torch.ones(147)))
    assert "column scale" in why and "two-digit" in why
    # a zero point that is not an integer code
    zp = torch.zeros(Co)
    zp[3] = 0.5
    assert u8_stem_reason(m, fields(Co, zp)) == "weight zero point is not an integer code"
    zp[3] = 600.0
    assert u8_stem_reason(m, fields(Co, zp)) == "weight zero point is not an integer code"
    zp[3] = 255.0
    assert u8_stem_reason(m, fields(Co, zp)) is None
    # a grouped stem
    m.weight = nn.Parameter(torch.zeros(64, 2, 7, 7))
    m.fwd_kwargs = dict(kw, groups=2)
    assert u8_stem_reason(m) == "grouped conv"
    m.fwd_kwargs = dict(kw)
    # Ci > 4; R or S > 7
    m.weight = nn.Parameter(torch.zeros(64, 5, 7, 7))
    assert "Ci = 5" in u8_stem_reason(m)
    m.weight = nn.Parameter(torch.zeros(64, 3, 9, 7))
    assert "kernel 9x7" in u8_stem_reason(m)
    m.weight = nn.Parameter(torch.zeros(64, 3, 7, 8))
    assert "kernel 7x8" in u8_stem_reason(m)
    m.weight = w
    # dilation != 1; padding not below the kernel, or a string
    m.fwd_kwargs = dict(kw, dilation=(2, 2))
    assert "dilation" in u8_stem_reason(m)
    m.fwd_kwargs = dict(kw, padding=(7, 3))
    assert "padding" in u8_stem_reason(m)
    m.fwd_kwargs = dict(kw, padding="same")
    assert "padding" in u8_stem_reason(m)
    m.fwd_kwargs = dict(kw)
    assert u8_stem_reason(m) is None
    # a producer with hooks
    h = m.register_forward_hook(lambda *a: None)
    assert "hook" in u8_stem_reason(m)
    h.remove()
    assert u8_stem_reason(m) is None
    # not a conv
    import torch.nn.functional as Fn
    fc = [q for q in qnn.modules() if getattr(q, "fwd_func", None) is Fn.linear][-1]
    assert u8_stem_reason(fc) == "not a conv"


def test_shape_rule_knob(monkeypatch):
    from shiftedscalequantization_amd.quant.integer import stem_u8_takes
    geo = ((64, 3, 7, 7), (64, 3, 224, 224), (2, 2), (3, 3))
    monkeypatch.setenv("SSQ_STEM_U8", "1")
    assert stem_u8_takes(*geo) is True
    monkeypatch.setenv("SSQ_STEM_U8", "0")
    assert stem_u8_takes(*geo) is False
    # auto: the measured classes (profiles/int_infer_u8_stem_rate.txt) -- the 7x7/2 stem on 32 x 32
    # images at batch 64 cleared the keep rule, the two 224 x 224 shapes did not
    monkeypatch.setenv("SSQ_STEM_U8", "auto")
    assert stem_u8_takes(*geo) is False
    assert stem_u8_takes((64, 3, 7, 7), (64, 3, 32, 32), (2, 2), (3, 3)) is True
    assert stem_u8_takes((64, 3, 7, 7), (2, 3, 32, 32), (2, 2), (3, 3)) is True
    assert stem_u8_takes((32, 3, 3, 3), (64, 3, 224, 224), (2, 2), (1, 1)) is False
    assert stem_u8_takes((32, 3, 3, 3), (64, 3, 32, 32), (2, 2), (1, 1)) is False
    # nothing outside the measured class: another kernel, another stride, more pixels
    assert stem_u8_takes((64, 3, 5, 5), (64, 3, 32, 32), (2, 2), (2, 2)) is False
    assert stem_u8_takes((64, 3, 7, 7), (64, 3, 32, 32), (1, 1), (3, 3)) is False
    assert stem_u8_takes((64, 3, 7, 7), (65, 3, 32, 32), (2, 2), (3, 3)) is False
    monkeypatch.delenv("SSQ_STEM_U8")
    assert stem_u8_takes(*geo) is False


def test_report_keys_with_and_without_the_keyword():
    from shiftedscalequantization_amd import quant as Q
    qnn = cpu_qnn("resnet18")
    base = set(Q.stem_carry_report(qnn))
    assert base == {"edges", "calls", "pooled"}
    qnn._int_u8 = {}                      # what enable_integer_inference(image_u8=...) leaves
    rep = Q.stem_carry_report(qnn)
    assert set(rep) == base | {"u8", "un_u8"} and rep["u8"] == {} and rep["un_u8"] == {}
    qnn._int_fused_stem = {}
    assert set(Q.stem_carry_report(qnn)) == base | {"u8", "un_u8", "fused", "unfused"}
    Q.disable_integer_inference(qnn)
    assert set(Q.stem_carry_report(qnn)) == base


def test_normalise_u8_is_the_three_torch_operations():
    from shiftedscalequantization_amd.quant.integer import normalise_u8
    u = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 16, 16).repeat(1, 3, 1, 1)
    mean = torch.tensor(MEAN[:3]).reshape(1, 3, 1, 1)
    std = torch.tensor(STD[:3]).reshape(1, 3, 1, 1)
    want = ((u.float() / 255) - mean) / std
    assert torch.equal(normalise_u8(u, mean, std), want)
