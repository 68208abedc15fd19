"""Integer inference of per-(co, ci) scaled weights and of the wide operand, host side: the grid
rule of kernels.perci_grid (one L, an fp32 base per row, an integer k per element with
fp32(base * fp32(k / L)) == scale bit for bit; the smallest L, then the smallest k at the row's
maximum, then the smaller base), colscale_grid's new limits, the two-digit split with a host
int64 reference of the wide sum, the new ABI, the flags, and the numpy references the GPU tests
compare against (test_qinfer_perci_gpu.py and test_qinfer_wide_gpu.py import them)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_qinfer_host import conv_i64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssq_qweight_prepare_perci", "ssq_qweight_prepare_grouped_perci",
       "ssq_qweight_prepared_bytes_wide", "ssq_qweight_prepare_wide", "ssq_qconv_i8_wide_fwd",
       "ssq_qconv_i8_wide_codes_fwd", "ssq_qconv_i8_wide_codes_res_fwd")
F32 = np.float32
SHIFT = (31 / 32, 33 / 32, 1.0)


# ---------------------------------------------------------------- numpy integer references
def perci_operand(qw, zw, k):
    """m[co, ci, r, s] = (q_w - z_w[co]) * k[co, ci]; qw (Co, Cig, R, S), k (Co, Cig) or flat."""
    qw = np.asarray(qw, np.int64)
    w = qw - np.asarray(zw, np.int64).reshape(-1, 1, 1, 1)
    return w * np.asarray(k, np.int64).reshape(qw.shape[0], qw.shape[1], 1, 1)


def operand_sum(qa, za, m, stride, pad, groups=1):
    """I = sum (q_a - z_a) m over co's group, in int64; a zero-padded tap contributes 0."""
    a = np.asarray(qa, np.int64) - int(za)
    Co, Cig = m.shape[:2]
    Cog = Co // groups
    outs = [conv_i64(a[:, g * Cig:(g + 1) * Cig], m[g * Cog:(g + 1) * Cog], stride, pad)
            for g in range(groups)]
    return np.concatenate(outs, axis=1)


def wide_sum(qa, za, m, stride, pad, alo):
    """The wide kernel's route restated in int64: the digit sums D_h, D_l over the shifted
    activations a_s = q_a - ca (a padded tap holds z_a - ca), I = 128 D_h + D_l + az * T[co]."""
    from shiftedscalequantization_amd import kernels as K
    h, lo = K.wide_digits(m)
    ca = alo + 128
    Dh = conv_i64(np.asarray(qa, np.int64) - ca, h, stride, pad, fill=za - ca)
    Dl = conv_i64(np.asarray(qa, np.int64) - ca, lo, stride, pad, fill=za - ca)
    assert max(np.abs(Dh).max(), np.abs(Dl).max()) < 2 ** 31
    T = m.reshape(m.shape[0], -1).sum(1)
    assert np.abs(T).max() < 2 ** 31
    return 128 * Dh + Dl + (ca - za) * T.reshape(1, -1, 1, 1)


def grid_scale(da, base, L):
    """s[co] = fp32(fp32(delta_a * base[co]) / fp32(L))."""
    s = F32(da) * np.asarray(base, F32)
    assert s.dtype == F32
    return s / F32(L)


def ref_output(I, scale):
    """The contract: fp32(I) * s[co] -- one conversion, one fp32 product."""
    return I.astype(F32) * np.asarray(scale, F32).reshape(1, -1, 1, 1)


def shifted_rows(rng, targets, Co, Ci, drop=None):
    """scale[co, ci] = fp32(delta[co] * fp32(target)) with random delta and a random target per
    element (every row holds each kept target at least once) -> (scale, delta, picked index)."""
    t = np.array(targets, F32)
    keep = [i for i in range(len(t)) if i != drop]
    d = rng.uniform(1e-3, 0.1, Co).astype(F32)
    pick = rng.choice(keep, (Co, Ci))
    for j, i in enumerate(keep):
        pick[:, j] = i
    s = d[:, None] * t[pick]
    assert s.dtype == F32
    return s, d, pick


def predicate(scale, L, base, k, kmax):
    """perci_grid's acceptance predicate, bit for bit."""
    Co, Ci = scale.shape
    k = k.numpy().reshape(Co, Ci)
    b = base.numpy()
    assert base.dtype == torch.float32 and b.shape == (Co,) and np.all(b > 0)
    assert k.dtype == np.int32 and k.min() >= 1 and k.max() <= kmax
    got = b[:, None] * (k.astype(F32) / F32(L))
    assert got.dtype == F32
    np.testing.assert_array_equal(got.view(np.int32), scale.view(np.int32))


# ---------------------------------------------------------------- the per-(co, ci) grid rule
def test_grid_of_shifted_scales():
    from shiftedscalequantization_amd import kernels as K
    rng = np.random.default_rng(0)
    s, d, pick = shifted_rows(rng, SHIFT, 64, 48)
    L, base, k = K.perci_grid(torch.from_numpy(s), 64, 48, 127)
    assert L == 32
    predicate(s, L, base, k, 127)
    np.testing.assert_array_equal(k.numpy().reshape(64, 48), np.array([31, 33, 32])[pick])
    np.testing.assert_array_equal(base.numpy().view(np.int32), d.view(np.int32))
    # any shape is flattened; a device-free torch tensor is all it needs
    assert K.perci_grid(torch.from_numpy(s).reshape(64, 48, 1, 1), 64, 48, 127)[0] == 32


def test_grid_without_the_unshifted_target():
    """No row holds the 1.0 target: L = 32 all the same, k in {31, 33}."""
    from shiftedscalequantization_amd import kernels as K
    rng = np.random.default_rng(1)
    s, d, pick = shifted_rows(rng, SHIFT, 64, 40, drop=2)
    L, base, k = K.perci_grid(torch.from_numpy(s), 64, 40, 127)
    assert L == 32
    predicate(s, L, base, k, 127)
    assert set(k.tolist()) == {31, 33}


def test_grid_halves_and_eighths():
    from shiftedscalequantization_amd import kernels as K
    rng = np.random.default_rng(2)
    s, _, pick = shifted_rows(rng, (1.0, 0.5), 64, 20)
    L, base, k = K.perci_grid(torch.from_numpy(s), 64, 20, 127)
    assert L == 1 and set(k.tolist()) == {1, 2}
    predicate(s, L, base, k, 127)
    s, _, pick = shifted_rows(rng, (7 / 8, 9 / 8, 1.0), 64, 20)
    L, base, k = K.perci_grid(torch.from_numpy(s), 64, 20, 127)
    assert L == 8
    predicate(s, L, base, k, 127)
    np.testing.assert_array_equal(k.numpy().reshape(64, 20), np.array([7, 9, 8])[pick])
    # every i / 8: on a grid of eighths at the latest (k <= 2 L admits L = 4 with k up to 8)
    s, _, _ = shifted_rows(rng, tuple(i / 8 for i in range(1, 9)), 64, 24)
    L, base, k = K.perci_grid(torch.from_numpy(s), 64, 24, 127)
    assert L in (4, 8)
    predicate(s, L, base, k, 127)


def test_grid_takes_the_smallest_l():
    """No smaller L than the one returned satisfies the predicate under the k <= 2 L rule: every
    smaller L is tried here by brute force on one row, all k and the three bases."""
    from shiftedscalequantization_amd import kernels as K
    rng = np.random.default_rng(3)
    s, _, _ = shifted_rows(rng, SHIFT, 64, 12)
    L, base, k = K.perci_grid(torch.from_numpy(s), 64, 12, 127)
    assert L == 32
    fails = 0
    for Ls in range(1, L):
        ok_rows = 0
        for row in s:
            v = np.unique(row)
            hit = False
            for kr in range(1, 2 * Ls + 1):
                b0 = F32(np.float64(v.max()) * Ls / kr)
                for b in (np.nextafter(b0, F32(0)), b0, np.nextafter(b0, F32(np.inf))):
                    kk = np.rint(v.astype(np.float64) / np.float64(b) * Ls)
                    if kk.min() < 1:
                        continue
                    got = F32(b) * (kk.astype(F32) / F32(Ls))
                    hit = hit or np.array_equal(got.view(np.int32), v.view(np.int32))
            ok_rows += hit
        fails += ok_rows < len(s)
    assert fails == L - 1
    # the smallest k at the row's maximum, then the smaller base: an all-equal row takes k = 1
    s[5] = s[5, 0]
    L, base, k = K.perci_grid(torch.from_numpy(s), 64, 12, 127)
    assert L == 32 and set(k.numpy().reshape(64, 12)[5].tolist()) == {1}
    predicate(s, L, base, k, 127)


def test_grid_refusals():
    from shiftedscalequantization_amd import kernels as K
    rng = np.random.default_rng(4)
    s, _, _ = shifted_rows(rng, SHIFT, 16, 12)
    for bad in (0.0, float("nan"), float("inf"), -0.01):
        t = s.copy()
        t[3, 4] = bad
        assert K.perci_grid(torch.from_numpy(t), 16, 12, 127) is None
    t = s.copy()
    t[3, 4] = np.nextafter(t[3, 4], F32(1))         # one ulp off its grid point
    t[3, 5] = t[3, 4] * F32(1.0001)                 # and a value on no grid with its row
    assert K.perci_grid(torch.from_numpy(t), 16, 12, 127) is None
    assert K.perci_grid(torch.from_numpy(s), 16, 11, 127) is None    # size mismatch
    # the wide limits: sixteenths of 1 / 1024 steps need L = 1024
    t = rng.uniform(1e-3, 0.1, (8, 1)).astype(F32) * (F32(1) + np.arange(6, dtype=F32) / F32(1024))
    assert K.perci_grid(torch.from_numpy(t), 8, 6, 127) is None
    L, base, k = K.perci_grid(torch.from_numpy(t), 8, 6, K.QWIDE_MAX)
    assert L == 1024 and k.max() <= K.QWIDE_MAX
    predicate(t, L, base, k, K.QWIDE_MAX)


def test_all_k_equal_l_is_plain():
    from shiftedscalequantization_amd import kernels as K
    d = np.random.default_rng(5).uniform(1e-3, 0.1, 24).astype(F32)
    s = np.repeat(d[:, None], 10, axis=1)
    g = K.perci_grid(torch.from_numpy(s), 24, 10, 127)
    assert g[0] == 1 and K.perci_plain(g)
    np.testing.assert_array_equal(g[1].numpy().view(np.int32), d.view(np.int32))
    s2, _, _ = shifted_rows(np.random.default_rng(6), SHIFT, 24, 10)
    assert not K.perci_plain(K.perci_grid(torch.from_numpy(s2), 24, 10, 127))
    assert not K.perci_plain(None)


def test_planning_time_of_a_resnet18_layer():
    """The largest per-(co, ci) layer of ResNet-18 (512 x 512) plans in well under a second."""
    import time
    from shiftedscalequantization_amd import kernels as K
    s, _, _ = shifted_rows(np.random.default_rng(7), SHIFT, 512, 512)
    t0 = time.perf_counter()
    assert K.perci_grid(torch.from_numpy(s), 512, 512, 127)[0] == 32
    assert time.perf_counter() - t0 < 5.0


# ---------------------------------------------------------------- the column grid's new limits
def test_colscale_grid_defaults_unchanged_and_wide_limits():
    from shiftedscalequantization_amd import kernels as K
    p = inspect.signature(K.colscale_grid).parameters
    assert p["max_l"].default == 127 and p["kmax"].default == 127
    for level in (1, 2, 3, 4, 8, 32, 127):
        rng = np.random.default_rng(level)
        k = rng.integers(1, level + 1, 300)
        k[0], k[-1] = 1, level
        c = torch.from_numpy(k.astype(F32) / F32(level))
        L, kk = K.colscale_grid(c)
        L2, kk2 = K.colscale_grid(c, 127, 127)
        assert L == L2 == level and torch.equal(kk, kk2) and kk.dtype == torch.int32
        np.testing.assert_array_equal(kk.numpy(), k)
    assert K.colscale_grid(torch.tensor([1.0, 1.0 / 128.0])) is None
    assert K.colscale_grid(torch.tensor([1.0, 1.0 / 127.0]))[0] == 127
    rng = np.random.default_rng(1024)
    k = rng.integers(1, 1025, 300)
    k[0], k[-1] = 1, 1024
    c = torch.from_numpy(k.astype(F32) / F32(1024))
    assert K.colscale_grid(c) is None
    L, kk = K.colscale_grid(c, max_l=1024, kmax=16319)
    assert L == 1024
    np.testing.assert_array_equal(kk.numpy(), k)
    assert K.colscale_grid(c, max_l=1024, kmax=1023) is None
    assert K.colscale_grid(torch.tensor([1.0, 1.0 / 1025.0]), 1024, 16319) is None


# ---------------------------------------------------------------- the digit split
def test_digits_recombine_over_the_whole_range():
    from shiftedscalequantization_amd import kernels as K
    assert K.QWIDE_MAX == 16319 == 128 * 127 + 63
    m = np.arange(-16319, 16320)
    h, lo = K.wide_digits(m)
    np.testing.assert_array_equal(128 * h + lo, m)
    assert lo.min() == -64 and lo.max() == 63 and h.min() == -127 and h.max() == 127
    np.testing.assert_array_equal(lo, ((m + 64) % 128) - 64)
    # one past the range leaves int8
    assert K.wide_digits(np.array([16320]))[0][0] == 128


def test_wide_sum_reference_equals_the_plain_sum():
    """128 D_h + D_l + az * T over the shifted activations is sum (q_a - z_a) m, padding
    included, with operands over the whole wide range."""
    rng = np.random.default_rng(8)
    qa, za, alo = rng.integers(0, 256, (2, 5, 6, 4)), 77, 0
    m = rng.integers(-16319, 16320, (7, 5, 3, 3))
    m[0], m[1] = 16319, -16319
    np.testing.assert_array_equal(wide_sum(qa, za, m, 1, 1, alo), operand_sum(qa, za, m, 1, 1))
    np.testing.assert_array_equal(wide_sum(qa, za, m, 2, 1, alo), operand_sum(qa, za, m, 2, 1))
    qs, zs, slo = rng.integers(-128, 128, (2, 5, 6, 4)), -3, -128
    np.testing.assert_array_equal(wide_sum(qs, zs, m, 1, 1, slo), operand_sum(qs, zs, m, 1, 1))


# ---------------------------------------------------------------- ABI
def test_new_symbols_declared_exported_and_bound():
    from shiftedscalequantization_amd import _capi
    src = open(os.path.join(ROOT, "include", "ssq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _capi.load()
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % s, src)
        assert m and hasattr(lib, s) and s in _capi.SIGNATURES, s
        assert len(_capi.SIGNATURES[s][1]) == m.group(1).count(",") + 1, s
    for form in ("fwd", "codes_fwd", "codes_res_fwd"):
        assert _capi.SIGNATURES[f"ssq_qconv_i8_wide_{form}"] == _capi.SIGNATURES[f"ssq_qconv_i8_{form}"]
    # as many prototypes as exports
    protos = set(re.findall(r"\b(ssq_\w+)\s*\(", src))
    assert protos == set(_capi.SIGNATURES)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(s in doc for s in NEW)


def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


def test_argument_errors_without_gpu():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    f = _fake
    lib.ssq_qweight_prepared_bytes_wide.restype = C.c_size_t
    narrow = lib.ssq_qweight_prepared_bytes(72, 70, 3, 3)
    wide = lib.ssq_qweight_prepared_bytes_wide(72, 70, 3, 3)
    Cop, Kp = 128, -(-9 * 80 // 64) * 64
    assert narrow == Cop * Kp + Kp + 8 * Cop and wide == narrow + Cop * Kp
    assert lib.ssq_qweight_prepared_bytes_wide(0, 70, 3, 3) == 0
    prep = lib.ssq_qweight_prepare_perci
    assert prep(f(), f(), None, 8, 8, 1, 1, 4, 0, f(), f(), None) == -1
    assert b"null" in lib.ssq_last_error()
    assert prep(f(), f(), f(), 8, 65537, 1, 1, 4, 0, f(), f(), None) == -1
    assert b"65536" in lib.ssq_last_error()
    wprep = lib.ssq_qweight_prepare_wide
    assert wprep(f(), f(), None, 1, 8, 8, 1, 1, 4, 0, f(), f(), None) == -1
    assert b"null" in lib.ssq_last_error()
    assert wprep(f(), f(), f(), 0, 8, 8, 1, 1, 9, 0, f(), f(), None) == -1
    gprep = lib.ssq_qweight_prepare_grouped_perci
    assert gprep(f(), f(), None, 8, 4, 3, 3, 2, 4, 0, f(), f(), None) == -1
    assert b"null" in lib.ssq_last_error()
    assert gprep(f(), f(), f(), 8, 1, 3, 3, 8, 4, 0, f(), f(), None) == -1      # depthwise
    assert b"depthwise" in lib.ssq_last_error()
    conv = lib.ssq_qconv_i8_wide_fwd
    args = lambda **kw: [kw.get(n, v) for n, v in (("Nb", 1), ("Ci", 8), ("H", 4), ("W", 4), ("Co", 8),
                                                   ("R", 1), ("S", 1), ("stride", 1), ("pad", 0),
                                                   ("groups", 1), ("zp", 0.0), ("qmin", 0),
                                                   ("qmax", 255))]
    assert conv(None, f(), f(), *args(), f(), None) == -1 and b"null" in lib.ssq_last_error()
    assert conv(f(), f(), f(), *args(groups=2), f(), None) == -1 and b"groups" in lib.ssq_last_error()
    assert conv(f(), f(), f(), *args(zp=0.5), f(), None) == -1 and b"zero point" in lib.ssq_last_error()
    assert conv(f(), f(), f(), *args(Ci=65537), f(), None) == -1 and b"65536" in lib.ssq_last_error()


def test_wrapper_routes_and_refuses_a_wide_blob(monkeypatch):
    """Without a device: the wide blob's entry points, and the reasons it is refused for split-K
    (K23's split form), the grouped kernels (K26) and the pooled-operand fc (K30)."""
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    wide = K.QPrepared(None, (4, 4, 1, 1), None, centred=True, wide=True)
    assert wide.wide and not K.QPrepared(None, (4, 4, 1, 1), None, centred=True).wide
    for centred in (True, False):
        monkeypatch.setattr(K, "QCONV_CENTRED", centred)
        for form in ("fwd", "codes_fwd", "codes_res_fwd"):
            assert K._qconv_fn(wide, 1, form) == f"ssq_qconv_i8_wide_{form}"
    with pytest.raises(SSQError, match="K26"):
        K._qconv_fn(K.QPrepared(None, (4, 2, 3, 3), None, groups=2, centred=True, wide=True), 2, "fwd")
    with pytest.raises(SSQError, match="split-K"):
        K._qconv_split("qconv", wide, 1, "fwd", 2, None, torch.zeros(1, 4, 4, 16, dtype=torch.int8), 1, 0)
    assert K.QCONV_WIDE in ("auto", "1")


# ---------------------------------------------------------------- flags
def test_cli_flags():
    from shiftedscalequantization_amd.cli import parse_args
    a = parse_args([])
    assert not a.int_infer_per_ci and not a.int_infer_wide and not a.int_infer
    a = parse_args(["--int_infer_per_ci"])
    assert a.int_infer_per_ci and a.int_infer and not a.int_infer_wide and not a.int_infer_colscale
    a = parse_args(["--int_infer_wide"])
    assert a.int_infer_wide and a.int_infer and not a.int_infer_per_ci
    a = parse_args(["--int_infer_per_ci", "--int_infer_wide", "--int_infer_carry_head"])
    assert a.int_infer_per_ci and a.int_infer_wide and a.int_infer_carry_stem


def test_planner_defaults_and_todays_reasons():
    """The new keywords default to off, and the two reasons a layer meets with them off are
    spelled as before (the planner itself runs in test_qinfer_perci_model_gpu.py)."""
    from shiftedscalequantization_amd.quant import enable_integer_inference, integer
    p = inspect.signature(enable_integer_inference).parameters
    assert p["per_ci"].default is False and p["wide"].default is False
    src = inspect.getsource(integer.enable_integer_inference)
    assert 'f"weight scale is per (co, ci) ({f[\'kind\']})"' in src
    assert ('"scaled weight (q - z) * k leaves int8 (|m| > 127), or a zero point "\n'
            '                            "is not an integer code"') in src
