"""The cases of tests/shift_cases.py, checked with the oracle alone (no GPU): every case
meets the caps on what its comparisons leave out, its hard-rounding form holds exact clamp
hits, the g_p the alpha bound is scaled by is the oracle's own, and the oracle's distance
between an fp32 and an fp64 softmax stays under 1 * 2^-23 * G -- a sixteenth of the bound the
kernels are held to, so that bound does not rest on the oracle's noise."""
import numpy as np
import pytest

from oracle import ssq_ref as R
import shift_cases as C

F32 = np.float32
CASE_S = [pytest.param(shape, bits, S, id=f"{C.id_of(shape, bits)}-S{S}")
          for shape, bits in C.CASES for S in C.shift_counts(bits)]


@pytest.mark.parametrize("shape,bits,S", CASE_S)
def test_case_meets_caps_by_oracle_alone(shape, bits, S):
    """Exclusion caps (fewer than 16 channels: none; else max(1, 1 %) of the channels; 0.1 %
    of the elements of an elementwise comparison) and >= 1 exact clamp hit at hard rounding."""
    counts = C.check_case(shape, S, bits)
    assert counts["hr1"][1] >= 1


@pytest.mark.parametrize("shape,bits,S", CASE_S)
def test_gp_is_the_oracles(shape, bits, S):
    """shift_cases re-forms g_p (the alpha bound's scale); the oracle's chain applied to it
    gives R.adashift_bwd's galpha bit for bit, so it is the g_p the oracle used."""
    for hard_r in (0, 1):
        r = C.adashift_ref(shape, S, bits, hard_r)
        np.testing.assert_array_equal(R._softmax_clamp_bwd(r.case.alpha, r.g_p), r.galpha)
        assert r.g_p.shape == r.case.alpha.shape and r.g_p.dtype == np.float64


def _chain(s32, s64, g_p):
    u = s32 * R.ZMG + R.GAMMA
    g_s = np.where((u >= 0) & (u <= 1), g_p, 0.0) * float(R.ZMG)
    return s64 * (g_s - (g_s * s64).sum(axis=-1, keepdims=True))


@pytest.mark.parametrize("S", [2, 3, 4, 8])
@pytest.mark.parametrize("shape", [(143, 9, 3, 3), (200, 37, 3, 3), (257, 300, 1, 1), (64, 300)],
                         ids=C.id_of)
def test_oracle_softmax_noise_under_one_ulp(shape, S):
    """The oracle rounds an fp64 softmax to fp32.  Against a softmax computed in fp32
    throughout (numpy's exp and divide) and against one kept in fp64, its galpha moves by at
    most 1 * 2^-23 * G on the rows kept (measured 0.3)."""
    for hard_r in (0, 1):
        r = C.adashift_ref(shape, S, 2, hard_r)
        a = r.case.alpha
        e32 = np.exp(a - a.max(axis=-1, keepdims=True))
        s32 = (e32 / e32.sum(axis=-1, keepdims=True, dtype=F32)).astype(F32)
        assert s32.dtype == F32
        e64 = np.exp((a - a.max(axis=-1, keepdims=True)).astype(np.float64))
        s64 = e64 / e64.sum(axis=-1, keepdims=True)
        G = C.alpha_scale(r.g_p)
        for other in (_chain(s32, s32.astype(np.float64), r.g_p), _chain(R.softmax(a), s64, r.g_p)):
            err = np.abs(other - r.galpha).max(axis=-1)
            err = np.where(r.rows_out, 0.0, err)
            assert np.all(err <= 2.0 ** -23 * G), float((err / np.maximum(G, 1e-300)).max() * 2 ** 23)


def test_cases_are_fixed_and_read_only():
    a = C.make_case((8, 6, 3, 3), 3, 2)
    C.make_case.cache_clear()
    b = C.make_case((8, 6, 3, 3), 3, 2)
    for k in ("w", "delta", "zp", "alpha", "beta", "gy"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
        assert getattr(a, k).dtype == F32 and not getattr(a, k).flags.writeable
    assert a.alpha.shape == (6, 3) and C.make_case((6, 1, 3, 3), 3, 2).alpha.shape == (1, 3)
    assert C.make_case((10, 12), 5, 2).alpha.shape == (10, 12, 5)
    assert a.shifts == [31 / 32, 33 / 32, 1.0]


def test_lhs_and_adaround_multi_cases():
    """The lhs cases' alpha rows and the 11 adaround_multi weights: sizes around the
    512-element tile, more than 8 segments, exclusions within the elementwise cap."""
    sizes = [int(np.prod(s)) for s, _, _, _ in C.ADAROUND_MULTI]
    assert len(sizes) == 11 and {54, 512, 513, 1023, 1025, 2047, 2049, 4095, 4097} <= set(sizes)
    assert any(len(s) == 2 for s, _, _, _ in C.ADAROUND_MULTI)
    for shape, bits, per_ci, scale in C.ADAROUND_MULTI:
        r = C.adaround_ref(shape, bits, per_ci, scale)
        C.check_caps(r.case, elems_out=r.out)
        assert r.delta.size == (shape[0] * shape[1] if per_ci else shape[0])
    for shape in C.FIVE_SHAPES:
        for S in C.LHS_COUNTS:
            r = C.lhs_ref(shape, S, 2)
            C.check_caps(r.case, rows_out=r.rows_out)
            np.testing.assert_array_equal(R._softmax_clamp_bwd(r.case.alpha, r.g_p), r.galpha)
