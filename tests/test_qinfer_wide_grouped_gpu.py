"""The two-digit weight operand on the grouped and depthwise kernels
(ssq_qweight_prepare_grouped_wide, K26's WIDE instantiations, K25 on its int32 blob with
|m| <= 16319): y.view(int32) must EQUAL the host int64 reference fp32(I) * s[co],
I = sum (q_a - z_a) m over co's group, s[co] = fp32(fp32(delta_a * base[co]) / fp32(L)).

Grouped shapes: g = 3 / Cig = 24 / Cog = 8 (windows off the 16-byte grid, one fragment per tile,
8-byte code stores) as 3x3 stride 1 and 2 and 1x1, and g = 2 / Cig = 16 / Cog = 72 (two channel
tiles, the second with one fragment), batch 2 on a 5 x 7 plane (M = 70: a pixel tile and a part
of one); W4 / L32 and W8 / L32 per-(co, ci), W4 / L1024 column-scaled; A4 and A8, symmetric or not.
Then the accumulator extremes (K = 576, every m = +-16319, |I| > 2^31), bit identity with K26 on
the centred int8 blob (SSQ_QCONV_WIDE=1), the code-emitting form against the uncarried route
(padding, ownership of the code tile, the NaN count), the depthwise form (C = 20, factors up to
16319, |I| > 2^24 where the conversion rounds) and the prepare's count for both kinds."""
import functools
import types
import zlib

import numpy as np
import pytest
import torch

from test_qinfer_carry_gpu import pick_quantizer
from test_qinfer_colscale_gpu import encode_colscale
from test_qinfer_colscale_host import centred_operand
from test_qinfer_host import qrange
from test_qinfer_perci_gpu import dev, draw_perci_weight, encode_perci, host
from test_qinfer_perci_host import grid_scale, operand_sum, perci_operand, predicate, ref_output

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


# (N, C, H, W, Co, R, stride, pad, G)
SHAPES = {
    "g3_3x3_s1": (2, 72, 5, 7, 24, 3, 1, 1, 3),
    "g3_3x3_s2": (2, 72, 5, 7, 24, 3, 2, 1, 3),
    "g3_1x1": (2, 72, 5, 7, 24, 1, 1, 0, 3),
    "g2_cog72": (2, 32, 5, 7, 144, 3, 1, 1, 2),
}
WEIGHTS = ["perci_w4_l32", "perci_w8_l32", "col_w4_l1024"]
ACTS = [(4, True), (8, False), (4, False), (8, True)]           # (n_bits_a, sym)
# every (shape, weight form); the activation forms rotate so that each shape and each weight form
# meets A4 and A8, symmetric and not
CASES = [(n, w, ACTS[(i + j) % len(ACTS)]) for i, n in enumerate(SHAPES) for j, w in enumerate(WEIGHTS)]
CASES += [("g3_3x3_s1", "perci_w4_l32", a) for a in ACTS[1:]]


def draw_weight(K, rng, ws, wform):
    """(wb, qw, zw, packed, m, L, base[co], prepare keywords) of one grouped weight form; ws is the
    weight's own (Co, Cig, R, S), the grid found from the stored floats."""
    Co, Cig = ws[:2]
    if wform.startswith("perci"):
        wb = 4 if "w4" in wform else 8
        qw, zw, wscale = draw_perci_weight(rng, ws, wb)
        L, base, k = K.perci_grid(torch.from_numpy(wscale), Co, Cig, K.QWIDE_MAX)
        assert L == 32
        predicate(wscale, L, base, k, K.QWIDE_MAX)
        _, packed = encode_perci(K, qw, zw, wscale, wb)
        return wb, qw, zw, packed, perci_operand(qw, zw, k.numpy()), L, base.numpy(), dict(kfac=k)
    wb, whi = 4, 15
    qw = rng.integers(0, whi + 1, ws)
    zw = rng.integers(0, whi + 1, Co)
    zw[0], zw[-1] = 0, whi
    k = rng.integers(1, 1025, int(np.prod(ws[1:])))
    k[0], k[-1] = 1, 1024
    d1 = rng.uniform(1e-3, 2e-2, Co).astype(F32)
    _, packed = encode_colscale(K, qw, zw, d1, k, 1024, wb)
    L, kk = K.colscale_grid(torch.from_numpy(k.astype(F32) / F32(1024)), K.QWIDE_MAX_L, K.QWIDE_MAX)
    assert L == 1024 and np.array_equal(kk.numpy(), k)
    return wb, qw, zw, packed, centred_operand(qw, zw, k), L, d1, dict(kcol=kk)


@functools.lru_cache(maxsize=None)
def layer(name, wform, aform):
    """One wide grouped layer: the prepared blob, the encoded input and the host reference."""
    from shiftedscalequantization_amd import kernels as K
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(repr((name, wform, aform)).encode()))
    ab, asym = aform
    alo, ahi = qrange(ab, asym)
    qa = rng.integers(alo, ahi + 1, (N, Cc, H, W))
    za = int(rng.integers(alo, ahi + 1))
    wb, qw, zw, packed, m, L, base, kw = draw_weight(K, rng, (Co, Cc // G, R, R), wform)
    assert 127 < np.abs(m).max() <= K.QWIDE_MAX
    prep = K.qweight_prepare_scaled(packed, qw.shape, dev(zw), wb, 0, groups=G, wide=True,
                                    wide_all=True, **kw)
    assert prep.wide and prep.wide_all and prep.centred and prep.groups == G
    assert int(prep.bad.item()) == 0 and K.qconv_kind(prep) == "grouped"
    da = F32(rng.uniform(0.01, 0.2))
    codes, nb = K.act_encode(dev((qa - za).astype(F32) * da), float(da), float(za), ab, asym)
    assert int(nb.item()) == 0
    scale = grid_scale(da, base, L)
    I = operand_sum(qa, za, m, stride, pad, G)
    return types.SimpleNamespace(prep=prep, codes=codes, scale=scale, ref=ref_output(I, scale), G=G,
                                 kw=dict(groups=G, act_zp=float(za), act_bits=ab, act_sym=asym),
                                 geo=(stride, pad), Co=Co)


def test_cases_cover_the_issue():
    for n in SHAPES:
        assert {w for s, w, _ in CASES if s == n} == set(WEIGHTS)
    for w in WEIGHTS:
        forms = {a for _, ww, a in CASES if ww == w}
        assert {a[0] for a in forms} == {4, 8} and {a[1] for a in forms} == {False, True}
    assert {a for s, w, a in CASES if (s, w) == ("g3_3x3_s1", "perci_w4_l32")} == set(ACTS)


@pytest.mark.parametrize("name,wform,aform", CASES)
def test_grouped_wide_bit_exact(K, name, wform, aform):
    Ly = layer(name, wform, aform)
    stride, pad = Ly.geo
    assert K._qconv_fn(Ly.prep, Ly.G, "fwd") == "ssq_qconv_i8_grouped_wide_fwd"
    y = K.qconv(Ly.codes, Ly.prep, dev(Ly.scale), stride, pad, **Ly.kw)
    assert Ly.ref.any()
    np.testing.assert_array_equal(host(y).view(np.int32), Ly.ref.view(np.int32))


# ---------------------------------------------------------------- the code-emitting form
def epilogue_vectors(Co, seed=7):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 0.05, Co).astype(F32), rng.uniform(0.5, 1.5, Co).astype(F32),
            rng.normal(0, 0.05, Co).astype(F32))


def emitted_and_uncarried(K, Ly, prep=None, gamma=None):
    """(the code-emitting kernel's bytes, the uncarried route's: the fp32 form -> the K13 epilogue
    -> act_encode, the kernel's `bad`)."""
    prep = Ly.prep if prep is None else prep
    stride, pad = Ly.geo
    bias, g0, phi = epilogue_vectors(Ly.Co)
    gamma = g0 if gamma is None else gamma
    d, z = pick_quantizer(np.maximum(Ly.ref, 0), 4, False)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    fused = K.qconv_codes(Ly.codes, prep, dev(Ly.scale), stride, pad, bias=dev(bias), gamma=dev(gamma),
                          phi=dev(phi), relu=1, out_delta=float(d), out_zp=float(z), out_bits=4,
                          bad=bad, **Ly.kw)
    y = K.qconv(Ly.codes, prep, dev(Ly.scale), stride, pad, **Ly.kw)
    q = types.SimpleNamespace(delta=dev(np.array([d], F32)), zero_point=dev(np.array([z], F32)),
                              n_bits=4, sym=False)
    with torch.no_grad():
        yq = K.epilogue(y, dev(bias), dev(gamma), dev(phi), None, 1, q)
    plain, _ = K.act_encode(yq, float(d), float(z), 4, False)
    return host(fused), host(plain), int(bad.item())


@pytest.mark.parametrize("name,wform,aform", CASES[:len(SHAPES) * len(WEIGHTS)])
def test_grouped_wide_codes_equal_the_uncarried_route(K, name, wform, aform):
    Ly = layer(name, wform, aform)
    assert K._qconv_fn(Ly.prep, Ly.G, "codes_fwd") == "ssq_qconv_i8_grouped_wide_codes_fwd"
    got, want, bad = emitted_and_uncarried(K, Ly)
    real = got[..., :Ly.Co].astype(np.int64) + 128
    assert (real == 0).any() and (real == 15).any() and ((real > 0) & (real < 15)).any()
    assert bad == 0 and not got[..., Ly.Co:].any()          # padded channels are 0
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", ["g3_3x3_s1", "g2_cog72"])
def test_code_tiles_write_their_own_bytes_only(K, name):
    """The entry point on a caller's buffer filled with a sentinel, with guard bytes on both sides:
    every byte of the output is written (a tile owns [c0, c1) of each pixel: 8-byte units for
    Cog = 8, the layer's padding included), the bytes equal the wrapper's, so no tile wrote over
    another's, and no guard byte changes."""
    from shiftedscalequantization_amd import _capi as A
    Ly = layer(name, "perci_w4_l32", (4, True))
    stride, pad = Ly.geo
    want, _, _ = emitted_and_uncarried(K, Ly)
    bias, gamma, phi = (dev(v) for v in epilogue_vectors(Ly.Co))
    d, z = pick_quantizer(np.maximum(Ly.ref, 0), 4, False)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    args, keep, _ = K._qconv_args("qconv_codes", Ly.codes, Ly.prep, dev(Ly.scale), stride, pad, Ly.G,
                                  Ly.kw["act_zp"], Ly.kw["act_bits"], Ly.kw["act_sym"], None, bad)
    guard, sentinel = 256, 0x5A
    buf = torch.full((want.size + 2 * guard,), sentinel, dtype=torch.int8, device="cuda")
    out = buf[guard:guard + want.size]
    A.call("ssq_qconv_i8_grouped_wide_codes_fwd", *args, K._vp(bias), K._vp(gamma), K._vp(phi), 1,
           float(d), float(z), 0, 15, K._vp(out), K._vp(bad), A.stream_of(buf))
    got = host(buf)
    assert (got[:guard] == sentinel).all() and (got[guard + want.size:] == sentinel).all()
    np.testing.assert_array_equal(got[guard:guard + want.size].reshape(want.shape), want)
    assert int(bad.item()) == 0


def test_nan_gamma_channels_are_qmin_and_counted_exactly(K):
    """gamma^z = NaN on two channels of different groups: every pixel of those channels is stored as
    qmin and counted once; every other byte is the uncarried route's."""
    Ly = layer("g3_3x3_s1", "perci_w4_l32", (4, True))
    clean, _, bad0 = emitted_and_uncarried(K, Ly)
    _, gamma, _ = epilogue_vectors(Ly.Co)
    gamma = gamma.copy()
    gamma[[3, 17]] = np.nan
    got, _, bad = emitted_and_uncarried(K, Ly, gamma=gamma)
    M = got.shape[0] * got.shape[1] * got.shape[2]
    assert bad0 == 0 and bad == 2 * M
    assert (got[..., [3, 17]] == -128).all()                # qmin = 0 stored as 0 - 128
    keep = np.ones(got.shape[-1], bool)
    keep[[3, 17]] = False
    np.testing.assert_array_equal(got[..., keep], clean[..., keep])


# ---------------------------------------------------------------- accumulator extremes
@pytest.mark.parametrize("at", ["qmax", "qmin"])
def test_accumulator_extremes(K, at):
    """g = 2, Cig = 64, 3x3 on a 3x3 plane (K = 576): every m = +-16319 ((q - z) = +-1, k = 16319),
    every activation at qmax with z_a = qmin, or at qmin with z_a = qmax: |I| = 576 * 255 * 16319
    passes 2^31 in the centre and the conversion rounds; one channel all +, one all -, one all +
    but a single tap, the rest mixed."""
    N, Cig, G, Co = 1, 64, 2, 16
    rng = np.random.default_rng(5)
    sign = rng.integers(0, 2, (Co, Cig, 3, 3)) * 2 - 1
    sign[0], sign[1], sign[2], sign[8], sign[9] = 1, -1, 1, 1, -1
    sign[2, 0, 1, 1] = -1
    zw = np.ones(Co, np.int64)
    qw = 1 + sign                                               # W2 codes 0 / 2 around z = 1
    k = np.full(Cig * 9, 16319)
    m = centred_operand(qw, zw, k)
    assert set(np.unique(m)) == {-16319, 16319}
    shape = (N, Cig * G, 3, 3)
    qa, za = (np.full(shape, 255), 0) if at == "qmax" else (np.zeros(shape, np.int64), 255)
    d1 = np.linspace(0.5, 1.5, Co).astype(F32)
    _, packed = encode_colscale(K, qw, zw, d1, k, 1024, 2)
    prep = K.qweight_prepare(packed, qw.shape, dev(zw), 2, 0, groups=G, kcol=torch.from_numpy(k),
                             wide=True, wide_all=True)
    assert prep.wide and prep.wide_all and int(prep.bad.item()) == 0
    scale = grid_scale(F32(1.0), d1, 1024)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = K.qconv(dev((qa - za).astype(F32)), prep, dev(scale), 1, 1, groups=G, act_zp=float(za),
                act_bits=8, act_delta=1.0, bad=bad)
    I = operand_sum(qa, za, m, 1, 1, G)
    assert np.abs(I).max() == 576 * 255 * 16319 > 2 ** 31 and I.min() == -I.max()
    assert np.any(I.astype(F32).astype(np.int64) != I)
    assert int(bad.item()) == 0
    np.testing.assert_array_equal(host(y).view(np.int32), ref_output(I, scale).view(np.int32))


# ---------------------------------------------------------------- one weight, two operands
@pytest.mark.parametrize("form", ["fp32", "codes"])
def test_wide_knob_is_bit_identical_to_k26_on_the_centred_int8_blob(K, monkeypatch, form):
    """A W2 / L32 per-(co, ci) grouped weight (|m| <= 99) under SSQ_QCONV_WIDE=1 takes the wide
    blob and gives K26's bytes on the centred int8 blob; under auto it stays int8."""
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES["g3_3x3_s1"]
    rng = np.random.default_rng(41)
    qw, zw, wscale = draw_perci_weight(rng, (Co, Cc // G, R, R), 2)
    L, base, k = K.perci_grid(torch.from_numpy(wscale), Co, Cc // G, 127)
    m = perci_operand(qw, zw, k.numpy())
    assert 64 <= np.abs(m).max() <= 127                         # both digits in use
    _, packed = encode_perci(K, qw, zw, wscale, 2)
    preps = {}
    for knob in ("auto", "1"):
        monkeypatch.setattr(K, "QCONV_WIDE", knob)
        preps[knob] = K.qweight_prepare_scaled(packed, qw.shape, dev(zw), 2, 0, groups=G, kfac=k,
                                               wide=True, wide_all=True)
        assert int(preps[knob].bad.item()) == 0 and preps[knob].centred
    assert not preps["auto"].wide and not preps["auto"].wide_all
    assert preps["1"].wide and preps["1"].wide_all
    assert K._qconv_fn(preps["auto"], G, "fwd") == "ssq_qconv_i8_grouped_fwd"
    assert preps["1"].blob.numel() > preps["auto"].blob.numel()
    qa, za = rng.integers(0, 16, (N, Cc, H, W)), 6
    da = F32(0.125)
    codes, _ = K.act_encode(dev((qa - za).astype(F32) * da), float(da), float(za), 4, False)
    scale = grid_scale(da, base.numpy(), L)
    ref = ref_output(operand_sum(qa, za, m, stride, pad, G), scale)
    Ly = types.SimpleNamespace(codes=codes, scale=scale, ref=ref, geo=(stride, pad), Co=Co, G=G,
                               kw=dict(groups=G, act_zp=float(za), act_bits=4, act_sym=False))
    if form == "fp32":
        ys = [host(K.qconv(codes, preps[kn], dev(scale), stride, pad, **Ly.kw)) for kn in ("auto", "1")]
        np.testing.assert_array_equal(ys[0].view(np.int32), ref.view(np.int32))
        np.testing.assert_array_equal(ys[1].view(np.int32), ys[0].view(np.int32))
        return
    narrow, _, _ = emitted_and_uncarried(K, Ly, preps["auto"])
    wide, _, _ = emitted_and_uncarried(K, Ly, preps["1"])
    assert narrow.any()
    np.testing.assert_array_equal(wide, narrow)


# ---------------------------------------------------------------- depthwise
DEPTHWISE = {"dw3_s1": (3, 1, 1), "dw3_s2": (3, 2, 1), "dw5_s1": (5, 1, 2), "dw5_s2": (5, 2, 2)}


def draw_depthwise(K, rng, C, R):
    """W2 codes one step around their zero points against column factors up to 16319."""
    zw = rng.integers(1, 3, C)
    qw = zw.reshape(-1, 1, 1, 1) + rng.integers(-1, 2, (C, 1, R, R))
    k = rng.integers(1, 16320, R * R)
    k[0], k[-1] = 16319, 1
    d1 = rng.uniform(1e-3, 2e-2, C).astype(F32)
    _, packed = encode_colscale(K, qw, zw, d1, k, 1024, 2)
    return qw, zw, k, d1, packed


@pytest.mark.parametrize("name", list(DEPTHWISE))
@pytest.mark.parametrize("extreme", [False, True])
def test_depthwise_wide_bit_exact(K, name, extreme):
    """C = 20 (a chunk and a part of one), batch 2 on a 7 x 9 plane.  `extreme`: every activation
    at qmax against z_a = 0 and the first channels all +, all -: |I| passes 2^24 and fp32(I) rounds
    (stated on the host reference); the int8 blob does not hold the weight."""
    R, stride, pad = DEPTHWISE[name]
    C, N, H, W = 20, 2, 7, 9
    rng = np.random.default_rng(zlib.crc32(repr((name, extreme)).encode()))
    qw, zw, k, d1, packed = draw_depthwise(K, rng, C, R)
    if extreme:
        qw[0], qw[1] = zw[0] + 1, zw[1] - 1
        _, packed = encode_colscale(K, qw, zw, d1, k, 1024, 2)
    m = centred_operand(qw, zw, k)
    assert np.abs(m).max() == 16319
    kk = torch.from_numpy(k)
    assert K.qweight_prepare_scaled(packed, qw.shape, dev(zw), 2, 0, groups=C, kcol=kk, wide=True) is None
    prep = K.qweight_prepare_scaled(packed, qw.shape, dev(zw), 2, 0, groups=C, kcol=kk, wide=True,
                                    wide_all=True)
    assert prep.wide and prep.wide_all and int(prep.bad.item()) == 0
    assert K.qconv_kind(prep) == "depthwise"
    assert K._qconv_fn(prep, C, "fwd") == "ssq_qconv_i8_grouped_wide_fwd"
    qa, za = (np.full((N, C, H, W), 255), 0) if extreme else (rng.integers(0, 256, (N, C, H, W)), 131)
    scale = grid_scale(F32(1.0), d1, 1024)
    I = operand_sum(qa, za, m, stride, pad, C)
    if extreme:
        assert 2 ** 24 < np.abs(I).max() < 2 ** 31
        assert np.any(I.astype(F32).astype(np.int64) != I)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(groups=C, act_zp=float(za), act_bits=8)
    y = K.qconv(dev((qa - za).astype(F32)), prep, dev(scale), stride, pad, act_delta=1.0, bad=bad, **kw)
    ref = ref_output(I, scale)
    assert int(bad.item()) == 0 and ref.any()
    np.testing.assert_array_equal(host(y).view(np.int32), ref.view(np.int32))
    # the code-emitting form against the uncarried route
    codes, _ = K.act_encode(dev((qa - za).astype(F32)), 1.0, float(za), 8, False)
    Ly = types.SimpleNamespace(prep=prep, codes=codes, scale=scale, ref=ref, geo=(stride, pad), Co=C,
                               G=C, kw=dict(act_sym=False, **kw))
    got, want, nb = emitted_and_uncarried(K, Ly)
    assert nb == 0 and got[..., :C].any() and not got[..., C:].any()
    np.testing.assert_array_equal(got, want)


def test_depthwise_has_no_per_ci_form(K):
    from shiftedscalequantization_amd._capi import SSQError
    packed = torch.zeros(256, dtype=torch.uint8, device="cuda")
    with pytest.raises(SSQError, match="depthwise"):
        K.qweight_prepare(packed, (20, 1, 3, 3), torch.zeros(20, device="cuda"), 4, 0, groups=20,
                          kfac=torch.full((20,), 200, dtype=torch.int32), wide=True, wide_all=True)


# ---------------------------------------------------------------- the prepare's count
@pytest.mark.parametrize("kind", ["depthwise", "grouped_col", "grouped_perci"])
def test_prepare_counts_what_leaves_two_digits(K, kind):
    """*bad = the elements with |m| > 16319 + the elements under a factor outside [1, 16319] (each
    once) + the channels whose zero point is no code (taken as qmin), through the entry point
    itself: the wrapper refuses such factors before the call."""
    from shiftedscalequantization_amd import _capi as A
    rng = np.random.default_rng(zlib.crc32(kind.encode()))
    Co, Cig, G, R = (20, 1, 20, 3) if kind == "depthwise" else (24, 8, 3, 3)
    qw = rng.integers(0, 16, (Co, Cig, R, R))
    zw = rng.integers(0, 16, Co).astype(F32)
    zw[2], zw[Co - 1] = 3.5, 700.0                              # fractional; outside the code range
    per_ci = kind == "grouped_perci"
    k = rng.integers(1000, 3000, Co * Cig if per_ci else Cig * R * R)
    k[1], k[4], k[5] = 0, 16320, 16319
    what = qw.astype(F32)                                       # q itself: zero point 0, scale 1
    packed, nb = K.pack_encode(dev(what), dev(np.zeros(Co)), dev(np.ones(Co, F32)), False, None, 4, 0, 15)
    assert nb == 0
    zok = (zw == np.rint(zw)) & (zw >= -256) & (zw <= 511)
    z = np.where(zok, zw, 0).astype(np.int64).reshape(-1, 1, 1, 1)
    kf = (k.reshape(Co, Cig, 1, 1) if per_ci else k.reshape(1, Cig, R, R)) * np.ones(qw.shape, np.int64)
    kbad = (kf < 1) | (kf > 16319)
    over = ~kbad & (np.abs((qw - z) * kf) > 16319)
    want = int(kbad.sum() + over.sum() + (~zok).sum())
    assert kbad.any() and over.any() and (~zok).sum() == 2
    nbytes = A.query("ssq_qweight_prepared_bytes_grouped_wide", Co, Cig, R, R, G)
    assert nbytes > 0
    blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    kd = dev(k, torch.int32)
    A.call("ssq_qweight_prepare_grouped_wide", K._vp(packed), K._vp(dev(zw)), K._vp(kd), int(per_ci),
           Co, Cig, R, R, G, 4, 0, K._vp(blob), K._vp(bad), A.stream_of(blob))
    assert int(bad.item()) == want
