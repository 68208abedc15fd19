"""K32 on the device (csrc/qinfer_stemu8.hip): both output forms against the numpy restatement of
the contract, `u8_stem_ref` (test_qinfer_stemu8_host.py), bit for bit.

The fp32 form is compared with view(int32) equality; the code form byte for byte with the numpy
restatement of qepi_code_y (test_qinfer_carry_host.ref_pre_quant / quant_codes / stored) applied
to the restatement's y, and with K27 run on K32's own fp32 output.  The cases are the smallest at
which the tiling can go wrong (the table in `CASES`)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from test_qinfer_carry_host import cpad, quant_codes, ref_pre_quant, stored
from test_qinfer_gpu import dev, host
from test_qinfer_host import qrange
from test_qinfer_stemu8_host import MEAN, STD, pack_codes, u8_stem_ref, u8_tables_ref

pytestmark = pytest.mark.gpu
F32 = np.float32

# name: (u shape, Co, (R, S), stride, padding, weight bits, symmetric, per-(co, ci) scale)
CASES = {
    # ResNet form: one k step of 49 taps, a full channel tile, odd plane, a column tile tail
    "r7": ((2, 3, 19, 37), 64, (7, 7), (2, 2), (3, 3), 8, False, False),
    # MobileNetV2 / RegNetX form; a second channel tile (72 = 64 + 8)
    "m3": ((2, 3, 17, 33), 72, (3, 3), (2, 2), (1, 1), 8, False, False),
    "m3co8": ((2, 3, 17, 33), 8, (3, 3), (2, 2), (1, 1), 8, True, False),
    "m3co64": ((2, 3, 17, 33), 64, (3, 3), (2, 2), (1, 1), 4, False, True),
    # stride 1, four input channels, a fragment tail (8 of 16 channels), two column tiles
    "s1": ((1, 4, 9, 40), 8, (3, 3), (1, 1), (1, 1), 4, True, True),
    # one input channel, rectangular kernel, stride and padding, no padding along w
    "rect": ((1, 1, 12, 35), 8, (5, 3), (2, 1), (2, 0), 8, False, False),
    # a plane on which interior and border tiles both occur (24 x 3 tiles of 2 x 32)
    "plane": ((1, 3, 96, 160), 64, (7, 7), (2, 2), (3, 3), 8, False, False),
    # a stride above the kernel along each axis (the patch keeps the windows only); 48 channels
    "far": ((1, 2, 20, 23), 48, (2, 3), (3, 5), (1, 2), 2, True, False),
    # the taller tiles: 8 (then 4) tile rows only when that still leaves 512 workgroups
    "th8": ((8, 1, 127, 130), 16, (3, 3), (1, 1), (1, 1), 8, False, False),
    "th4": ((4, 1, 127, 130), 16, (3, 3), (1, 1), (1, 1), 8, False, False),
}
MATRIX = ("r7", "m3")
EPILOGUES = list(itertools.product((False, True), (False, True), (0, 1, 2), (8, 4)))
PLAIN = (True, True, 1, 8)
ZP = 3.0


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


@functools.lru_cache(maxsize=None)
def inputs(name):
    us, Co, ker, _, _, bits, sym, per_ci = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 320)
    lo, hi = qrange(bits, sym)
    u = rng.integers(0, 256, us).astype(np.uint8)
    qw = rng.integers(lo, hi + 1, (Co, us[1]) + ker)
    zw = rng.integers(lo, hi + 1, Co)
    zw[0], zw[-1] = lo, hi
    d = (rng.uniform(0.5, 2.0, (Co, us[1]) if per_ci else Co) / (hi - lo)).astype(F32)
    bias = rng.normal(0, 0.5, Co).astype(F32)
    gamma = rng.uniform(-1.5, 1.5, Co).astype(F32)
    gamma[0], gamma[-1] = -0.75, 1.25                 # both signs, whatever the draw
    phi = rng.normal(0, 0.3, Co).astype(F32)
    return u, qw, zw, lo, d, bias, gamma, phi


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's y for the case: computed once, shared, never written."""
    u, qw, zw, lo, d = inputs(name)[:5]
    y = u8_stem_ref(u, qw, zw, lo, d, MEAN, STD, CASES[name][3], CASES[name][4])
    y.setflags(write=False)
    return y


def prepare(K, qw, zw, lo, bits, d, zp=None):
    """(StemU8Weight, M, s) on the device from integer codes."""
    Co, Ci = qw.shape[:2]
    packed = torch.as_tensor(pack_codes(qw, lo, bits)).cuda()
    prep = K.stem_u8_weight_prepare(packed, qw.shape, dev(zw if zp is None else zp), bits, lo)
    M, s = K.stem_u8_tables(torch.tensor(MEAN[:Ci]), torch.tensor(STD[:Ci]), dev(d), Co, Ci)
    return prep, M, s


def operands(K, name):
    u, qw, zw, lo, d = inputs(name)[:5]
    prep, M, s = prepare(K, qw, zw, lo, CASES[name][5], d)
    assert int(prep.bad.item()) == 0
    Mr, sr = u8_tables_ref(MEAN, STD, d, *qw.shape[:2])
    assert np.array_equal(host(M).view(np.int32), Mr.view(np.int32))
    assert np.array_equal(host(s).view(np.int32), sr.view(np.int32))
    return torch.as_tensor(u).cuda(), prep, M, s


def epilogue_args(name, epi, y):
    use_bias, use_affine, act, bits = epi
    bias, gamma, phi = inputs(name)[5:]
    bias = bias if use_bias else None
    gamma, phi = (gamma, phi) if use_affine else (None, None)
    t = ref_pre_quant(y, bias, gamma, phi, act)
    lo, hi = qrange(bits, False)
    fin = t[np.isfinite(t)]
    # half the value range on the grid: both clamp edges and the interior occur, and z != 0
    span = max(float(fin.max() - fin.min()), 1e-3)
    d = F32(span * 0.5 / (hi - lo))
    z = ZP if act else float(np.clip(np.rint(-(float(fin.min()) + 0.25 * span) / d), 1, hi))
    return bias, gamma, phi, act, d, z, bits


def ref_codes(y, bias, gamma, phi, act, d, z, bits):
    q, nbad = quant_codes(ref_pre_quant(y, bias, gamma, phi, act), d, z, bits, False)
    return stored(q, bits, False), nbad


def edges_occur(ref, Co, epi):
    act, hi = epi[2], 2 ** epi[3] - 1
    real = ref[..., :Co].astype(np.int64) + 128
    assert real.min() == (0 if act == 0 else int(ZP)) and real.max() == hi
    assert ((real > real.min()) & (real < hi)).any()


def run_codes(K, name, ops, bias, gamma, phi, act, d, z, bits, out=None, border=False):
    """(K32's code bytes, its NaN count); `out`: launch over this pre-filled buffer."""
    stride, pad = CASES[name][3], CASES[name][4]
    tu, prep, M, s = ops
    tb = lambda v: None if v is None else dev(v)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    if out is None:
        got = K.stem_conv_u8_codes(tu, prep, M, s, tb(bias), tb(gamma), tb(phi), act, float(d),
                                   float(z), bits, False, bad, stride=stride, padding=pad,
                                   every_tile_border=border)
        return got, int(bad.item())
    vp = K._vp
    tbias, tgamma, tphi = tb(bias), tb(gamma), tb(phi)
    N, Ci, H, W = tu.shape
    Co, _, R, S = prep.shape
    K.call("ssq_stem_conv_u8_codes_fwd", vp(tu), vp(prep.blob), prep.blob.numel(), vp(M), vp(s), N,
           Ci, H, W, Co, R, S, *stride, *pad, int(border), vp(tbias), vp(tgamma), vp(tphi), act,
           float(d), float(z), *qrange(bits, False), vp(out), vp(bad), K.stream_of(out))
    return out, int(bad.item())


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_forms_equal_the_restatement(K, name):
    us, Co, ker, stride, pad = CASES[name][:5]
    want = reference(name)
    ops = operands(K, name)
    tu, prep, M, s = ops
    y = K.stem_conv_u8(tu, prep, M, s, stride, pad)
    assert y.dtype == torch.float32 and tuple(y.shape) == want.shape
    assert np.array_equal(host(y).view(np.int32), want.view(np.int32)), "K32's fp32 form"
    # forcing the border path on every tile gives the same bits
    yb = K.stem_conv_u8(tu, prep, M, s, stride, pad, every_tile_border=True)
    assert torch.equal(yb.view(torch.int32), y.view(torch.int32))
    args = epilogue_args(name, PLAIN, want)
    ref, ref_bad = ref_codes(want, *args)
    got, bad = run_codes(K, name, ops, *args)
    assert got.dtype == torch.int8 and tuple(got.shape) == ref.shape
    assert ref_bad == 0 and bad == 0
    assert np.array_equal(host(got), ref), "K32's codes differ from qepi_code_y on the restatement"
    edges_occur(ref, Co, PLAIN)
    # every byte is written, padded channels as 0: the same launch over a junk-filled buffer,
    # this time with every tile on the border path
    junk = torch.full_like(got, 0x55)
    again, bad2 = run_codes(K, name, ops, *args, out=junk, border=True)
    assert bad2 == 0 and np.array_equal(host(again), ref)
    assert ref.shape[-1] == cpad(Co) and not host(again)[..., Co:].any()
    # identity: K27 on K32's own fp32 output
    tb = lambda v: None if v is None else dev(v)
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    bias, gamma, phi, act, d, z, bits = args
    k27 = K.epilogue_codes(y, tb(bias), tb(gamma), tb(phi), act, float(d), float(z), bits, False, cnt)
    assert int(cnt.item()) == 0 and np.array_equal(host(k27), host(got))


def test_cases_cover_the_tiling(K):
    shapes = {n: reference(n).shape for n in CASES if n not in ("th8", "th4")}
    assert shapes["r7"][2:] == (10, 19) and shapes["m3"][2:] == (9, 17)
    assert shapes["s1"][2:] == (9, 40) and shapes["rect"][2:] == (6, 33)
    assert {CASES[n][1] for n in ("m3co8", "m3co64", "m3")} == {8, 64, 72}
    assert {(CASES[n][5], CASES[n][7]) for n in CASES} >= {(8, False), (4, True)}
    # both paths run on the plane, and only the border path on the small cases
    tiles = lambda n, codes: K.stem_u8_tiles(K.StemU8Weight(None, (CASES[n][1], CASES[n][0][1])
                                                            + CASES[n][2], None),
                                             CASES[n][0], CASES[n][3], CASES[n][4], codes)
    for codes in (False, True):
        inner, border = tiles("plane", codes)
        assert inner == 22 and border == 50
        assert tiles("r7", codes)[0] == 0 and tiles("m3", codes)[0] == 0
        assert tiles("rect", codes) == (1, 5)         # rows 2..3 of the first 32 columns
    # workgroups at TH tile rows (one channel tile): the launch's rule is >= 512
    wgs = lambda n, TH: CASES[n][0][0] * -(-CASES[n][0][2] // TH) * -(-CASES[n][0][3] // 32)
    assert wgs("th8", 8) >= 512 and wgs("th4", 8) < 512 <= wgs("th4", 4)
    assert tiles("th8", True)[0] > 0 and tiles("th4", True)[0] > 0
    assert all(wgs(n, 4) < 512 for n in CASES if n not in ("th8", "th4"))


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("name", MATRIX)
def test_epilogue_matrix(K, name, epi):
    want = reference(name)
    args = epilogue_args(name, epi, want)
    ref, ref_bad = ref_codes(want, *args)
    got, bad = run_codes(K, name, operands(K, name), *args)
    edges_occur(ref, CASES[name][1], epi)
    assert ref_bad == 0 and bad == 0 and np.array_equal(host(got), ref)


@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("q,z", [(255, 0), (0, 255)])
def test_extreme_images_and_weights(K, fill, q, z):
    """Images of all 0 and all 255 against weights at a code extreme with the zero point at the
    other: |A_c| at its bound 49 * 255 * 255, and a padded tap is x = 0, not u = 0."""
    us, Co, ker, stride, pad = CASES["r7"][:5]
    rng = np.random.default_rng(fill + q)
    u = np.full(us, fill, np.uint8)
    qw, zw = np.full((Co, us[1]) + ker, q), np.full(Co, z)
    d = rng.uniform(0.002, 0.01, Co).astype(F32)
    want = u8_stem_ref(u, qw, zw, 0, d, MEAN, STD, stride, pad)
    prep, M, s = prepare(K, qw, zw, 0, 8, d)
    assert int(prep.bad.item()) == 0
    for border in (False, True):
        y = K.stem_conv_u8(torch.as_tensor(u).cuda(), prep, M, s, stride, pad, every_tile_border=border)
        assert np.array_equal(host(y).view(np.int32), want.view(np.int32))
    # a corner output sees fewer taps than an interior one
    assert abs(want[0, 0, 0, 0]) < abs(want[0, 0, 5, 9])


def test_bad_counting(K):
    """The prepare counts the channels whose zero point is not an integer code (taken as qmin);
    the code form counts a NaN y, stores qmin, and leaves every other element alone."""
    name = "m3"
    u, qw, zw, lo, d = inputs(name)[:5]
    stride, pad = CASES[name][3], CASES[name][4]
    Co = qw.shape[0]
    zp = zw.astype(F32)
    zp[1], zp[5], zp[70] = 0.5, 1000.0, np.nan
    prep, M, s = prepare(K, qw, zw, lo, 8, d, zp=zp)
    assert int(prep.bad.item()) == 3
    as_qmin = zw.copy()
    as_qmin[[1, 5, 70]] = lo
    tu = torch.as_tensor(u).cuda()
    y = K.stem_conv_u8(tu, prep, M, s, stride, pad)
    want = u8_stem_ref(u, qw, as_qmin, lo, d, MEAN, STD, stride, pad)
    assert np.array_equal(host(y).view(np.int32), want.view(np.int32))
    # a NaN in the table of channel 2: all of its outputs are NaN
    ops = operands(K, name)
    s2 = ops[3].clone()
    s2[2, 1] = float("nan")
    clean = reference(name)
    args = epilogue_args(name, PLAIN, clean)
    got, bad = run_codes(K, name, (ops[0], ops[1], ops[2], s2), *args)
    npix = clean.shape[0] * clean.shape[2] * clean.shape[3]
    ref = ref_codes(clean, *args)[0]
    got = host(got)
    assert bad == npix and (got[..., 2] == -128).all()
    keep = np.arange(got.shape[-1]) != 2
    assert np.array_equal(got[..., keep], ref[..., keep])


@pytest.mark.parametrize("name", ("r7", "m3"))
def test_two_runs_and_a_graph_replay_give_the_same_bits(K, name):
    stride, pad = CASES[name][3], CASES[name][4]
    bias = inputs(name)[5]
    want = reference(name)
    args = epilogue_args(name, (True, False, 1, 8), want)
    tu, prep, M, s = operands(K, name)
    tbias = dev(bias)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    both = lambda: (K.stem_conv_u8(tu, prep, M, s, stride, pad),
                    K.stem_conv_u8_codes(tu, prep, M, s, tbias, None, None, 1, float(args[4]),
                                         args[5], 8, False, bad, stride=stride, padding=pad))
    y1, c1 = both()
    y2, c2 = both()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)) and torch.equal(c1, c2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yg, cg = both()
    yg.zero_()
    cg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg.view(torch.int32), y1.view(torch.int32)) and torch.equal(cg, c1)
    assert np.array_equal(host(yg).view(np.int32), want.view(np.int32)) and int(bad.item()) == 0


def test_refusals_raise_before_any_launch(K):
    from shiftedscalequantization_amd._capi import SSQError
    name = "m3co8"
    tu, prep, M, s = operands(K, name)
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    out = torch.full((2, 9, 17, 16), 0x55, dtype=torch.int8, device="cuda")
    vp, nb = K._vp, prep.blob.numel()

    def raw(u=vp(tu), blob_p=vp(prep.blob), nbytes=nb, M_p=vp(M), s_p=vp(s),
            geo=(2, 3, 17, 33, 8, 3, 3), stride=(2, 2), pad=(1, 1), out_p=vp(out), bad_p=vp(bad)):
        K.call("ssq_stem_conv_u8_codes_fwd", u, blob_p, nbytes, M_p, s_p, *geo, *stride, *pad, 0,
               None, None, None, 1, 0.1, 0.0, 0, 255, out_p, bad_p, K.stream_of(out))

    packed = torch.zeros(16 * 5 * 9, dtype=torch.uint8, device="cuda")
    with pytest.raises(SSQError, match="outside K32's geometry"):
        K.stem_u8_weight_prepare(packed, (16, 5, 3, 3), dev(np.zeros(16, F32)), 8, 0)
    with pytest.raises(SSQError, match="outside K32's geometry"):
        K.stem_u8_weight_prepare(packed, (16, 3, 8, 3), dev(np.zeros(16, F32)), 8, 0)
    with pytest.raises(SSQError, match="too small"):
        K.stem_u8_weight_prepare(packed[:100], (16, 3, 3, 3), dev(np.zeros(16, F32)), 8, 0)
    with pytest.raises(SSQError, match="one entry per output channel"):
        K.stem_u8_weight_prepare(packed, (16, 3, 3, 3), dev(np.zeros(15, F32)), 8, 0)
    with pytest.raises(SSQError, match="stem geometry"):
        raw(geo=(2, 5, 17, 33, 8, 3, 3))
    with pytest.raises(SSQError, match="stem geometry"):
        raw(geo=(2, 3, 17, 33, 8, 8, 3))
    with pytest.raises(SSQError, match="padding"):
        raw(pad=(3, 1))
    with pytest.raises(SSQError, match="padding"):
        K.stem_conv_u8(tu, prep, M, s, 2, (1, 3))
    for kw in (dict(u=None), dict(blob_p=None), dict(M_p=None), dict(s_p=None), dict(out_p=None),
               dict(bad_p=None)):
        with pytest.raises(SSQError, match="null"):
            raw(**kw)
    with pytest.raises(SSQError, match="prepared blob"):
        raw(nbytes=nb - 4)
    with pytest.raises(SSQError, match=r"\(N, 3, H, W\)"):
        K.stem_conv_u8(torch.zeros(1, 4, 9, 11, dtype=torch.uint8, device="cuda"), prep, M, s, 2, 1)
    with pytest.raises(SSQError, match="uint8"):
        K.stem_conv_u8(tu.float(), prep, M, s, 2, 1)
    with pytest.raises(SSQError, match="stem_u8_tables"):
        K.stem_conv_u8(tu, prep, M, s[:4], 2, 1)
    with pytest.raises(SSQError, match="one entry per"):
        K.stem_conv_u8_codes(tu, prep, M, s, dev(np.ones(5, F32)), None, None, 1, 0.1, 0.0, 8, False,
                             bad, stride=2, padding=1)
    torch.cuda.synchronize()
    assert int(bad.item()) == 7 and bool((out == 0x55).all())
    raw()                                                   # and the same call, valid, writes
    assert int(bad.item()) == 7 and not bool((out == 0x55).all())
