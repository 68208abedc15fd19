"""K31 on the device (csrc/qinfer_stemconv.hip): both output forms against the host restatement
of the contract, `chain_conv` (test_qinfer_stemconv_host.py), bit for bit.

The fp32 form is compared with view(int32) equality; the code form byte for byte with the numpy
restatement of qepi_code_y (test_qinfer_carry_host.ref_pre_quant / quant_codes / stored, the one
K27's tests use) applied to the chain's y, and with K27 run on K31's own fp32 output.  The cases
are the smallest at which the tiling can go wrong (the table in `CASES`)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from test_qinfer_carry_host import cpad, quant_codes, ref_pre_quant, stored
from test_qinfer_gpu import dev, host
from test_qinfer_host import qrange
from test_qinfer_stemconv_host import chain_conv

pytestmark = pytest.mark.gpu
F32 = np.float32

# name: (x shape, Co, (R, S), stride, padding)
CASES = {
    # ResNet form; K tail 147 -> 148; 180 pixels (pixel tail); every border class
    "r7": ((2, 3, 18, 20), 64, (7, 7), (2, 2), (3, 3)),
    # MobileNetV2 / RegNetX form; odd plane; K 27 -> 28
    "m3": ((1, 3, 9, 11), 32, (3, 3), (2, 2), (1, 1)),
    # padded channels written as 0 into a junk-filled output; a second channel tile
    "cotail24": ((1, 3, 8, 8), 24, (3, 3), (1, 1), (1, 1)),
    "cotail72": ((1, 3, 8, 8), 72, (3, 3), (1, 1), (1, 1)),
    # K 9 -> 12 and 36; no padding
    "ci1": ((2, 1, 7, 9), 16, (3, 3), (1, 1), (0, 0)),
    "ci4": ((2, 4, 7, 9), 16, (3, 3), (1, 1), (0, 0)),
    # three images inside 64 pixels; rectangular everything
    "rect": ((3, 3, 5, 5), 16, (5, 3), (1, 2), (2, 0)),
    # a row longer than one pixel tile; patch halo across tiles
    "wide": ((1, 3, 6, 150), 16, (7, 7), (2, 2), (3, 3)),
    # a stride above the kernel along each axis (the patch keeps the windows only); 48 channels
    "far": ((1, 2, 20, 23), 48, (2, 3), (3, 5), (1, 2)),
    # more rows than one tile and two row tiles
    "tall": ((1, 3, 40, 6), 16, (3, 3), (2, 1), (1, 1)),
    # the taller tiles: the launch takes 8 (then 4) tile rows only when that still leaves 512
    # workgroups, so every case above runs 2-row tiles; these leave 640 at 8 and at 4 rows, with
    # a row tail (127 = 15 * 8 + 7) and a column tail (130 = 4 * 32 + 2)
    "th8": ((8, 1, 127, 130), 16, (3, 3), (1, 1), (1, 1)),
    "th4": ((4, 1, 127, 130), 16, (3, 3), (1, 1), (1, 1)),
}
MATRIX = ("r7", "m3")
# (bias, affine, act, out bits): bias on / off, gamma^z / phi^z on / off (both signs of gamma),
# act 0 / 1 / 2, output quantizers at 8 and 4 bits, asymmetric with z != 0
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
    xs, Co, ker, stride, pad = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    x = rng.standard_normal(xs).astype(F32)
    w = (rng.standard_normal((Co, xs[1]) + ker) / np.sqrt(xs[1] * ker[0] * ker[1])).astype(F32)
    bias = rng.normal(0, 0.5, Co).astype(F32)
    gamma = rng.uniform(-1.5, 1.5, Co).astype(F32)
    gamma[0], gamma[-1] = -0.75, 1.25                 # both signs, whatever the draw
    phi = rng.normal(0, 0.3, Co).astype(F32)
    return x, w, bias, gamma, phi


@functools.lru_cache(maxsize=None)
def reference(name):
    """The chain's y for the case: computed once, shared, never written."""
    x, w = inputs(name)[:2]
    y = chain_conv(x, w, CASES[name][3], CASES[name][4])
    y.setflags(write=False)
    return y


def epilogue_args(name, epi, y):
    use_bias, use_affine, act, bits = epi
    _, _, bias, gamma, phi = inputs(name)
    bias = bias if use_bias else None
    gamma, phi = (gamma, phi) if use_affine else (None, None)
    t = ref_pre_quant(y, bias, gamma, phi, act)
    lo, hi = qrange(bits, False)
    fin = t[np.isfinite(t)]
    # half the value range on the grid: the clamp edges sit a quarter of the range inside its
    # minimum and maximum, the interior occurs, and z != 0.  Behind a ReLU / ReLU6 the range starts
    # at 0 and the lowest code is the zero point itself
    span = max(float(fin.max() - fin.min()), 1e-3)
    d = F32(span * 0.5 / (hi - lo))
    z = ZP if act else float(np.clip(np.rint(-(float(fin.min()) + 0.25 * span) / d), 1, hi))
    return bias, gamma, phi, act, d, z, bits


def ref_codes(y, bias, gamma, phi, act, d, z, bits):
    q, nbad = quant_codes(ref_pre_quant(y, bias, gamma, phi, act), d, z, bits, False)
    return stored(q, bits, False), nbad


def edges_occur(ref, Co, epi):
    """The reference holds the upper clamp edge, the interior and the lowest code the epilogue
    can reach: qmin = 0 without an activation, the zero point behind a ReLU / ReLU6 (t >= 0)."""
    act, hi = epi[2], 2 ** epi[3] - 1
    real = ref[..., :Co].astype(np.int64) + 128
    assert real.min() == (0 if act == 0 else int(ZP)) and real.max() == hi
    assert ((real > real.min()) & (real < hi)).any()


def run_codes(K, name, x, blob, bias, gamma, phi, act, d, z, bits, out=None):
    """(K31's code bytes, its NaN count); `out`: launch over this pre-filled buffer."""
    _, _, _, stride, pad = CASES[name]
    tb = lambda v: None if v is None else dev(v)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    if out is None:
        got = K.stem_conv_codes(x, blob, tb(bias), tb(gamma), tb(phi), act, float(d), float(z), bits,
                                False, bad, stride=stride, padding=pad)
        return got, int(bad.item())
    vp = K._vp
    tbias, tgamma, tphi = tb(bias), tb(gamma), tb(phi)
    N, Ci, H, W = x.shape
    Co, _, R, S = blob.shape
    K.call("ssq_stem_conv_codes_fwd", vp(x), vp(blob.blob), blob.blob.numel(), N, Ci, H, W, Co, R, S,
           *stride, *pad, vp(tbias), vp(tgamma), vp(tphi), act, float(d), float(z),
           *qrange(bits, False), vp(out), vp(bad), K.stream_of(out))
    return out, int(bad.item())


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_forms_equal_the_chain(K, name):
    xs, Co, ker, stride, pad = CASES[name]
    x, w = inputs(name)[:2]
    want = reference(name)
    tx = dev(x)
    blob = K.stem_weight_prepare(dev(w))
    y = K.stem_conv(tx, blob, stride, pad)
    assert y.dtype == torch.float32 and tuple(y.shape) == want.shape
    assert np.array_equal(host(y).view(np.int32), want.view(np.int32)), "K31's fp32 form"
    # the library conv is close, as a sanity check of the case itself (not of the contract)
    lib = torch.nn.functional.conv2d(tx, dev(w), None, stride, pad)
    assert torch.allclose(lib, y, rtol=1e-4, atol=1e-5)
    args = epilogue_args(name, PLAIN, want)
    ref, ref_bad = ref_codes(want, *args)
    got, bad = run_codes(K, name, tx, blob, *args)
    assert got.dtype == torch.int8 and tuple(got.shape) == ref.shape
    assert ref_bad == 0 and bad == 0
    assert np.array_equal(host(got), ref), "K31's codes differ from qepi_code_y on the chain"
    edges_occur(ref, Co, PLAIN)
    # every byte is written, padded channels as 0: the same launch over a junk-filled buffer
    junk = torch.full_like(got, 0x55)
    again, bad2 = run_codes(K, name, tx, blob, *args, out=junk)
    assert bad2 == 0 and np.array_equal(host(again), ref)
    assert ref.shape[-1] == cpad(Co) and not host(again)[..., Co:].any()
    # identity: K27 on K31's own fp32 output
    tb = lambda v: None if v is None else dev(v)
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    bias, gamma, phi, act, d, z, bits = args
    k27 = K.epilogue_codes(y, tb(bias), tb(gamma), tb(phi), act, float(d), float(z), bits, False, cnt)
    assert int(cnt.item()) == 0 and np.array_equal(host(k27), host(got))


def test_cases_cover_the_tiling():
    npix = lambda n: reference(n).shape[0] * reference(n).shape[2] * reference(n).shape[3]
    assert npix("r7") == 180 and reference("wide").shape[3] == 75 and npix("rect") == 30
    K_of = lambda n: CASES[n][0][1] * CASES[n][2][0] * CASES[n][2][1]
    assert [K_of(n) for n in ("r7", "m3", "ci1", "ci4")] == [147, 27, 9, 36]
    assert reference("tall").shape[2] == 20 and len(EPILOGUES) == 24
    # workgroups at TH tile rows (one channel tile): the launch's rule is >= 512
    wgs = lambda n, TH: CASES[n][0][0] * -(-CASES[n][0][2] // TH) * -(-CASES[n][0][3] // 32)
    assert wgs("th8", 8) >= 512 and wgs("th4", 8) < 512 <= wgs("th4", 4)
    assert all(wgs(n, 4) < 512 for n in CASES if n not in ("th8", "th4"))


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("name", MATRIX)
def test_epilogue_matrix(K, name, epi):
    x, w = inputs(name)[:2]
    want = reference(name)
    args = epilogue_args(name, epi, want)
    ref, ref_bad = ref_codes(want, *args)
    got, bad = run_codes(K, name, dev(x), K.stem_weight_prepare(dev(w)), *args)
    edges_occur(ref, CASES[name][1], epi)
    assert ref_bad == 0 and bad == 0 and np.array_equal(host(got), ref)


@pytest.mark.parametrize("name", MATRIX)
def test_specials_give_qmin_are_counted_and_stay_local(K, name):
    xs, Co, (R, S), (sh, sw), (ph, pw) = CASES[name]
    x, w = inputs(name)[:2]
    x = x.copy()
    spots = {(0, 0, 4, 5): np.nan, (0, 1, 0, 0): np.inf, (0, 2, xs[2] - 1, xs[3] - 2): -np.inf}
    for at, v in spots.items():
        x[at] = v
    with np.errstate(invalid="ignore"):
        y = chain_conv(x, w, (sh, sw), (ph, pw))
    clean = reference(name)
    # outputs whose window touches a special pixel, from the geometry
    touched = np.zeros(y.shape[2:], bool)
    for (_, _, h, v) in spots:
        for oh in range(y.shape[2]):
            for ow in range(y.shape[3]):
                if 0 <= h - (oh * sh - ph) < R and 0 <= v - (ow * sw - pw) < S:
                    touched[oh, ow] = True
    assert touched.any() and not touched.all()
    assert not np.isfinite(y[0][:, touched]).any()     # inf * w, then inf - inf or NaN
    args = epilogue_args(name, PLAIN, clean)
    ref, ref_bad = ref_codes(y, *args)
    tx, blob = dev(x), K.stem_weight_prepare(dev(w))
    got_y = host(K.stem_conv(tx, blob, (sh, sw), (ph, pw)))
    nan = np.isnan(y)
    assert np.array_equal(np.isnan(got_y), nan)
    assert np.array_equal(got_y[~nan].view(np.int32), y[~nan].view(np.int32))
    got, bad = run_codes(K, name, tx, blob, *args)
    got = host(got)
    assert ref_bad > 0 and bad == ref_bad and np.array_equal(got, ref)
    # a NaN / inf accumulator leaves as qmin's stored form wherever the epilogue keeps it NaN
    q, _ = quant_codes(ref_pre_quant(y, *args[:4]), *args[4:6], 8, False)
    isnan = np.moveaxis(np.isnan(q), 1, -1)
    assert isnan.sum() == ref_bad and (got[..., :Co][isnan] == -128).all()
    # neighbours whose window does not touch a special pixel are unchanged
    clean_codes = ref_codes(clean, *args)[0]
    assert np.array_equal(got[0][~touched], clean_codes[0][~touched])
    assert np.array_equal(got[1:], clean_codes[1:])


@pytest.mark.parametrize("name", ("r7", "cotail72"))
def test_two_runs_and_a_graph_replay_give_the_same_bits(K, name):
    _, _, _, stride, pad = CASES[name]
    x, w, bias = inputs(name)[:3]
    want = reference(name)
    args = epilogue_args(name, (True, False, 1, 8), want)
    tx, blob, tbias = dev(x), K.stem_weight_prepare(dev(w)), dev(bias)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    both = lambda: (K.stem_conv(tx, blob, stride, pad),
                    K.stem_conv_codes(tx, blob, tbias, None, None, 1, float(args[4]), args[5], 8, False,
                                      bad, stride=stride, padding=pad))
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
    x, w = inputs("m3")[:2]
    tx = dev(x)
    blob = K.stem_weight_prepare(dev(w))
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    out = torch.full((1, 5, 6, 32), 0x55, dtype=torch.int8, device="cuda")
    vp, nb = K._vp, blob.blob.numel()

    def raw(x=vp(tx), blob_p=vp(blob.blob), nbytes=nb, geo=(1, 3, 9, 11, 32, 3, 3), stride=(2, 2),
            pad=(1, 1), out_p=vp(out), bad_p=vp(bad)):
        K.call("ssq_stem_conv_codes_fwd", x, blob_p, nbytes, *geo, *stride, *pad, None, None, None,
               1, 0.1, 0.0, 0, 255, out_p, bad_p, K.stream_of(out))

    with pytest.raises(SSQError, match="outside K31's geometry"):
        K.stem_weight_prepare(dev(np.zeros((16, 5, 3, 3), F32)))
    with pytest.raises(SSQError, match="outside K31's geometry"):
        K.stem_weight_prepare(dev(np.zeros((16, 3, 8, 3), F32)))
    with pytest.raises(SSQError, match="stem geometry"):
        raw(geo=(1, 5, 9, 11, 32, 3, 3))
    with pytest.raises(SSQError, match="stem geometry"):
        raw(geo=(1, 3, 9, 11, 32, 8, 3))
    with pytest.raises(SSQError, match="padding"):
        raw(pad=(3, 1))
    with pytest.raises(SSQError, match="padding"):
        K.stem_conv(tx, blob, 2, (1, 3))
    for kw in (dict(x=None), dict(blob_p=None), dict(out_p=None), dict(bad_p=None)):
        with pytest.raises(SSQError, match="null"):
            raw(**kw)
    with pytest.raises(SSQError, match="prepared blob"):
        raw(nbytes=nb - 4)
    with pytest.raises(SSQError, match="prepared blob"):
        K.stem_conv(tx, K.StemWeight(blob.blob[:-16], blob.shape), 2, 1)
    with pytest.raises(SSQError, match=r"\(N, 3, H, W\)"):
        K.stem_conv(dev(np.zeros((1, 4, 9, 11), F32)), blob, 2, 1)
    with pytest.raises(SSQError, match="one entry per"):
        K.stem_conv_codes(tx, blob, dev(np.ones(5, F32)), None, None, 1, 0.1, 0.0, 8, False, bad,
                          stride=2, padding=1)
    torch.cuda.synchronize()
    assert int(bad.item()) == 7 and bool((out == 0x55).all())
    raw()                                                   # and the same call, valid, writes
    assert int(bad.item()) == 7 and not bool((out == 0x55).all())
