"""K23 split along K on the device (ssq_qconv_i8_*splitk_*; kernels.qconv / qconv_codes with
splits=Z).  The integer sum is exact and associative, so the oracle is twofold and exact: the
bytes of the unsplit entry point on the same inputs, and the host int64 references the unsplit
tests use (ref_output; ref_codes / ref_codes_res for the code forms).  Cases are the smallest
that can go wrong: uneven slices with K, Co and M tails, many slices, two channel tiles with an M
tail, 1x1 stride 2, a linear, padded taps that land in different slices, H != W; each of the four
epilogue forms on plain and centred blobs; the accumulator's edges; a workspace that is junk
before the call and fenced by sentinels; every refusal."""
import functools
import types
import zlib

import numpy as np
import pytest
import torch

from test_qinfer_carry_gpu import pick_quantizer
from test_qinfer_carry_host import cpad, quant_codes, ref_pre_quant, stored
from test_qinfer_colscale_gpu import draw_weight, encode_colscale
from test_qinfer_colscale_host import colscale_scale
from test_qinfer_colscale_host import ref_output as ref_output_colscale
from test_qinfer_gpu import SHAPES as BASE_SHAPES
from test_qinfer_gpu import dev, encode_weight, host
from test_qinfer_host import qrange, ref_output
from test_qinfer_tail_gpu import RES_Q
from test_qinfer_tail_host import decode_res

pytestmark = pytest.mark.gpu
F32 = np.float32

# (N, Ci, H, W, Co, R, stride, pad); H = None: a linear.  test_qinfer_gpu's, plus two channel
# tiles (Co = 80) with an M tail (M = 50)
SHAPES = dict(BASE_SHAPES, co80_m50=(2, 16, 5, 5, 80, 3, 1, 1))
# (weight bits, weight sym, act bits, act sym)
W2A4, W8A8, W8A8S, W4A2 = (2, False, 4, False), (8, False, 8, False), (8, True, 8, True), (4, False, 2, False)
WIDTHS = [W2A4, W8A8, W8A8S, W4A2]
# (shape, Z): nk is the shape's k steps
SPLITS = [("k180_tails", 2), ("k180_tails", 3), ("k180_tails", 5),             # nk = 5; Co 33; M 75
          ("k1440", 2), ("k1440", 4), ("k1440", 8), ("k1440", 16),             # nk = 23
          ("co80_m50", 2), ("co80_m50", 3),                                    # nk = 3
          ("ci130_s2", 2), ("ci130_s2", 3),                                    # nk = 3, 1x1 stride 2
          ("linear", 2),                                                       # nk = 2
          ("7x7", 4),                                                          # nk = 13, pad 3
          ("nonsquare", 3)]                                                    # nk = 3, H != W
CASES = [(n, Z, WIDTHS[(i + j) % 4]) for i, (n, Z) in enumerate(SPLITS) for j in (0, 1)]
FORM_SHAPES = ("k180_tails", "co80_m50")
FORMS = ("fp32", "codes", "res_fp32", "res_codes")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def nk_of(name):
    N, Ci, H, W, Co, R, stride, pad = SHAPES[name]
    return -(-R * R * cpad(Ci) // 64)


def test_cases_cover_every_width_and_shape():
    assert {b for _, _, b in CASES} == set(WIDTHS)
    assert {(n, Z) for n, Z, _ in CASES} == set(SPLITS)
    assert {n for n, _ in SPLITS} >= {"k180_tails", "k1440", "co80_m50", "ci130_s2", "linear", "7x7",
                                      "nonsquare"}
    assert [nk_of(n) for n in ("k180_tails", "k1440", "co80_m50", "ci130_s2", "linear", "7x7")] == \
        [5, 23, 3, 3, 2, 13]
    assert all(2 <= Z <= min(16, nk_of(n)) for n, Z in SPLITS)
    assert ("k180_tails", 5) in SPLITS and ("k1440", 16) in SPLITS      # Z = nk; Z = the ABI's bound
    N, Ci, H, W, Co, R, stride, pad = SHAPES["co80_m50"]
    assert Co == 80 and N * ((H + 2 * pad - R) // stride + 1) ** 2 == 50


@functools.lru_cache(maxsize=None)
def layer(name, bits, centred=False):
    """Seeded integer codes of one layer, its prepared weight (a column-scaled, centred blob with
    `centred`), the encoded input and the host reference of the fp32 output, made once."""
    from shiftedscalequantization_amd import kernels as K
    N, Ci, H, W, Co, R, stride, pad = SHAPES[name]
    wb, wsym, ab, asym = bits
    linear = H is None
    rng = np.random.default_rng(zlib.crc32(repr((name, bits, centred)).encode()))
    alo, ahi = qrange(ab, asym)
    L = types.SimpleNamespace(name=name, stride=stride, pad=pad, Co=Co, linear=linear)
    L.qa = rng.integers(alo, ahi + 1, (N, Ci, 1, 1) if linear else (N, Ci, H, W))
    L.za = int(rng.integers(alo, ahi + 1))
    da = F32(rng.uniform(0.01, 0.2))
    d1 = rng.uniform(1e-3, 2e-2, Co).astype(F32)
    wshape = (Co, Ci) if linear else (Co, Ci, R, R)
    if centred:
        assert not wsym and wb <= 4
        qw, zw, k = draw_weight(rng, (Co, Ci, R, R), wb, 8)
        _, packed = encode_colscale(K, qw, zw, d1, k, 8, wb)
        L.prep = K.qweight_prepare(packed, wshape, dev(zw), wb, 0, kcol=torch.from_numpy(k))
        assert L.prep.centred and int(L.prep.bad.item()) == 0
        L.scale = colscale_scale(da, d1, 8)
        L.ref_with = lambda scale: ref_output_colscale(L.qa, L.za, qw, zw, k, scale, stride, pad)
    else:
        wlo, whi = qrange(wb, wsym)
        qw = rng.integers(wlo, whi + 1, (Co, Ci, R, R))
        zw = rng.integers(wlo, whi + 1, Co)
        _, L.prep = encode_weight(K, qw.reshape(wshape), zw, d1, wb, wsym)
        L.scale = da * d1
        L.ref_with = lambda scale: ref_output(L.qa, L.za, qw, zw, scale, stride, pad)
    L.ref = L.ref_with(L.scale)
    xhat = (L.qa - L.za).astype(F32) * da
    L.codes, bad = K.act_encode(dev(xhat.reshape(N, Ci) if linear else xhat), float(da), float(L.za),
                                ab, asym)
    assert int(bad.item()) == 0
    L.az = alo + 128 - L.za
    L.kw = dict(act_zp=float(L.za), act_bits=ab, act_sym=asym)
    return L


def run_fp32(K, L, Z, **kw):
    y = K.qconv(L.codes, L.prep, dev(L.scale), L.stride, L.pad, splits=Z, **L.kw, **kw)
    torch.cuda.synchronize()
    return host(y).reshape(L.ref.shape)


# ---------------------------------------------------------------- 1. the fp32 form
@pytest.mark.parametrize("name,Z,bits", CASES)
def test_split_fp32_equals_unsplit_and_host_reference(K, name, Z, bits):
    L = layer(name, bits)
    whole, split = run_fp32(K, L, None), run_fp32(K, L, Z)
    np.testing.assert_array_equal(whole.view(np.int32), L.ref.view(np.int32))
    np.testing.assert_array_equal(split.view(np.int32), whole.view(np.int32))


def test_splits_one_is_the_unsplit_path(K):
    L = layer("k180_tails", W2A4)
    np.testing.assert_array_equal(run_fp32(K, L, 1).view(np.int32), L.ref.view(np.int32))


# ---------------------------------------------------------------- 2. the four forms, both blobs
def epilogue(L, rng, form, rq, nan_channel=None):
    """The epilogue operands of one case and its host reference codes: bias, gamma / phi, ReLU, an
    output quantizer with both clamp edges inside the data, and the form's residual."""
    Co = L.Co
    E = types.SimpleNamespace(act=1)
    E.bias = rng.normal(0, 1.0, Co).astype(F32)
    E.gamma, E.phi = rng.uniform(0.5, 1.5, Co).astype(F32), rng.normal(0, 0.5, Co).astype(F32)
    # the conv's outputs brought to a few units
    E.scale = (L.scale * F32(4.0 / max(float(L.ref.std()), 1e-6))).astype(F32)
    y = L.ref_with(E.scale)
    dims = y.shape
    E.res = E.res_codes = E.rquant = None
    if form == "res_fp32":
        E.res = rng.normal(0, 2.0, dims).astype(F32)
        if nan_channel is not None:
            E.res[:, nan_channel] = np.nan
    elif form == "res_codes":
        rb, rsym, rz = rq
        lo, hi = qrange(rb, rsym)
        rd = F32(4.0 / (hi - lo))
        E.res_codes = stored(rng.integers(lo, hi + 1, dims).astype(F32), rb, rsym)
        E.rquant = (float(rd), float(rz), rb, rsym)
        E.res = decode_res(E.res_codes, Co, rd, rz, rb, rsym)
    t = ref_pre_quant(y, E.bias, E.gamma, E.phi, 0 if E.res is not None else E.act)
    if E.res is not None:
        with np.errstate(invalid="ignore"):
            t = ref_pre_quant((t + E.res).astype(F32), None, None, None, E.act)
    E.d, E.z = pick_quantizer(t, 4, False)
    q, E.ref_bad = quant_codes(t, E.d, E.z, 4, False)
    E.ref = stored(q, 4, False)
    return E


def run_codes(K, L, E, Z, **kw):
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = None
    if E.res_codes is not None:
        res = K.carried(dev(E.res_codes, torch.int8), E.res.shape, *E.rquant)
    elif E.res is not None:
        res = dev(E.res)
    out = K.qconv_codes(L.codes, L.prep, dev(E.scale), L.stride, L.pad, bias=dev(E.bias),
                        gamma=dev(E.gamma), phi=dev(E.phi), relu=E.act, out_delta=float(E.d),
                        out_zp=float(E.z), out_bits=4, out_sym=False, bad=bad, residual=res,
                        splits=Z, **L.kw, **kw)
    torch.cuda.synchronize()
    return host(out), int(bad.item())


FORM_CASES = [(n, Z, f, c) for n, Z in (("k180_tails", 3), ("co80_m50", 2)) for f in FORMS
              for c in (False, True)]


@pytest.mark.parametrize("name,Z,form,centred", FORM_CASES)
def test_every_form_on_both_blobs(K, name, Z, form, centred):
    L = layer(name, W2A4, centred)
    assert L.az != 0
    assert bool(L.prep.centred) == centred and K.QCONV_CENTRED
    if form == "fp32":
        whole, split = run_fp32(K, L, None), run_fp32(K, L, Z)
        np.testing.assert_array_equal(whole.view(np.int32), L.ref.view(np.int32))
        np.testing.assert_array_equal(split.view(np.int32), whole.view(np.int32))
        return
    rng = np.random.default_rng(zlib.crc32(repr((name, form, centred)).encode()))
    for rq in (RES_Q if form == "res_codes" else RES_Q[:1]):
        E = epilogue(L, rng, form, rq)
        whole, bad_w = run_codes(K, L, E, None)
        split, bad_s = run_codes(K, L, E, Z)
        real = E.ref[..., :L.Co].astype(np.int64) + 128
        assert (real == 0).any() and (real == 15).any() and ((real > 0) & (real < 15)).any()
        assert E.ref_bad == 0 and bad_w == 0 and bad_s == 0
        assert split.shape[-1] == cpad(L.Co) and not split[..., L.Co:].any()
        assert np.array_equal(whole, E.ref), "unsplit codes differ from the host reference"
        assert np.array_equal(split, whole), "split codes differ from the unsplit kernel's"


@pytest.mark.parametrize("centred", [False, True])
def test_nan_residual_channel_is_qmin_and_counted_the_same(K, centred):
    L = layer("k180_tails", W2A4, centred)
    E = epilogue(L, np.random.default_rng(19), "res_fp32", None, nan_channel=L.Co // 2)
    whole, bad_w = run_codes(K, L, E, None)
    split, bad_s = run_codes(K, L, E, 5)
    npix = E.ref.shape[0] * E.ref.shape[1] * E.ref.shape[2]
    assert E.ref_bad == npix and bad_w == npix and bad_s == npix
    assert (split[..., L.Co // 2] == -128).all()          # qmin's stored form
    assert np.array_equal(whole, E.ref) and np.array_equal(split, whole)


# ---------------------------------------------------------------- 3. accumulator edges
def _extreme(K, qa, za, qw, zw, stride, pad, Z, linear=False):
    """Straight from 8-bit codes at delta 1 (x_hat = q - z exactly): split, unsplit, reference."""
    Co = qw.shape[0]
    scale = np.linspace(0.5, 1.5, Co).astype(F32)
    wshape = qw.shape[:2] if linear else qw.shape
    _, prep = encode_weight(K, qw.reshape(wshape), zw, np.ones(Co, F32), 8, False)
    xhat = (qa - za).astype(F32)
    codes, bad = K.act_encode(dev(xhat.reshape(xhat.shape[:2]) if linear else xhat), 1.0, float(za),
                              8, False)
    assert int(bad.item()) == 0
    kw = dict(act_zp=float(za), act_bits=8, act_sym=False)
    ref = ref_output(qa, za, qw, zw, scale, stride, pad)
    whole = host(K.qconv(codes, prep, dev(scale), stride, pad, **kw)).reshape(ref.shape)
    split = host(K.qconv(codes, prep, dev(scale), stride, pad, splits=Z, **kw)).reshape(ref.shape)
    np.testing.assert_array_equal(whole.view(np.int32), ref.view(np.int32))
    np.testing.assert_array_equal(split.view(np.int32), whole.view(np.int32))


@pytest.mark.parametrize("a,w", [(0, 0), (255, 255), (0, 255), (255, 0)])
def test_operands_at_the_int8_edges_k4608(K, a, w):
    """512 channels, 3x3 on a 2x2 plane, nk = 72, Z = 8: every stored operand is -128 (code 0) or
    127 (code 255); with the zero point at the activation's own code a padded tap holds it too."""
    qa, qw = np.full((1, 512, 2, 2), a), np.full((16, 512, 3, 3), w)
    zw = np.full(16, 255 - w)
    _extreme(K, qa, a, qw, zw, 1, 1, 8)
    _extreme(K, qa, 255 - a, qw, zw, 1, 1, 8)


@pytest.mark.parametrize("a,w", [(0, 0), (0, 255)])
def test_linear_k65536_reaches_the_accumulator_bound(K, a, w):
    """A linear at K = 65536, Z = 16 (64 k steps a slice): with all stored operands at -128 the
    whole-K D is 65536 * 128 * 128 = 2^30, and with the zero points at the other end |I| passes
    2^31."""
    qa, qw = np.full((2, 65536, 1, 1), a), np.full((16, 65536, 1, 1), w)
    zw = np.full(16, 255 - w)
    I = (a - (255 - a)) * (w - (255 - w)) * 65536
    assert abs(I) > 2 ** 31 and 65536 * 128 * 128 == 2 ** 30
    _extreme(K, qa, 255 - a, qw, zw, 1, 0, 16, linear=True)


# ---------------------------------------------------------------- 4. workspace discipline
@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("form", ["fp32", "codes"])
def test_workspace_is_fully_written_and_never_overrun(K, form, centred):
    """Junk in the workspace changes nothing (every element read was written first), and 256
    sentinel bytes on each side of it stay untouched."""
    L = layer("k180_tails", W2A4, centred)
    Z = 3
    N, Ci, H, W, Co, R, stride, pad = SHAPES["k180_tails"]
    need = K.qconv_split_workspace_bytes(L.prep, N, H, W, stride, pad, Z)
    assert need == Z * (Co + (0 if centred else 1)) * 75 * 4
    E = epilogue(L, np.random.default_rng(5), "codes", None) if form == "codes" else None
    run = (lambda **kw: run_fp32(K, L, Z, **kw).view(np.int32)) if E is None else \
        (lambda **kw: run_codes(K, L, E, Z, **kw)[0])
    want = run()
    buf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = buf[256:256 + need]
    ws.fill_(0x7F)
    got = run(workspace=ws)
    assert np.array_equal(got, want)
    fence = host(buf)
    assert (fence[:256] == 0xA5).all() and (fence[-256:] == 0xA5).all()
    assert (fence[256:-256] != 0x7F).any()
    if E is not None:
        assert np.array_equal(want, E.ref)


# ---------------------------------------------------------------- 5. refusals
def test_wrapper_refusals(K):
    from shiftedscalequantization_amd._capi import SSQError
    from test_qinfer_grouped_gpu import encode_weight as encode_weight_grouped
    L = layer("k180_tails", W2A4)                       # nk = 5
    N, Ci, H, W, Co, R, stride, pad = SHAPES["k180_tails"]
    E = epilogue(L, np.random.default_rng(3), "res_fp32", None)
    before = run_fp32(K, L, None)
    for Z in (0, -1, 17, 6):
        with pytest.raises(SSQError, match="splits"):
            run_fp32(K, L, Z)
        with pytest.raises(SSQError, match="splits"):
            run_codes(K, L, E, Z)
    need = K.qconv_split_workspace_bytes(L.prep, N, H, W, stride, pad, 2)
    short = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(SSQError, match="workspace"):
        run_fp32(K, L, 2, workspace=short)
    with pytest.raises(SSQError, match="workspace"):
        run_codes(K, L, E, 2, workspace=short)
    with pytest.raises(SSQError, match="workspace"):
        run_fp32(K, L, 2, workspace=torch.empty(need, dtype=torch.float32, device="cuda"))
    with pytest.raises(SSQError, match="workspace"):
        run_fp32(K, L, 2, workspace=torch.empty(need, dtype=torch.uint8))
    # what the parent refuses, refused with a split as well
    with pytest.raises(SSQError, match="zero point"):
        K.qconv(L.codes, L.prep, dev(L.scale), stride, pad, act_zp=4.5, act_bits=4, splits=2)
    # a grouped weight has no split form
    rng = np.random.default_rng(2)
    qw, zw = rng.integers(0, 4, (8, 8, 3, 3)), rng.integers(0, 4, 8)
    _, gprep = encode_weight_grouped(K, qw, zw, np.ones(8, F32), 2, False, 2)
    gcodes = torch.zeros((1, 4, 4, 16), dtype=torch.int8, device="cuda")
    with pytest.raises(SSQError, match="dense"):
        K.qconv(gcodes, gprep, dev(np.ones(8, F32)), 1, 1, groups=2, act_bits=4, splits=2)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(SSQError, match="dense"):
        K.qconv_codes(gcodes, gprep, dev(np.ones(8, F32)), 1, 1, groups=2, act_bits=4, bad=bad,
                      out_delta=0.1, out_bits=4, splits=2)
    # nothing was launched or left behind: the unsplit result is what it was
    np.testing.assert_array_equal(run_fp32(K, L, None).view(np.int32), before.view(np.int32))
    np.testing.assert_array_equal(run_fp32(K, L, 2, workspace=torch.empty(
        need, dtype=torch.uint8, device="cuda")).view(np.int32), before.view(np.int32))
