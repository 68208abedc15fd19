"""Integer inference of per-(co, ci) scaled weights on the device (ssq_qweight_prepare_perci,
ssq_qweight_prepare_grouped_perci, the centred K23 / K26 kernels).  Codes, zero points and shift
targets are drawn directly; the stored scale fp32(delta[co] * fp32(target)) goes through
kernels.perci_grid, and y.view(int32) must EQUAL the host int64 reference fp32(I) * s[co],
I = sum (q_a - z_a)(q_w - z_w[co]) k[co, ci], s[co] = fp32(fp32(delta_a * base[co]) / fp32(L)).
Shapes: batch 2 on a 9x7 plane (M = 126, no tile multiple); 3x3 at stride 1 and 2 with Ci = 70
(padded to 80: a K tail, two channel tiles of the activation) and Co = 72 (crosses the 64 tile);
1x1 with Ci = 16 (a single k step); a Linear 100 -> 10 (the scale is per element); grouped g = 3.
Weights W2 on the default shift targets (L = 32), activations at 4 and 8 bits, symmetric and
not.  Then the 9 * 2^-24 bound against the decoded path's fp64 convolution and the prepare
kernel's count of the elements that leave int8."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_qinfer_host import qrange
from test_qinfer_perci_host import (SHIFT, grid_scale, operand_sum, perci_operand, predicate,
                                    ref_output)

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def host(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def parity_log(rec):
    """Print the figure and append it to $SSQ_PARITY_LOG (jsonl) when set."""
    print(json.dumps(rec))
    path = os.environ.get("SSQ_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


# (N, C, H, W, Co, R, stride, pad, groups); H = None: a linear (N, C) -> (N, Co)
SHAPES = {
    "3x3_s1": (2, 70, 9, 7, 72, 3, 1, 1, 1),
    "3x3_s2": (2, 70, 9, 7, 72, 3, 2, 1, 1),
    "1x1": (2, 16, 9, 7, 72, 1, 1, 0, 1),
    "linear": (5, 100, None, None, 10, 1, 1, 0, 1),
    "g3": (2, 24, 9, 7, 72, 3, 1, 1, 3),
}
ACTS = [(4, False), (4, True), (8, False), (8, True)]           # (n_bits_a, sym)
CASES = [(n, a) for n in SHAPES for a in ACTS]


def draw_perci_weight(rng, ws, wb, targets=SHIFT):
    """Codes over the whole range, asymmetric per-channel zero points inside it, a shift target
    per (co, ci) -> (qw, zw, scale[co, ci] = fp32(delta[co] * fp32(target)))."""
    whi = 2 ** wb - 1
    qw = rng.integers(0, whi + 1, ws)
    zw = rng.integers(0, whi + 1, ws[0])
    zw[0], zw[-1] = 0, whi
    t = np.array(targets, F32)
    delta = rng.uniform(1e-3, 2e-2, ws[0]).astype(F32)
    scale = delta[:, None] * t[rng.integers(0, len(t), (ws[0], ws[1]))]
    assert scale.dtype == F32
    return qw, zw, scale


def encode_perci(K, qw, zw, scale, wb):
    """Integer codes -> W_hat = (q - zp) * scale[co, ci] -> the export's packed codes."""
    what = (qw - zw.reshape(-1, 1, 1, 1)).astype(F32) * scale.reshape(scale.shape + (1, 1))
    assert what.dtype == F32
    packed, bad = K.pack_encode(dev(what), dev(zw), dev(scale.reshape(-1)), True, None, wb, 0,
                                2 ** wb - 1)
    assert bad == 0
    return what, packed


@functools.lru_cache(maxsize=None)
def run_case(name, aform):
    """Device output and host references of one case, computed once for the bit-exact and the
    bound tests."""
    from shiftedscalequantization_amd import kernels as K
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES[name]
    ab, asym = aform
    linear = H is None
    rng = np.random.default_rng(zlib.crc32(repr((name, aform)).encode()))
    alo, ahi = qrange(ab, asym)
    xs = (N, Cc, 1, 1) if linear else (N, Cc, H, W)
    qa = rng.integers(alo, ahi + 1, xs)
    za = int(rng.integers(alo, ahi + 1))
    qw, zw, wscale = draw_perci_weight(rng, (Co, Cc // G, R, R), 2)
    L, base, k = K.perci_grid(torch.from_numpy(wscale), Co, Cc // G, 127)
    assert L == 32 and not K.perci_plain((L, base, k))
    predicate(wscale, L, base, k, 127)
    m = perci_operand(qw, zw, k.numpy())
    assert np.abs(m).max() <= 127
    da = F32(rng.uniform(0.01, 0.2))
    xhat = (qa - za).astype(F32) * da
    what, packed = encode_perci(K, qw, zw, wscale, 2)
    wshape = (Co, Cc) if linear else qw.shape
    prep = K.qweight_prepare(packed, wshape, dev(zw), 2, 0, groups=G, kfac=k)
    assert prep.centred and not prep.wide and int(prep.bad.item()) == 0
    scale = grid_scale(da, base.numpy(), L)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    x = dev(xhat.reshape(N, Cc) if linear else xhat)
    y = K.qconv(x, prep, dev(scale), stride, pad, groups=G, act_zp=float(za), act_bits=ab,
                act_sym=asym, act_delta=float(da), bad=bad)
    ref = ref_output(operand_sum(qa, za, m, stride, pad, G), scale)
    xt, wt = torch.from_numpy(xhat).double(), torch.from_numpy(what).double()
    ref64 = F.conv2d(xt, wt, stride=stride, padding=pad, groups=G).numpy()
    A = F.conv2d(xt.abs(), wt.abs(), stride=stride, padding=pad, groups=G).numpy()
    out = host(y)
    assert out.shape == ((N, Co) if linear else ref.shape)
    return out.reshape(ref.shape), ref, ref64, A, int(bad.item())


@pytest.mark.parametrize("name,aform", CASES)
def test_perci_bit_exact(K, name, aform):
    out, ref, _, _, bad = run_case(name, aform)
    assert bad == 0
    assert ref.any()
    np.testing.assert_array_equal(out.view(np.int32), ref.view(np.int32))


@pytest.mark.parametrize("name", list(SHAPES))
def test_perci_within_fp32_bound_of_decoded_path(K, name):
    """|y - conv64(x_hat, W_hat)| <= 9 * 2^-24 * conv64(|x_hat|, |W_hat|) elementwise: one
    rounding in x_hat, one in (q - z) * d1, two between d1 and base * k / L (k / L and the
    product), four in the integer epilogue (fp32(I), delta_a * base, / L, the product); the ninth
    unit covers the second-order terms."""
    worst = 0.0
    for n, aform in CASES:
        if n != name:
            continue
        out, _, ref64, A, _ = run_case(n, aform)
        err = np.abs(out.astype(np.float64) - ref64)
        nz = A > 0
        ratio = float((err[nz] / A[nz]).max()) if nz.any() else 0.0
        print({"case": (n, aform), "err_over_A_in_2^-24": ratio * 2 ** 24})
        assert np.all(err <= 9 * 2.0 ** -24 * A), (n, aform, ratio * 2 ** 24)
        worst = max(worst, ratio)
    parity_log({"test": "perci_qconv_vs_fp64", "shape": name,
                "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 9.0})


def test_cases_cover_the_forms():
    assert {n for n, _ in CASES} == set(SHAPES) and {a for _, a in CASES} == set(ACTS)
    assert 3 * 33 <= 127 < 7 * 33      # W2 on the default targets fits int8, W3 does not


@pytest.mark.parametrize("name", ["3x3_s1", "linear", "g3"])
def test_prepare_counts_elements_that_leave_int8(K, name):
    """W4 on the default targets: (q - z) * k reaches 15 * 33 = 495; the prepare counts exactly
    the real elements with |m| > 127, and none when the same codes meet factors of at most 8."""
    N, Cc, H, W, Co, R, stride, pad, G = SHAPES[name]
    rng = np.random.default_rng(17)
    ws = (Co, Cc // G, R, R)
    qw, zw, wscale = draw_perci_weight(rng, ws, 4)
    L, base, k = K.perci_grid(torch.from_numpy(wscale), Co, Cc // G, 127)
    over = int((np.abs(perci_operand(qw, zw, k.numpy())) > 127).sum())
    assert L == 32 and over > 0
    _, packed = encode_perci(K, qw, zw, wscale, 4)
    wshape = (Co, Cc) if H is None else ws
    prep = K.qweight_prepare(packed, wshape, dev(zw), 4, 0, groups=G, kfac=k)
    assert int(prep.bad.item()) == over
    k8 = torch.clamp(k - 25, 1, 8)
    assert np.abs(perci_operand(qw, zw, k8.numpy())).max() <= 127
    prep = K.qweight_prepare(packed, wshape, dev(zw), 4, 0, groups=G, kfac=k8)
    assert int(prep.bad.item()) == 0
    # a zero point that is no integer code is still counted, once per channel
    prep = K.qweight_prepare(packed, wshape, dev(zw + 0.5), 4, 0, groups=G, kfac=k8)
    assert int(prep.bad.item()) >= Co


def test_wrapper_refuses_bad_kfac(K):
    from shiftedscalequantization_amd._capi import SSQError
    packed = torch.zeros(64, dtype=torch.uint8, device="cuda")
    zp = torch.zeros(4, device="cuda")
    for kfac in (torch.ones(31, dtype=torch.int32), torch.zeros(32, dtype=torch.int32),
                 torch.full((32,), 128, dtype=torch.int32), torch.ones(32)):
        with pytest.raises(SSQError, match="kfac"):
            K.qweight_prepare(packed, (4, 8, 1, 1), zp, 4, 0, kfac=kfac)
    with pytest.raises(SSQError, match="do not go together"):
        K.qweight_prepare(packed, (4, 8, 1, 1), zp, 4, 0, kfac=torch.ones(32, dtype=torch.int32),
                          kcol=torch.ones(8, dtype=torch.int32))
    with pytest.raises(SSQError, match="depthwise"):
        K.qweight_prepare(packed, (4, 1, 3, 3), zp, 4, 0, groups=4,
                          kfac=torch.ones(4, dtype=torch.int32))
