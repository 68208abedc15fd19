"""K34, K.epilogue_actshift: the shifted-scale act quantizer inside the K13 epilogue pass, against
the two-pass route of the same build (bit for bit) and against a restatement of the contract:
the epilogue element by element in numpy fp32 (its stated op order: the quantizer's codes and
masks depend on x's bits), then tests/actshift_ref.py / actshift_delta_ref.py with the sums in
float64.  Before the feature K.epilogue_actshift did not exist."""
import numpy as np
import pytest
import torch

import actshift_delta_ref as DR
import actshift_ref as AR

pytestmark = pytest.mark.gpu

N, C = 2, 5
TARGETS = {1: [1.0], 2: [1.0, 0.5], 4: [1.0, 0.5, 0.75, 1.25]}
DELTA, ZP, BITS, EPS = 0.1, 3.0, 4, 2.0 ** -24
# plane: 8x8 float4 items, a wave per plane; 7x7 single elements; 34x34 289 float4 items, a
# workgroup per plane; 8x8off: every activation-sized input starts one float past a 16-B boundary.
# Thinned from the full product: every value of every parameter appears.
CASES = [  # plane, residual, affine, relu, hard, S, learned delta
    ("8x8", False, False, 0, False, 1, True),
    ("8x8", True, True, 0, True, 4, False),
    ("7x7", True, True, 1, True, 2, False),
    ("7x7", True, False, 2, False, 4, True),
    ("34x34", True, True, 2, False, 4, True),
    ("34x34", False, True, 1, False, 2, False),
    ("8x8off", False, True, 2, True, 2, True),
    ("8x8off", True, True, 1, False, 2, True),
]


@pytest.fixture(scope="module")
def K():
    from shiftedscalequantization_amd import kernels
    return kernels


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def inputs(plane, S, seed):
    """Seeded conv output / residual / g and the epilogue's operands.  Channel 0's epilogue is
    the identity (bias 0, gamma 1, phi 0), so what is planted in its conv output reaches the
    quantizer as it is: both clamp edges of every grid, ties, ReLU6's edge and +-0; channel 1
    has a negative gamma; large values of either sign sit on the activations' edges."""
    H = int(plane.split("x")[0])
    gen = torch.Generator().manual_seed(seed)
    shape = (N, C, H, H)
    conv = (torch.rand(shape, generator=gen) * 1.6 - 0.3) * 2 ** BITS * DELTA
    res = torch.randn(shape, generator=gen) * 0.3
    bias, phi = torch.randn(C, generator=gen) * 0.2, torch.randn(C, generator=gen) * 0.2
    gamma = torch.rand(C, generator=gen) + 0.5
    bias[0], gamma[0], phi[0], gamma[1] = 0.0, 1.0, 0.0, -gamma[1]
    res[:, 0] = 0.0
    plant = [6.0, 0.0, -0.0, 100.0, -100.0]
    for s in TARGETS[S]:
        d = float(AR.grid(torch.tensor(DELTA), s))
        plant += [np.float32(-ZP) * np.float32(d), np.float32(2 ** BITS - 1 - ZP) * np.float32(d),
                  np.float32(2.5) * np.float32(d)]
    conv[0, 0].view(-1)[:len(plant)] = torch.tensor(plant)
    conv[1, 1].view(-1)[:2] = torch.tensor([100.0, -100.0])
    g = torch.randn(shape, generator=gen)
    alpha = torch.randn(C, S, generator=gen)
    alpha[1] = 0.0                                      # a tie: the first maximum wins
    return conv, res, g, bias, gamma, phi, AR.soft_targets(alpha)


def restatement(conv, res, g, bias, gamma, phi, relu, p, shifts, hard):
    """(y, dconv, dres, dp64, |dp| terms, (ddelta, T, M)) by the contract."""
    bc = lambda v: v.numpy().reshape(1, -1, 1, 1)
    t = conv.numpy() + bc(bias)
    if gamma is not None:
        t = t * bc(gamma) + bc(phi)
    if res is not None:
        t = t + res.numpy()
    mask = np.ones(t.shape, bool)
    if relu >= 1:
        t = np.where(t < 0, np.float32(0), t)
        mask = ~(t <= 0)
    if relu == 2:
        t = np.where(t > 6, np.float32(6), t)
        mask = ~((t <= 0) | (t >= 6))
    assert t.dtype == np.float32
    x, d, z = torch.from_numpy(t), torch.tensor(DELTA), torch.tensor(ZP)
    y = AR.forward(x, p, d, z, shifts, BITS, hard)
    dxq, _ = AR.backward(x, g, p, d, z, shifts, BITS, hard)
    gt = torch.where(torch.from_numpy(mask), dxq, torch.zeros(()))
    dconv = gt if gamma is None else gt * gamma.reshape(1, -1, 1, 1)
    dp64, mag = AR.backward64(x, g, p, d, z, shifts, BITS)
    return y, dconv, gt, dp64, mag, DR.ddelta(x, g, p, d, z, shifts, BITS, hard)


def on_device(t, off):
    """t on the device, as a leaf; off: its first element one float past a 16-B boundary."""
    if not off:
        return t.cuda().requires_grad_()
    buf = torch.empty(t.numel() + 1, device="cuda")
    buf[1:] = t.reshape(-1).cuda()
    out = buf[1:].view(t.shape).detach().requires_grad_()
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("plane,with_res,affine,relu,hard,S,learn", CASES)
def test_fused_equals_two_passes_and_the_contract(K, plane, with_res, affine, relu, hard, S, learn):
    off, shifts = plane.endswith("off"), TARGETS[S]
    conv, res, g, bias, gamma, phi, p = inputs(plane.replace("off", ""), S, seed=len(plane) + 7 * S)
    res = res if with_res else None
    gamma, phi = (gamma, phi) if affine else (None, None)
    dev = lambda t: None if t is None else t.cuda()
    zp, gd = torch.tensor(ZP).cuda(), g.cuda()
    out = {}
    for route in ("fused", "two"):
        cv, rs = on_device(conv, off), None if res is None else on_device(res, off)
        pd = p.cuda().requires_grad_()
        dl = torch.tensor(DELTA).cuda().requires_grad_(learn)
        if route == "fused":
            y = K.epilogue_actshift(cv, dev(bias), dev(gamma), dev(phi), rs, relu, pd, dl, zp,
                                    shifts, BITS, hard)
        else:
            x = K.k13(cv, dev(bias), dev(gamma), dev(phi), rs, relu, None, nonaffine_q=True,
                      lazy=False)
            y = K.actshift(x, pd, dl, zp, shifts, BITS, hard)
        y.backward(gd)
        out[route] = dict(y=y, dconv=cv.grad, dres=None if rs is None else rs.grad, dp=pd.grad,
                          ddelta=dl.grad)
    f, t = out["fused"], out["two"]
    for k in f:
        assert (f[k] is None) == (t[k] is None), k
        assert f[k] is None or torch.equal(bits(f[k]), bits(t[k])), f"{k}: fused != two passes"
    assert (f["dp"] is None) == hard and (f["ddelta"] is None) == (not learn)

    y, dconv, dres, dp64, mag, (dd, T, M) = restatement(conv, res, g, bias, gamma, phi, relu, p,
                                                        shifts, hard)
    assert torch.equal(bits(f["y"]), bits(y)) and torch.equal(bits(f["dconv"]), bits(dconv))
    assert res is None or torch.equal(bits(f["dres"]), bits(dres))
    if not hard:        # test_actshift_gpu.py's bound: the order-free fp32 one against fp64
        err = (f["dp"].cpu().double() - dp64).abs()
        print(f"dp: max err {float(err.max()):.3e}, min slack {float((conv.numel() // C * EPS * mag - err).min()):.3e}")
        assert torch.all(err <= conv.numel() // C * EPS * mag)
    if learn:           # test_actshift_delta_gpu.py's bound
        err = abs(float(f["ddelta"].double().cpu()) - float(dd))
        bound = EPS * abs(float(dd)) + (M + 8) * 2.0 ** -53 * float(T)
        print(f"ddelta {float(f['ddelta']):.9g} ref {float(dd):.17g} err {err:.3e} bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("what,kw", [("shift targets", dict(S=5)), ("activation code", dict(relu=3)),
                                     ("two passes", dict(learn_bias=True)),
                                     ("residual shape", dict(bad_res=True))])
def test_refusals(K, what, kw):
    S = kw.get("S", 2)
    shifts = [1.0, 0.5, 0.75, 1.25, 1.5][:S]
    conv = torch.zeros(N, C, 4, 4, device="cuda")
    bias = torch.zeros(C, device="cuda", requires_grad=kw.get("learn_bias", False))
    res = torch.zeros(N, C, 2, 2, device="cuda") if kw.get("bad_res") else None
    with pytest.raises(K.A.SSQError, match=what):
        K.epilogue_actshift(conv, bias, None, None, res, kw.get("relu", 1),
                            torch.zeros(C, S, device="cuda"), torch.tensor(DELTA).cuda(),
                            torch.tensor(ZP).cuda(), shifts, BITS)
