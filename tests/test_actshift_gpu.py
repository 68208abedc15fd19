"""K33 (ssq_actshift_fwd / _bwd / _init) against the contract in tests/actshift_ref.py.

y (soft and hard) and dx are bit-equal to the fp32 reference (NaN where it has NaN); dp and
the init sums are held to the order-free fp32 summation bound M * 2^-24 * sum|term| against
the fp64 reference (M = N*H*W) on the finite inputs; the backward gives the same bits twice;
init_v's alpha equals the reference's, with every channel's argmin checked to be decided."""
import functools

import numpy as np
import pytest
import torch

import actshift_ref as AR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (3, 5, 7, 7), (2, 70, 8, 8), (4, 6), (2, 3, 1, 33)]
SHIFTS = [1.0, 0.5, 0.75, 0.25]
DELTA = 0.1
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def K():
    from shiftedscalequantization_amd import kernels
    assert torch.cuda.is_available()
    return kernels


@functools.lru_cache(maxsize=None)
def case(shape, S, n_bits, z):
    """Inputs and CPU references of one case, computed once: exact ties (k + 0.5) * d_i,
    negatives, values beyond both clamp edges, +-0 and (x only) a few NaN / +-inf."""
    seed = hash((shape, S, n_bits, z)) & 0xffff
    g = torch.Generator().manual_seed(seed)
    n = 2 ** n_bits
    shifts = SHIFTS[:S]
    delta = torch.tensor(DELTA, dtype=torch.float32)
    zp = torch.tensor(float(z), dtype=torch.float32)
    numel = int(np.prod(shape))
    # centred on the grid's middle, wide enough to cross both edges of every candidate
    x = ((torch.rand(numel, generator=g) * 1.6 - 0.3) * n - z) * DELTA
    pos = torch.randperm(numel, generator=g)
    if numel < 8:
        # one element: the s = 1 grid's lowest code exactly (error 0), which every finer grid
        # clamps short of (z = 3), so init's argmin is decided
        x[0] = -z * DELTA
    for j in range(numel // 4 if numel >= 8 else 0):
        i = j % S
        k = int(torch.randint(0, n - 1, (1,), generator=g))
        x[pos[j]] = (torch.tensor(k - z + 0.5) * AR.grid(delta, shifts[i])).float()
    if numel >= 8:
        x[pos[-1]], x[pos[-2]] = 0.0, -0.0
        x[pos[-3]] = -1.0e-3
    xf = x.reshape(shape).clone()                       # the finite input
    if numel >= 8:
        x[pos[-4]], x[pos[-5]], x[pos[-6]] = float("nan"), float("inf"), float("-inf")
    x = x.reshape(shape)
    gy = torch.randn(shape, generator=g)
    C = shape[1]
    alpha = torch.randn(C, S, generator=g)
    if C >= 2:
        alpha[1] = 0.0                                   # a tie: the first maximum wins
    p = AR.soft_targets(alpha)
    ref = {}
    for hard in (False, True):
        ref["y", hard] = AR.forward(x, p, delta, zp, shifts, n_bits, hard)
        ref["dx", hard], _ = AR.backward(x, gy, p, delta, zp, shifts, n_bits, hard)
    ref["dp64"], ref["mag"] = AR.backward64(xf, gy, p, delta, zp, shifts, n_bits)
    ref["dxf"], _ = AR.backward(xf, gy, p, delta, zp, shifts, n_bits, False)
    ref["mse64"] = AR.init_mse64(xf, delta, zp, shifts, n_bits)
    return dict(x=x, xf=xf, gy=gy, p=p, delta=delta, zp=zp, shifts=shifts, ref=ref,
                M=numel // C)


def same_bits(a, b, what):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    assert a.shape == b.shape, what
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"{what}: NaN pattern differs"
    ok = (a.view(np.int32) == b.view(np.int32)) | na
    assert ok.all(), f"{what}: {int((~ok).sum())} of {a.size} elements differ"


@pytest.mark.parametrize("z", [0, 3])
@pytest.mark.parametrize("n_bits", [2, 4, 8])
@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_the_contract(K, shape, S, n_bits, z):
    c = case(shape, S, n_bits, z)
    dev = lambda t: t.cuda()
    x, xf, gy, p, d, zp = (dev(c[k]) for k in ("x", "xf", "gy", "p", "delta", "zp"))
    sh, ref = c["shifts"], c["ref"]
    for hard in (False, True):
        y = K.actshift_fwd(x, p, d, zp, sh, n_bits, hard)
        same_bits(y, ref["y", hard], f"y hard={hard}")
        dx, dp = K.actshift_bwd(x, gy, p, d, zp, sh, n_bits, hard)
        same_bits(dx, ref["dx", hard], f"dx hard={hard}")
        if hard:
            assert not dp.any(), "hard backward: dp must be zero"
            dx0, none = K.actshift_bwd(x, gy, p, d, zp, sh, n_bits, True, want_dp=False)
            assert none is None
            same_bits(dx0, ref["dx", True], "dx hard, dp not asked for")
    # the channel sums on the finite input: the order-free fp32 bound against fp64
    dx, dp = K.actshift_bwd(xf, gy, p, d, zp, sh, n_bits, False)
    same_bits(dx, ref["dxf"], "dx (finite input)")
    err = (dp.cpu().double() - ref["dp64"]).abs()
    bound = c["M"] * EPS * ref["mag"]
    print(f"dp: max err {float(err.max()):.3e}, min slack {float((bound - err).min()):.3e}")
    assert torch.all(err <= bound), (float(err.max()), float(bound.min()))
    dx2, dp2 = K.actshift_bwd(xf, gy, p, d, zp, sh, n_bits, False)
    assert torch.equal(dx, dx2) and torch.equal(dp.view(torch.int32), dp2.view(torch.int32))
    mse = K.actshift_init(xf, d, zp, sh, n_bits)
    err = (mse.cpu().double() - ref["mse64"]).abs()
    print(f"mse: max err {float(err.max()):.3e}")
    assert torch.all(err <= c["M"] * EPS * ref["mse64"])
    assert torch.equal(mse, K.actshift_init(xf, d, zp, sh, n_bits))


@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_init_v_alpha_equals_the_reference(K, shape, S):
    """Every channel's argmin is decided in the fp64 reference (best two errors further than
    1e-4 relative apart), so the kernel's sums must pick the same shift: alpha is equal."""
    from shiftedscalequantization_amd import quant as Q
    c = case(shape, S, 4, 3)
    m64 = c["ref"]["mse64"]
    if S > 1:
        top2 = torch.sort(m64, dim=-1).values[:, :2]
        gap = (top2[:, 1] - top2[:, 0]) / top2[:, 1]
        assert torch.all(gap > 1e-4), f"undecided channel in the test's own input: {gap.min()}"
    uaq = Q.UniformAffineQuantizer(n_bits=4, channel_wise=False, scale_method="mse", leaf_param=True)
    uaq.delta = torch.nn.Parameter(c["delta"].cuda())
    uaq.zero_point = torch.nn.Parameter(c["zp"].cuda())
    uaq.inited = True
    q = Q.ChannelQuantAct(uaq=uaq, shiftTarget=list(c["shifts"]))
    q.init_v(c["xf"].cuda())
    C = shape[1]
    assert isinstance(q.alpha, torch.nn.Parameter) and q.alpha.shape == (C, S)
    assert q.opt_mode == "shiftFeature" and q.inited
    want = AR.init_alpha(m64.float().cuda())
    assert torch.equal(q.alpha.detach(), want)
    assert torch.equal(torch.argmin(m64, -1), torch.argmin(K.actshift_init(
        c["xf"].cuda(), uaq.delta, uaq.zero_point, c["shifts"], 4).cpu(), -1))
    # get_delta: fp32(delta * s_k) per channel
    k = torch.argmax(AR.soft_targets(want.cpu()), -1)
    dk = torch.stack([AR.grid(c["delta"], c["shifts"][int(i)]) for i in k]).view(1, C, 1, 1)
    assert q.get_delta().shape == (1, C, 1, 1) and torch.equal(q.get_delta().cpu(), dk)


def test_quantizer_forward_backward_through_autograd(K):
    """ChannelQuantAct 'shiftFeature' end to end: alpha's gradient is dp pushed through the
    softmax by autograd, x gets the clamp-masked straight-through gradient, and the hard
    quantizer equals the per-channel 'none'-mode selection bit for bit."""
    from shiftedscalequantization_amd import quant as Q
    c = case((3, 5, 7, 7), 2, 4, 3)
    uaq = Q.UniformAffineQuantizer(n_bits=4, channel_wise=False, scale_method="mse", leaf_param=True)
    uaq.delta = torch.nn.Parameter(c["delta"].cuda())
    uaq.zero_point = torch.nn.Parameter(c["zp"].cuda())
    uaq.inited = True
    q = Q.ChannelQuantAct(uaq=uaq, shiftTarget=[1.0, 0.5])
    q.init_v(c["xf"].cuda())
    x = c["xf"].cuda().requires_grad_(True)
    y = q(x)
    y.backward(c["gy"].cuda())
    # the reference on the probabilities the device's softmax produced
    p = q.get_sig_soft_targets()
    pc = p.detach().cpu()
    same_bits(y, AR.forward(c["xf"], pc, c["delta"], c["zp"], [1.0, 0.5], 4), "soft y")
    dxr, _ = AR.backward(c["xf"], c["gy"], pc, c["delta"], c["zp"], [1.0, 0.5], 4)
    same_bits(x.grad, dxr, "dx")
    # alpha's gradient: the fp64 dp through the same softmax Jacobian; |dp_i/dalpha_j| <=
    # (zeta - gamma) / 4 < 1, so the dp bound (plus its rounding to fp32) summed over i holds
    dp64, mag = AR.backward64(c["xf"], c["gy"], pc, c["delta"], c["zp"], [1.0, 0.5], 4)
    want, = torch.autograd.grad(p, q.alpha, dp64.float().cuda())
    tol = ((c["M"] + 1) * EPS * mag).sum(-1, keepdim=True).float() + 1e-12
    assert torch.all((q.alpha.grad - want).abs().cpu() <= tol)
    assert uaq.delta.grad is None and uaq.zero_point.grad is None
    q.hard_targets = True
    yh = q(c["xf"].cuda())
    k = q.shift_index().cpu()
    for ch in range(5):
        q1 = Q.ChannelQuantAct(uaq=uaq, shiftTarget=[1.0, 0.5])
        q1.shiftedScale = [1.0, 0.5][int(k[ch])]
        same_bits(yh[:, ch], q1(c["xf"].cuda())[:, ch], f"hard channel {ch}")
