"""ssq_actshift_bwd_delta (K33's backward with the delta gradient) against the contract in
tests/actshift_delta_ref.py, through autograd, and in block_recon_fused_shiftedScale(act=True,
act_shift_learn_delta=True).  Before the feature the entry point did not exist."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import actshift_delta_ref as DR
import actshift_ref as AR

pytestmark = pytest.mark.gpu

# scalar / float4 path x plane per wave / per workgroup (above 256 work items), and 2-D
SHAPES = [(2, 3, 7, 7), (2, 5, 8, 8), (1, 2, 40, 40), (3, 2, 33, 33), (4, 6)]
TARGETS = {1: [1.0], 2: [1.0, 0.5], 4: [1.0, 0.5, 0.75, 1.25]}
DELTA, ZP = 0.1, 3


@pytest.fixture(scope="module")
def K():
    from shiftedscalequantization_amd import kernels
    return kernels


@functools.lru_cache(maxsize=None)
def case(shape, S, n_bits):
    """x across both clamps with exact ties (k + 0.5) * d_i and zeros, random g, a p row with a
    tie; the float64 reference of both forms, computed once."""
    gen = torch.Generator().manual_seed(hash((shape, S, n_bits)) & 0xffff)
    n, shifts, numel = 2 ** n_bits, TARGETS[S], int(np.prod(shape))
    delta, zp = torch.tensor(DELTA), torch.tensor(float(ZP))
    x = ((torch.rand(numel, generator=gen) * 1.6 - 0.3) * n - ZP) * DELTA
    pos = torch.randperm(numel, generator=gen)
    for j in range(numel // 4):
        k = int(torch.randint(0, n - 1, (1,), generator=gen))
        x[pos[j]] = (torch.tensor(k - ZP + 0.5) * AR.grid(delta, shifts[j % S])).float()
    x[pos[-1]], x[pos[-2]] = 0.0, -0.0
    x = x.reshape(shape)
    assert x.min() < -ZP * DELTA and x.max() > (n - 1 - ZP) * DELTA * max(shifts)
    g = torch.randn(shape, generator=gen)
    alpha = torch.randn(shape[1], S, generator=gen)
    alpha[1] = 0.0
    p = AR.soft_targets(alpha)
    ref = {hard: DR.ddelta(x, g, p, delta, zp, shifts, n_bits, hard) for hard in (False, True)}
    return dict(x=x, g=g, p=p, delta=delta, zp=zp, shifts=shifts, ref=ref)


def bits(t):
    return t.detach().cpu().view(torch.int32)


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("n_bits", [4, 8])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ddelta_matches_the_contract(K, shape, S, n_bits, hard):
    c = case(shape, S, n_bits)
    x, g, p, d, zp = (c[k].cuda() for k in ("x", "g", "p", "delta", "zp"))
    dx0, dp0 = K.actshift_bwd(x, g, p, d, zp, c["shifts"], n_bits, hard)
    dx, dp, dd = K.actshift_bwd_delta(x, g, p, d, zp, c["shifts"], n_bits, hard)
    assert torch.equal(bits(dx), bits(dx0)) and torch.equal(bits(dp), bits(dp0))
    dx2, dp2, dd2 = K.actshift_bwd_delta(x, g, p, d, zp, c["shifts"], n_bits, hard)
    assert torch.equal(bits(dd), bits(dd2)) and torch.equal(bits(dx), bits(dx2))
    want, T, M = c["ref"][hard]
    err = abs(float(dd.double().cpu()) - float(want))
    # one fp32 rounding of the result, eight double roundings per term (the kernel states five,
    # the reference makes three of its own) and at most M for the sum
    bound = 2.0 ** -24 * abs(float(want)) + (M + 8) * 2.0 ** -53 * float(T)
    print(f"ddelta {float(dd):.9g} ref {float(want):.17g} err {err:.3e} bound {bound:.3e}")
    assert dd.shape == () and err <= bound


def test_autograd_reaches_delta_only_when_asked(K):
    c = case((2, 5, 8, 8), 2, 4)
    g, zp = c["g"].cuda(), c["zp"].cuda()
    grads = {}
    for learn in (True, False):
        x, p = c["x"].cuda().requires_grad_(), c["p"].cuda().requires_grad_()
        d = c["delta"].cuda().reshape(1).requires_grad_(learn)
        K.actshift(x, p, d, zp, c["shifts"], 4).backward(g)
        grads[learn] = (x.grad, p.grad, d.grad)
    _, _, dd = K.actshift_bwd_delta(c["x"].cuda(), g, c["p"].cuda(), c["delta"].cuda(), zp,
                                    c["shifts"], 4)
    assert grads[True][2].shape == (1,) and torch.equal(bits(grads[True][2]), bits(dd.reshape(1)))
    assert grads[False][2] is None
    for a, b in zip(grads[True][:2], grads[False][:2]):
        assert torch.equal(bits(a), bits(b))


def _cpu_loop(R, block, start, dtype, iters, batch, lr_delta, bump=False):
    """The loop restated on the CPU: Adam(1e-3) on the alphas, Adam(lr_delta) with cosine
    annealing to 0 on the deltas, over the loop's draws.  bump: conv1's start delta one ulp up."""
    with torch.no_grad():
        w1, w2 = (m.weight_quantizer(m.weight).detach().cpu().to(dtype) for m in (block.conv1, block.conv2))
        b1, b2 = (None if m.bias is None else m.bias.detach().cpu().to(dtype)
                  for m in (block.conv1, block.conv2))

    def fwd(x, aq1, aq2):      # BN folded: conv + bias, ReLU, act quantizer, conv + residual, ...
        h = aq1(F.relu(F.conv2d(x, w1, b1, padding=1)))
        return aq2(F.relu(F.conv2d(h, w2, b2, padding=1) + x))
    inp = torch.cat(block.cached_inp_features).cpu().to(dtype)
    tgt = torch.cat(block.cached_out_features).cpu().to(dtype)
    aq = {}
    for name, old in (("conv1", block.conv1.act_quantizer), ("block", block.act_quantizer)):
        d0 = start[name, "delta"].cpu()
        if bump and name == "conv1":
            d0 = torch.nextafter(d0, torch.full_like(d0, float("inf")))
        aq[name] = DR.RefActQuant(d0.to(dtype), old.zero_point.cpu(), R.SHIFTS, old.n_bits,
                                  start[name, "alpha"].cpu().to(dtype))
    opt = torch.optim.Adam([q.alpha for q in aq.values()], lr=1e-3)
    opt_d = torch.optim.Adam([q.delta for q in aq.values()], lr=lr_delta)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt_d, T_max=iters, eta_min=0.)
    torch.manual_seed(1005)
    for _ in range(iters):
        idx = torch.randperm(inp.shape[0])[:batch]
        opt.zero_grad()
        opt_d.zero_grad()
        (fwd(inp[idx], aq["conv1"], aq["block"]) - tgt[idx]).abs().pow(2.0).sum(1).mean().backward()
        opt.step()
        opt_d.step()
        sched.step()
    return {(n, k): getattr(q, k).detach().double() for n, q in aq.items() for k in ("alpha", "delta")}


def _block8(R):
    """test_actshift_recon_gpu's block with 8 cached samples."""
    qnn, block, cali = R.make()
    block.cached_inp_features = [torch.cat(block.cached_inp_features)[:8]]
    block.cached_out_features = [torch.cat(block.cached_out_features)[:8]]
    return qnn, block


def _run(Q, qnn, block, start=None, **kw):
    def hook(i):
        if start is not None and i == 0:
            for n, q in (("conv1", block.conv1.act_quantizer), ("block", block.act_quantizer)):
                start[n, "alpha"], start[n, "delta"] = q.alpha.detach().clone(), q.delta.detach().clone()
    torch.manual_seed(1005)
    return Q.block_recon_fused_shiftedScale(block, iters=6, model=qnn, act=True, batch_size=4,
                                            verbose=False, iter_hook=hook, **kw)


def test_loop_learns_delta_with_the_shifts():
    """6 iterations on a QuantBasicBlock (8 channels, 8x8 planes, 8 cached samples, batch 4).
    Alphas: test_actshift_recon_gpu's rule, within 4x the fp32 CPU restatement's drift from its
    fp64 version.  Deltas: that rule does not carry over to a scalar whose six Adam steps are
    about lr * sign(g) each (the fp32 and fp64 restatements can agree to the last bit), so the
    bound is twice the restatement's own drift under a one-ulp perturbation of conv1's start
    delta, and at least one ulp of delta; both figures are in the log line."""
    import test_actshift_recon_gpu as R
    from shiftedscalequantization_amd import quant as Q
    lr = 4e-5
    qnn, block = _block8(R)
    start = {}
    res = _run(Q, qnn, block, start, act_shift_learn_delta=True)
    assert len(res) == 2 and all(np.isfinite(v) for v in res)
    qs = {"conv1": block.conv1.act_quantizer, "block": block.act_quantizer}
    got = {(n, k): getattr(q, k).detach().double().cpu() for n, q in qs.items() for k in ("alpha", "delta")}
    assert all(q.delta.grad is None and not q.learn_delta and q.hard_targets for q in qs.values())
    r32 = _cpu_loop(R, block, start, torch.float32, 6, 4, lr)
    r64 = _cpu_loop(R, block, start, torch.float64, 6, 4, lr)
    rup = _cpu_loop(R, block, start, torch.float32, 6, 4, lr, bump=True)
    worst = lambda a, b, k: max(float((a[n, k] - b[n, k]).abs().max()) for n in qs)
    drift_a, err_a = worst(r32, r64, "alpha"), worst(got, r32, "alpha")
    ulp = max(float(torch.finfo(torch.float32).eps * start[n, "delta"].abs().max()) for n in qs)
    drift_d = max(worst(r32, rup, "delta"), ulp)
    err_d = worst(got, r32, "delta")
    moved = max(float((got[n, "delta"] - start[n, "delta"].double().cpu()).abs().max()) for n in qs)
    R.log_parity({"test": "actshift_loop_delta", "iters": 6, "alpha_drift": drift_a, "alpha_err": err_a,
                  "delta_one_ulp_drift": drift_d, "delta_tolerance": 2 * drift_d, "delta_err": err_d,
                  "delta_moved": moved})
    assert moved > lr                          # Adam stepped the deltas: six steps of about lr
    assert err_a <= 4 * drift_a, (err_a, drift_a)
    assert err_d <= 2 * drift_d, (err_d, drift_d)
    # the export reads the learned delta
    block.clear_cached_features()
    tensors, _ = Q.export_quantized(qnn)
    assert torch.equal(tensors["model.3.act_delta"].reshape(-1), block.act_quantizer.delta.detach().reshape(-1))

    # flag off: the deltas keep their bits and the result is the default call's
    out = []
    for kw in ({}, {"act_shift_learn_delta": False}):
        qnn, block = _block8(R)
        before = [block.conv1.act_quantizer.delta.detach().clone(), block.act_quantizer.delta.detach().clone()]
        out.append(_run(Q, qnn, block, **kw))
        after = [block.conv1.act_quantizer.delta, block.act_quantizer.delta]
        assert all(torch.equal(bits(a), bits(b)) and b.grad is None for a, b in zip(before, after))
    assert out[0] == out[1]
