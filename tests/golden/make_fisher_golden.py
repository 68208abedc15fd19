"""Fixtures of BRECQ's Fisher-weighted reconstruction losses, from the REFERENCE on CPU.

Like make_golden.py (whose loading recipe, tiny network and helpers it imports) this runs
only where the reference is present; what it writes is data:

  recon_brecq_fisher_diag.npz / recon_brecq_fisher_full.npz
      block_reconstruction(..., act_quant=False, opt_mode=...) on the recon_brecq setup (16
      samples of 3x16x16, batch 8, 10 iterations, b_range (20, 2), warmup 0.2): what
      recon_brecq.npz stores for its weight phase, plus the reference's cached_grads, the
      per-iteration reconstruction loss and, for the first 3 iterations, the loss pass's
      operands and results (below).
  recon_layer_fisher_diag.npz
      layer_reconstruction(..., opt_mode='fisher_diag') on the tiny net's Linear layer: the
      2-D case, stored the same way (its tensors are small: nothing is subsampled).

The loss pass of iteration k < 3 (TRUTH_ITERS): pred, tgt[idx], grad[idx], the fp32 gradient
of the reconstruction loss wrt pred (autograd of the reference's expression), and the same
loss and gradient recomputed in float64 from those fp32 operands.  Iteration 0 is stored
whole (its float64 gradient at G64_POINTS seeded positions); of iterations 1 and 2 the block
fixtures keep KEEP seeded samples of the batch (with every sample's s_n in float64, which
fisher_full's gradient needs), so that each file stays well under the committed-file limit.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fisher_golden.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as MG  # noqa: E402
from make_golden import BR, QuantModule, _Spy, _build_tiny_qnn, _dump_block, save, t2n  # noqa: E402

TRUTH_ITERS = 3
KEEP = 2
G64_POINTS = 4096


def rec_loss_expr(pred, tgt, grad, mode):
    """The reference's expressions (block_recon.py:156-162), dtype-generic."""
    if mode == "fisher_diag":
        return ((pred - tgt).pow(2) * grad.pow(2)).sum(1).mean()
    a = (pred - tgt).abs()
    g = grad.abs()
    batch_dotprod = torch.sum(a * g, (1, 2, 3)).view(-1, 1, 1, 1)
    return (batch_dotprod * a * g).mean() / 100


class _LossPassSpy:
    """Wraps a reference LossFunction.__call__: the reconstruction loss of every iteration
    and, for the first TRUTH_ITERS, the loss pass's operands, fp32 gradient and float64
    truth."""

    def __init__(self, loss_cls, mode):
        self.loss_cls, self.mode = loss_cls, mode
        self.rec32, self.passes = [], []

    def __enter__(self):
        self.orig = self.loss_cls.__call__
        spy = self

        def call(lf, pred, tgt, grad=None):
            p = pred.detach().clone().requires_grad_(True)
            with torch.enable_grad():
                l32 = rec_loss_expr(p, tgt, grad, spy.mode)
                g32, = torch.autograd.grad(l32, p)
            l32, g32 = l32.detach(), g32.detach()
            spy.rec32.append(float(l32))
            if len(spy.passes) < TRUTH_ITERS:
                p64 = pred.detach().double().requires_grad_(True)
                with torch.enable_grad():
                    l64 = rec_loss_expr(p64, tgt.double(), grad.double(), spy.mode)
                    g64, = torch.autograd.grad(l64, p64)
                spy.passes.append({"pred": pred.detach().clone(), "tgt": tgt.detach().clone(),
                                   "grad": grad.detach().clone(), "g32": g32, "g64": g64,
                                   "l32": float(l32), "l64": float(l64.detach())})
            return spy.orig(lf, pred, tgt, grad)

        self.loss_cls.__call__ = call
        return self

    def __exit__(self, *exc):
        self.loss_cls.__call__ = self.orig

    def dump(self, out, subsample):
        rng = np.random.default_rng(1005)
        out["rec_loss"] = np.array(self.rec32, np.float64)
        out["it_loss32"] = np.array([p["l32"] for p in self.passes], np.float32)
        out["it_loss64"] = np.array([p["l64"] for p in self.passes], np.float64)
        for k, p in enumerate(self.passes):
            n = p["pred"].shape[0]
            out[f"it{k}_shape"] = np.array(p["pred"].shape, np.int64)
            g64 = p["g64"].numpy().astype(np.float64)
            if p["pred"].dim() == 4:
                s = (p["pred"].double() - p["tgt"].double()).abs() * p["grad"].double().abs()
                out[f"it{k}_s64"] = s.sum((1, 2, 3)).numpy().astype(np.float64)
            if not subsample or k == 0:
                keep = np.arange(n)
            else:
                keep = np.sort(rng.choice(n, KEEP, replace=False))
            out[f"it{k}_keep"] = keep.astype(np.int64)
            for name in ("pred", "tgt", "grad", "g32"):
                out[f"it{k}_{name}"] = t2n(p[name][keep])
            if subsample and k == 0:
                at = np.sort(rng.choice(g64.size, G64_POINTS, replace=False))
                out[f"it{k}_g64_at"] = at.astype(np.int64)
                out[f"it{k}_g64"] = g64.reshape(-1)[at]
            else:
                out[f"it{k}_g64"] = g64[keep]


class _Wrap:
    """module.name replaced by a wrapper that keeps the last result."""

    def __init__(self, module, name):
        self.module, self.name, self.last = module, name, None

    def __enter__(self):
        self.orig = getattr(self.module, self.name)

        def wrapped(*a, **k):
            self.last = self.orig(*a, **k)
            return self.last

        setattr(self.module, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.module, self.name, self.orig)


def _setup(n_cali=16, res=16):
    qnn = _build_tiny_qnn()
    torch.manual_seed(1005)
    cali = torch.randn(n_cali, 3, res, res)
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:8])
    return qnn, cali


def gen_block(mode, iters=10):
    qnn, cali = _setup()
    block = qnn.model[3]
    out = {"cali": t2n(cali)}
    _dump_block(out, block)
    MG._dump_qms(out, qnn, "")
    for n in MG.CONVS:
        q = getattr(block, n).weight_quantizer
        out[n + "_delta"] = t2n(q.delta.reshape(-1))
        out[n + "_zp"] = t2n(q.zero_point.reshape(-1))
    torch.manual_seed(1005)
    with _Wrap(BR, "save_grad_data") as grads, _LossPassSpy(BR.LossFunction, mode) as lp, \
            _Spy(BR.LossFunction) as spy:
        BR.block_reconstruction(qnn, block, cali, batch_size=8, iters=iters, weight=0.01,
                                asym=True, b_range=(20, 2), warmup=0.2, act_quant=False,
                                opt_mode=mode)
    out["cached_grads"] = t2n(grads.last)
    out["w_perms"] = np.stack([p.numpy() for p in spy.perms]).astype(np.int64)
    out["w_total_loss"] = np.array([r[1] for r in spy.rec], np.float64)
    lp.dump(out, subsample=True)
    for n in MG.CONVS:
        m = getattr(block, n)
        out[n + "_alpha"] = t2n(m.weight_quantizer.alpha)
        with torch.no_grad():
            out[n + "_what_hard"] = t2n(m.weight_quantizer(m.weight))
    out["iters"] = np.array([iters])
    save("recon_brecq_" + mode, **out)


def gen_layer(mode="fisher_diag", iters=10):
    from quant import layer_recon as LR
    qnn, cali = _setup()
    layer = qnn.model[6]
    assert isinstance(layer, QuantModule) and layer.weight.dim() == 2
    out = {"cali": t2n(cali)}
    MG._dump_qms(out, qnn, "")
    torch.manual_seed(1005)
    with _Wrap(LR, "save_grad_data") as grads, _LossPassSpy(LR.LossFunction, mode) as lp, \
            _Spy(LR.LossFunction) as spy:
        LR.layer_reconstruction(qnn, layer, cali, batch_size=8, iters=iters, weight=0.01,
                                asym=True, b_range=(20, 2), warmup=0.2, act_quant=False,
                                opt_mode=mode)
    out["cached_grads"] = t2n(grads.last)
    out["w_perms"] = np.stack([p.numpy() for p in spy.perms]).astype(np.int64)
    out["w_total_loss"] = np.array([r[1] for r in spy.rec], np.float64)
    lp.dump(out, subsample=False)
    out["fc_alpha"] = t2n(layer.weight_quantizer.alpha)
    with torch.no_grad():
        out["fc_what_hard"] = t2n(layer.weight_quantizer(layer.weight))
    out["iters"] = np.array([iters])
    save("recon_layer_" + mode, **out)


if __name__ == "__main__":
    gen_block("fisher_diag")
    gen_block("fisher_full")
    gen_layer("fisher_diag")
