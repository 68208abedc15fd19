"""The delta gradient of the shifted-scale activation quantizer (ssq_actshift_bwd_delta, DESIGN.md
section 6) in plain torch, with candidates, codes and masks made as tests/actshift_ref.py makes
them (in x's dtype; fp32 is the contract):

  d_i = fp32(delta * s_i);  v_i = round(x / d_i) + z;  c_i = clamp(v_i, 0, n-1);  in_i = [0 <= v_i <= n-1]
  soft   ddelta = sum g * p[c,i] * s_i * ((c_i - z) - in_i * x / d_i)   over n, c, hw and i
  hard   ddelta = sum g * s_k * ((c_k - z) - in_k * x / d_k),  k = first argmax_i p[c,i]

Every term is worked in float64 from those values, x / d_i included, and summed in float64.
"""
import torch

import actshift_ref as AR


def terms(x, g, p, delta, zp, shifts, n_bits, hard=False):
    """The float64 terms: (S, *x.shape) soft, (1, *x.shape) hard."""
    z = zp.detach().reshape(()).to(x.dtype)
    hi = float(2 ** n_bits - 1)
    xd, out = x.double(), []
    for s in shifts:
        d = AR.grid(delta, s, x.dtype)
        v = torch.round(x / d) + z
        c, inside = torch.clamp(v, 0, hi), ((v >= 0) & (v <= hi)).to(x.dtype)
        t = (c.double() - z.double()) - inside.double() * (xd / d.double())
        out.append(torch.tensor(float(s), dtype=torch.float32).double().to(x.device) * t)
    if hard:
        k = AR._bc(torch.argmax(p, dim=-1), x)
        t = out[0]
        for i in range(1, len(shifts)):
            t = torch.where(k == i, out[i], t)
        return (g.double() * t).unsqueeze(0)
    return torch.stack([g.double() * (AR._bc(p[:, i], x).double() * out[i])
                        for i in range(len(shifts))])


def ddelta(x, g, p, delta, zp, shifts, n_bits, hard=False):
    """(ddelta, T = sum of |term|, M = number of terms), the first two as float64 scalars."""
    t = terms(x, g, p, delta, zp, shifts, n_bits, hard)
    return t.sum(), t.abs().sum(), t.numel()


class ActShiftDeltaRef(torch.autograd.Function):
    """AR.ActShiftRef with delta's gradient: the contract as an autograd Function of torch ops."""

    @staticmethod
    def forward(ctx, x, p, delta, zp, shifts, n_bits, hard):
        ctx.save_for_backward(x, p, delta, zp)
        ctx.cfg = (shifts, n_bits, hard)
        return AR.forward(x, p.to(x.dtype), delta, zp, shifts, n_bits, hard)

    @staticmethod
    def backward(ctx, g):
        x, p, delta, zp = ctx.saved_tensors
        shifts, n_bits, hard = ctx.cfg
        dx, dp = AR.backward(x, g, p.to(x.dtype), delta, zp, shifts, n_bits, hard)
        dd = ddelta(x, g, p.to(x.dtype), delta, zp, shifts, n_bits, hard)[0]
        return dx, dp.to(p.dtype), dd.to(delta.dtype).reshape(delta.shape), None, None, None, None


class RefActQuant(torch.nn.Module):
    """ChannelQuantAct 'shiftFeature' with a learned delta: alpha (C, S) and delta are parameters."""

    def __init__(self, delta, zp, shifts, n_bits, alpha):
        super().__init__()
        self.zero_point = zp.detach().clone()
        self.shifts, self.n_bits = tuple(float(s) for s in shifts), int(n_bits)
        self.alpha = torch.nn.Parameter(alpha.detach().clone())
        self.delta = torch.nn.Parameter(delta.detach().clone())

    def forward(self, x):
        return ActShiftDeltaRef.apply(x, AR.soft_targets(self.alpha), self.delta, self.zero_point,
                                      self.shifts, self.n_bits, False)
