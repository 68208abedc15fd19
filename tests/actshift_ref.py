"""The shifted-scale activation contract in plain torch.

No reference run can pin ChannelQuantAct's 'shiftFeature' mode (the reference's own code for
it never ran), so this file is the specification the kernels are held to:

  candidates   Q_i(x) = (clamp(round(x / d_i) + z, 0, n-1) - z) * d_i,  d_i = fp32(delta * s_i)
               in_i(x) = 1 where 0 <= round(x / d_i) + z <= n-1, else 0
  soft         y = Q_0*p[c,0]; y = y + Q_i*p[c,i]        (every product and sum rounded)
  hard         y = Q_k, k = first argmax_i p[c,i]
  backward     soft: dx = g * m, m = ((+0 + p[c,0]*in_0) + p[c,1]*in_1) + ...
                     dp[c,i] = sum_{n,h,w} g * Q_i
               hard: dx = g * in_k, dp = 0
  init         mse[c,i] = sum_{n,h,w} (x - Q_i)^2 -> ChannelQuant.init_alpha's table

Three forms: the fp32 eager one (the stated operation order), the fp64 one (the same
candidates -- they are the contract's fp32 values, a tie must not move -- with every mix and
sum in double), and ActShiftRef, an autograd Function of torch ops only that runs in the
dtype of its input on any device.
"""
import torch
import torch.nn.functional as F

GAMMA, ZETA = -0.1, 1.1


def _bc(v, x):
    """A (C,) vector broadcast over x = (N, C, ...)."""
    return v.reshape((1, -1) + (1,) * (x.dim() - 2))


def grid(delta, s, dtype=torch.float32):
    """d_i = fp32(delta * s_i): the product of the fp32 delta and the fp32 s_i."""
    d = delta.detach().reshape(()).to(torch.float32) * torch.tensor(float(s), dtype=torch.float32,
                                                                   device=delta.device)
    return d.to(dtype)


def candidates(x, delta, zp, shifts, n_bits):
    """([Q_i], [in_i]) in x's dtype, by ChannelQuantAct 'none' (channelQuantAct.py:56-67)."""
    z = zp.detach().reshape(()).to(x.dtype)
    hi = float(2 ** n_bits - 1)
    Q, inside = [], []
    for s in shifts:
        d = grid(delta, s, x.dtype)
        v = torch.round(x / d) + z
        Q.append((torch.clamp(v, 0, hi) - z) * d)
        inside.append(((v >= 0) & (v <= hi)).to(x.dtype))
    return Q, inside


def soft_targets(alpha):
    return torch.clamp(F.softmax(alpha, dim=-1) * (ZETA - GAMMA) + GAMMA, 0, 1)


def forward(x, p, delta, zp, shifts, n_bits, hard=False):
    """fp32 eager forward in the stated order."""
    Q, _ = candidates(x, delta, zp, shifts, n_bits)
    if hard:
        k = _bc(torch.argmax(p, dim=-1), x)
        y = Q[0]
        for i in range(1, len(shifts)):
            y = torch.where(k == i, Q[i], y)
        return y
    y = Q[0] * _bc(p[:, 0], x)
    for i in range(1, len(shifts)):
        y = y + Q[i] * _bc(p[:, i], x)
    return y


def _reduce_dims(x):
    return [0] + list(range(2, x.dim()))


def backward(x, g, p, delta, zp, shifts, n_bits, hard=False):
    """fp32 eager (dx, dp)."""
    Q, inside = candidates(x, delta, zp, shifts, n_bits)
    if hard:
        k = _bc(torch.argmax(p, dim=-1), x)
        m = inside[0]
        for i in range(1, len(shifts)):
            m = torch.where(k == i, inside[i], m)
        return g * m, torch.zeros_like(p)
    m = torch.zeros_like(x)
    for i in range(len(shifts)):
        m = m + _bc(p[:, i], x) * inside[i]
    dp = torch.stack([(g * Q[i]).sum(dim=_reduce_dims(x)) for i in range(len(shifts))], dim=-1)
    return g * m, dp


def backward64(x, g, p, delta, zp, shifts, n_bits):
    """(dp in fp64, sum |g*Q_i| in fp64): the fp32 candidates, products and sums in double."""
    Q, _ = candidates(x, delta, zp, shifts, n_bits)
    gd = g.double()
    dims = _reduce_dims(x)
    dp = torch.stack([(gd * q.double()).sum(dim=dims) for q in Q], dim=-1)
    mag = torch.stack([(gd * q.double()).abs().sum(dim=dims) for q in Q], dim=-1)
    return dp, mag


def init_mse(x, delta, zp, shifts, n_bits):
    """fp32 eager mse (C, S)."""
    Q, _ = candidates(x, delta, zp, shifts, n_bits)
    return torch.stack([((x - q) ** 2).sum(dim=_reduce_dims(x)) for q in Q], dim=-1)


def init_mse64(x, delta, zp, shifts, n_bits):
    """mse (C, S) in fp64 from the fp32 candidates."""
    Q, _ = candidates(x, delta, zp, shifts, n_bits)
    xd = x.double()
    return torch.stack([((xd - q.double()) ** 2).sum(dim=_reduce_dims(x)) for q in Q], dim=-1)


def inverse_softmax(t):
    t = (t - GAMMA) / (ZETA - GAMMA)
    logits = torch.log(t)
    return logits - torch.mean(logits, dim=-1, keepdim=True)


def init_alpha(mse):
    """ChannelQuant.init_alpha (channelQuant.py:158-191) on a (C, S) error table: clip is
    overridden to 0.33 (:160), to 1.0 for a single target."""
    S = mse.shape[-1]
    _, idx = torch.min(mse, dim=-1)
    clip, remain = (1.0, 0) if S == 1 else (0.33, (1.0 - 0.33) / (S - 1))
    table = torch.full((mse.shape[0], S), remain, dtype=torch.float, device=mse.device)
    table[idx.unsqueeze(-1) == torch.arange(S, device=mse.device)] = clip
    return inverse_softmax(table)


class ActShiftRef(torch.autograd.Function):
    """The contract as an autograd Function of torch ops, in x's dtype (fp32: the stated order;
    fp64: the same rule with the candidates computed in double)."""

    @staticmethod
    def forward(ctx, x, p, delta, zp, shifts, n_bits, hard):
        ctx.save_for_backward(x, p, delta, zp)
        ctx.cfg = (shifts, n_bits, hard)
        return forward(x, p.to(x.dtype), delta, zp, shifts, n_bits, hard)

    @staticmethod
    def backward(ctx, g):
        x, p, delta, zp = ctx.saved_tensors
        shifts, n_bits, hard = ctx.cfg
        dx, dp = backward(x, g, p.to(x.dtype), delta, zp, shifts, n_bits, hard)
        return dx, dp.to(p.dtype), None, None, None, None, None


class RefActQuant(torch.nn.Module):
    """ChannelQuantAct 'shiftFeature' built from ActShiftRef: alpha (C, S) is its parameter."""

    def __init__(self, delta, zp, shifts, n_bits, alpha):
        super().__init__()
        self.delta, self.zero_point = delta.detach().clone(), zp.detach().clone()
        self.shifts, self.n_bits = tuple(float(s) for s in shifts), int(n_bits)
        self.alpha = torch.nn.Parameter(alpha.detach().clone())
        self.hard_targets = False

    def forward(self, x):
        return ActShiftRef.apply(x, soft_targets(self.alpha), self.delta, self.zero_point,
                                 self.shifts, self.n_bits, self.hard_targets)
