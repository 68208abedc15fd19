"""ChannelQuantAct (reference: quant/channelQuantAct.py).

Only opt_mode 'none' runs in the reference: per-tensor q/dq at delta*shiftedScale with a
[0, n-1] clamp and torch.round -- not round_ste, so no gradient reaches x
(channelQuantAct.py:56-67) -> ssq_fq_fwd / ssq_fq_round_bwd here.  Its init_v refers to an
undefined `x` and a missing `isFC`/`x_q` (channelQuantAct.py:125-134, AttributeError /
NameError [probed]), and the 'adaShift' / 'adaround' branches read attributes that are
never created, so those modes raise here too, with an explicit message.

'shiftFeature' is the reference's evident intent for activations (channelQuantAct.py:69
"TODO: from here make function for activation"): the weight side's
shifted_x_quant with the candidates Q_i = 'none'-mode q/dq at delta*s_i computed from the
live tensor, mixed per channel by p = get_sig_soft_targets() (C, S) -> ssq_actshift_fwd /
ssq_actshift_bwd (K33); init_v(x) starts alpha from the per-channel squared errors
(ssq_actshift_init) by ChannelQuant.init_alpha's rule.  delta and zero_point are not
learned in this mode.
"""
import torch
from torch import nn
import torch.nn.functional as F

from .. import kernels as K
from .quant_layer import UniformAffineQuantizer


class ChannelQuantAct(nn.Module):
    @torch.no_grad()
    def __init__(self, uaq: UniformAffineQuantizer, shiftTarget: list = [2 / 2, 2 / 2], name='--'):
        super().__init__()
        self.n_bits = uaq.n_bits
        self.sym = uaq.sym
        self.delta = uaq.delta
        self.zero_point = uaq.zero_point
        self.n_levels = uaq.n_levels
        self.device = 'cuda:0'
        self.shiftedScale = 1.0
        self.shiftTarget = shiftTarget
        self.opt_mode = 'none'
        self.hard_targets = False
        self.gamma, self.zeta = -0.1, 1.1
        self.alpha = None
        self.shiftedDone = False
        self.disable_act_quant = getattr(uaq, 'disable_act_quant', False)
        # code that asks an act quantizer whether its scale exists keeps working
        self.inited = getattr(uaq, 'inited', True)
        self.name = name

    def forward(self, x):
        if self.opt_mode == 'none':
            # asymmetric [0, n-1] clamp whatever uaq.sym says (channelQuantAct.py:63)
            return K.round_quant(x, self.delta, self.zero_point, self.n_bits, False,
                                 scale=self.shiftedScale)
        if self.opt_mode == 'shiftFeature':
            if self.alpha is None:
                raise RuntimeError("ChannelQuantAct 'shiftFeature' needs init_v(x) first")
            return K.actshift(K.materialize_epi(x), self.get_sig_soft_targets(), self.delta,
                              self.zero_point, self.shiftTarget, self.n_bits, self.hard_targets)
        raise NotImplementedError(
            f"ChannelQuantAct opt_mode={self.opt_mode!r} is broken in the reference "
            "(channelQuantAct.py:38-61,125-134 read attributes that are never set)")

    def get_sig_soft_targets(self):
        return torch.clamp(F.softmax(self.alpha, dim=-1) * (self.zeta - self.gamma) + self.gamma, 0, 1)

    def get_soft_targets(self):
        return torch.clamp(torch.sigmoid(self.alpha) * (self.zeta - self.gamma) + self.gamma, 0, 1)

    def inverse_softmax(self, x):
        x = (x - self.gamma) / (self.zeta - self.gamma)
        logits = torch.log(x)
        return logits - torch.mean(logits, dim=-1, keepdim=True)

    def init_alpha(self, mse, clip=0.80):
        """ChannelQuant.init_alpha (channelQuant.py:158-191) from the (C, S) squared errors:
        the argmin shift gets `clip`, the others share the rest; clip is overridden to 0.33
        as on the weight side (:160), and to 1.0 for a single target."""
        clip = 0.33
        S = mse.shape[-1]
        _, min_index = torch.min(mse, dim=-1)
        if S == 1:
            remain, clip = 0, 1.0
        else:
            remain = (1.0 - clip) / (S - 1)
        alpha = torch.full((mse.shape[0], S), remain, dtype=torch.float, device=mse.device)
        mask = min_index.unsqueeze(-1) == torch.arange(S, device=mse.device)
        alpha[mask] = clip
        return self.inverse_softmax(alpha)

    @torch.no_grad()
    def init_v(self, x: torch.Tensor):
        """The evident intent of channelQuantAct.py:125-134 with the input it forgot to take:
        per-channel errors of the S candidates on x -> alpha (C, S); mode -> 'shiftFeature'."""
        S = len(self.shiftTarget)
        if S > K.ACTSHIFT_MAX_S:
            raise ValueError(f"ChannelQuantAct: at most {K.ACTSHIFT_MAX_S} shift targets, got {S}")
        mse = K.actshift_init(K.materialize_epi(x), self.delta, self.zero_point, self.shiftTarget,
                              self.n_bits)
        self.shiftedScale = 1.0
        self.alpha = nn.Parameter(self.init_alpha(mse, clip=(0.90 - 0.05 * S)))
        self.opt_mode = 'shiftFeature'
        self.inited = True
        return mse

    def shift_index(self):
        """The chosen shift target per channel: first argmax of p (torch.argmax's tie rule)."""
        return torch.argmax(self.get_sig_soft_targets().detach(), dim=-1)

    def get_delta(self):
        """fp32(delta * s_k) per channel, (1, C, 1, 1) (channelQuantAct.py:107-123)."""
        st = torch.tensor([float(s) for s in self.shiftTarget], dtype=torch.float32,
                          device=self.alpha.device)
        return (self.delta.detach().reshape(()) * st[self.shift_index()]).view(1, -1, 1, 1)
