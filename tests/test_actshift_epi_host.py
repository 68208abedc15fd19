"""K34 (the shifted-scale act quantizer inside the K13 epilogue) without a device: the ABI, the
refusals that come before any launch, and the rule that admits a site to the fused route."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = ("ssq_epilogue_actshift_fwd", "ssq_epilogue_actshift_bwd",
       "ssq_epilogue_actshift_bwd_workspace_size")


def test_entry_points_declared_exported_and_bound():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssq.h")).read(), flags=re.S)
    for s in ABI:
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % s, src)
        assert proto and hasattr(lib, s) and s in _capi.SIGNATURES, s
        assert len(proto.group(1).split(",")) == len(_capi.SIGNATURES[s][1]), s
    # dp's partials, then one ddelta partial per plane
    assert lib.ssq_epilogue_actshift_bwd_workspace_size(4, 8, 49, 2) == 4 * 8 * (2 + 1) * 8


def test_argument_refusals_without_gpu():
    """What K33 and K13 refuse is refused here too, on the host, before any launch."""
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    sh = (C.c_float * 5)(1.0, 0.5, 0.75, 0.25, 0.125)
    one = C.c_void_p(16)       # never dereferenced: every case below is refused first

    def fwd(S=2, N=2, C_=3, HW=4, relu=1, conv=one, phi=one):
        return lib.ssq_epilogue_actshift_fwd(conv, one, one, phi, None, relu, one, one, one, sh, S,
                                             N, C_, HW, 15, 0, one, None)

    def bwd(S=2, relu=1, g=one, res=None, dres=None, dp=one, hard=0, ws=None, wsn=0):
        return lib.ssq_epilogue_actshift_bwd(one, g, one, one, one, res, relu, one, one, one, sh, S,
                                             2, 3, 4, 15, hard, one, dres, dp, None, ws, wsn, None)
    for f, kw, what in ((fwd, dict(S=5), b"shift targets"), (fwd, dict(conv=None), b"null"),
                        (fwd, dict(N=1 << 11, C_=1 << 10, HW=1 << 10), b"2^31"),
                        (fwd, dict(relu=3), b"activation code"),
                        (fwd, dict(phi=None), b"gamma and phi"),
                        (bwd, dict(S=0), b"shift targets"), (bwd, dict(g=None), b"null"),
                        (bwd, dict(relu=-1), b"activation code"),
                        (bwd, dict(dp=None), b"null pointer (dp)"),
                        (bwd, dict(dres=one), b"dres without res")):
        assert f(**kw) == -1 and what in lib.ssq_last_error(), what
    assert bwd() == -2 and b"workspace" in lib.ssq_last_error()


class DeviceScalar:
    """Stands for a one-element device tensor: the rule reads these two and nothing else."""
    is_cuda = True

    def numel(self):
        return 1


def test_fusability_rule_states_each_condition(monkeypatch):
    from shiftedscalequantization_amd import kernels as K, quant as Q
    from shiftedscalequantization_amd.quant.quant_layer import (UniformAffineQuantizer,
                                                                fusable_shift_act_quantizer)

    def make(**over):
        q = Q.ChannelQuantAct(UniformAffineQuantizer(n_bits=4, disable_act_quant=True),
                              shiftTarget=[1.0, 0.5])
        q.delta, q.zero_point = DeviceScalar(), torch.zeros(())
        q.alpha, q.opt_mode = torch.nn.Parameter(torch.zeros(3, 2)), 'shiftFeature'
        for k, v in over.items():
            setattr(q, k, v)
        return q
    good = make()
    assert fusable_shift_act_quantizer(good, True, (None, torch.ones(3), None)) is good
    hooked = make()
    hooked.register_forward_pre_hook(lambda m, a: None)
    learned = torch.ones(3, requires_grad=True)
    for q, active, params in ((good, False, ()),                        # quantizer off
                              (make(opt_mode='none'), True, ()),        # not the shifted mode
                              (make(alpha=None), True, ()),             # init_v not done
                              (make(delta=torch.ones(2)), True, ()),    # per-channel delta
                              (make(delta=torch.ones(())), True, ()),   # on the CPU
                              (make(zero_point=torch.zeros(2)), True, ()),
                              (hooked, True, ()),
                              (UniformAffineQuantizer(n_bits=4), True, ()),
                              (good, True, (None, learned, None))):     # gamma^z learns
        assert fusable_shift_act_quantizer(q, active, params) is None
    with torch.no_grad():              # no backward: the epilogue parameters are constants
        assert fusable_shift_act_quantizer(good, True, (learned,)) is good
    monkeypatch.setattr(K, "ACTSHIFT_EPI", "0")
    assert fusable_shift_act_quantizer(good, True, ()) is None
    # the Function itself refuses a learned epilogue parameter rather than drop its gradient
    with pytest.raises(K.A.SSQError, match="two passes"):
        K.epilogue_actshift(torch.zeros(1, 3, 2, 2), learned, None, None, None, 0,
                            torch.zeros(3, 2), torch.ones(()), torch.zeros(()), [1.0, 0.5], 4)
