"""block_recon_fused_shiftedScale(act=True, act_shift_learn_delta=True) with the act quantizers
inside the epilogue pass (K34, K.ACTSHIFT_EPI = "auto") against the two-pass route ("0"): the
same losses, alphas and deltas bit for bit, on test_actshift_recon_gpu's toy (a QuantBasicBlock,
8 channels, 8x8 planes, 16 cached samples), rebuilt here.  Before the feature there was no
fused Function to run."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def make():
    """(qnn, block): weight and act quantizers initialised, the block's features cached."""
    from shiftedscalequantization_amd import drivers as D, nets, quant as Q
    torch.manual_seed(5)
    net = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8), nn.ReLU(),
                        nets.BasicBlock(8, 8), nn.AdaptiveAvgPool2d(1), nn.Flatten(),
                        nn.Linear(8, 10)).eval()
    qnn = Q.QuantModel(net, {"n_bits": 4, "channel_wise": True, "scale_method": "max"},
                       {"n_bits": 4, "channel_wise": False, "scale_method": "mse",
                        "leaf_param": True}).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    cali = torch.randn(16, 3, 8, 8, generator=torch.Generator().manual_seed(21)).cuda()
    qnn.set_quant_state(True, True)
    with torch.no_grad():
        qnn(cali)
    qnn.disable_network_output_quantization()
    block = D.cache_block_features(qnn, ".model.3", cali, 8, cali.device)
    qnn.set_quant_state(True, True)          # (caching the FP outputs switched act quant off)
    return qnn, block


def run(K, switch, monkeypatch):
    """10 iterations -> (per-iteration losses, final alphas, final deltas, fused forwards run)."""
    from shiftedscalequantization_amd import quant as Q
    monkeypatch.setattr(K, "ACTSHIFT_EPI", switch)
    qnn, block = make()
    losses, calls0 = [], K.EpilogueActShiftFn.calls
    h = block.register_forward_hook(
        lambda m, a, out: losses.append(out.detach().clone()) if torch.is_grad_enabled() else None)
    torch.manual_seed(1005)
    res = Q.block_recon_fused_shiftedScale(block, iters=10, model=qnn, act=True, batch_size=8,
                                           verbose=False, act_shift_learn_delta=True)
    h.remove()
    qs = (block.conv1.act_quantizer, block.act_quantizer)
    assert all(isinstance(q, Q.ChannelQuantAct) for q in qs) and len(losses) == 10
    return (res, losses, [q.alpha.detach().clone() for q in qs],
            [q.delta.detach().clone() for q in qs], K.EpilogueActShiftFn.calls - calls0)


def test_loop_is_bit_identical_with_and_without_the_fused_pass(monkeypatch):
    from shiftedscalequantization_amd import kernels as K
    fused, two = run(K, "auto", monkeypatch), run(K, "0", monkeypatch)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    # conv1's epilogue and the block's tail, each of the 10 training forwards at the least
    assert fused[4] >= 20 and two[4] == 0
    assert fused[0] == two[0]                          # [soft, hard] reconstruction losses
    for k in (1, 2, 3):     # each iteration's block output (the loss's only input), alphas, deltas
        assert len(fused[k]) == len(two[k]) and all(same(a, b) for a, b in zip(fused[k], two[k]))
