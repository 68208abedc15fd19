"""Grouped and depthwise integer convs on per-channel act grids (grouped=True, act_shift=True): K24
folds k_a[ci] into the operand by kind, the CHQ forms of K25 / K26 emit onto out_dch[Co].  On the
parent the wrappers raise and the planner reports these layers as refused."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_qinfer_actshift_gpu import (AB, TARGETS, ZA, code_ref, dev, fake_quant_chain, grid, host,
                                      on_grid, stored, word)
from test_qinfer_grouped_gpu import SHAPES, encode_weight
from test_qinfer_perci_host import operand_sum, ref_output

F32 = np.float32
WIDE_TARGETS = [1.0, 31.0 / 32.0]          # L_a = 32, k_a in {32, 31}: W4's |q - z| * k_a passes 127


def reader_case(K, name, form, seed=0):
    """Per-channel input codes, a hard weight with k_a folded in by kind, the int64 reference I.
    `form`: "wide", W4 on WIDE_TARGETS; "kcol" (depthwise), a column scale {1/2, 1} (exact in fp32)
    beside k_a."""
    N, C, H, W, Co, R, st, pad, G = SHAPES[name]
    Cig, wide = C // G, form == "wide"
    wb = 4 if wide else 2
    rng = np.random.default_rng(zlib.crc32(repr((name, form, seed)).encode()))
    _, idx, delta = grid(rng, C, 2)
    tg = WIDE_TARGETS if wide else TARGETS[2]
    d = delta * np.array(tg, F32)[idx]
    La, k = K.actshift_grid(float(delta), tg)
    ka = np.array(k)[idx]
    qa, xhat = on_grid(rng, (N, C, H, W), d)
    qw, zw = rng.integers(0, 2 ** wb, (Co, Cig, R, R)), rng.integers(0, 2 ** wb, Co)
    d1 = rng.uniform(1e-3, 2e-2, Co).astype(F32)
    what, _ = encode_weight(K, qw, zw, d1, wb, False, G)
    kc = rng.integers(1, 3, R * R) if form == "kcol" else np.ones(R * R, np.int64)     # k / 2
    what = what * (kc.astype(F32) / F32(2 if form == "kcol" else 1)).reshape(1, 1, R, R)
    packed, bad = K.pack_encode(dev(what), dev(zw), dev(d1), False, dev(kc / 2) if form == "kcol"
                                else None, wb, 0, 2 ** wb - 1)
    assert bad == 0
    kfac = ka.reshape(G, 1, Cig).repeat(Co // G, 1).reshape(Co, Cig)      # k_a of co's own group
    fold = dict(kfac=torch.from_numpy(kfac))
    if Cig == 1 and Co == G:
        fold = dict(kch=torch.from_numpy(ka), kcol=torch.from_numpy(kc) if form == "kcol" else None)
    prep = K.qweight_prepare(packed, qw.shape, dev(zw), wb, 0, groups=G, wide=wide, wide_all=wide, **fold)
    m = (qw - zw.reshape(-1, 1, 1, 1)) * kfac[:, :, None, None] * kc.reshape(1, 1, R, R)
    assert int(prep.bad.item()) == 0 and prep.wide == wide and (np.abs(m).max() > 127) == wide
    scale = ((delta * d1) / F32(La * (2 if form == "kcol" else 1))).astype(F32)
    return dict(x=dev(xhat), xhat=xhat, what=what, prep=prep, rng=rng, Co=Co, cs=K.ChannelScale(dev(d)),
                scale=scale, I=operand_sum(qa, int(ZA), m, st, pad, G),
                conv=dict(stride=st, padding=pad, groups=G), act=dict(act_zp=ZA, act_bits=AB))


@pytest.mark.gpu
@pytest.mark.parametrize("name,form", [(n, None) for n in ("g2_one_chunk", "cig24_s2", "multiplier2",
                                                           "dw_c5", "dw_c40_s2", "dw_5x5")] +
                         [("cig24_s2", "wide"), ("dw_c40_s2", "wide"), ("dw_5x5", "kcol")])
def test_folded_reader(name, form):
    """K.qconv: fp32(I) * scale[co] bit for bit, and within 9 * 2^-24 * conv64(|x_hat|, |W_hat|) of
    the decoded conv (test_folded_consumer's bound: 8 roundings, one more for the conversion)."""
    from shiftedscalequantization_amd import kernels as K
    c, bad = reader_case(K, name, form), word()
    y = K.qconv(c["x"], c["prep"], dev(c["scale"]), **c["conv"], **c["act"], act_delta=c["cs"], bad=bad)
    ref, out = ref_output(c["I"], c["scale"]), host(y)
    assert int(bad.item()) == 0 and ref.any()
    assert np.array_equal(out.view(np.int32), ref.view(np.int32))
    xt, wt = torch.from_numpy(c["xhat"]).double(), torch.from_numpy(c["what"]).double()
    ref64, A = F.conv2d(xt, wt, **c["conv"]).numpy(), F.conv2d(xt.abs(), wt.abs(), **c["conv"]).numpy()
    err = np.abs(out.astype(np.float64) - ref64)
    print({"case": (name, form), "err_over_A_in_2^-24": float((err[A > 0] / A[A > 0]).max() * 2 ** 24)})
    assert np.all(err <= 9 * 2.0 ** -24 * A)


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,zero", [("cig40_cog20", None, False), ("1x1_cog65", None, False),
                                            ("dw_c5", None, False), ("dw_c40_s2", None, False),
                                            ("cig24_s2", "wide", False), ("dw_c5", None, True),
                                            ("cig40_cog20", None, True)])
def test_emitters_grouped(name, form, zero):
    """K.qconv_codes onto out_dch: code_ref's codes, decoded the fake-quant chain on the same y bit
    for bit, zero channel padding.  `zero`: the last out_dch entry is 0, no activation and a bias
    that keeps its t > 0: each of the channel's elements is t / 0 = inf, a NaN code (qinfer_epi.h),
    counted once, and the entry itself once per launch -- *bad = pixels + 1, exactly."""
    from shiftedscalequantization_amd import kernels as K
    c = reader_case(K, name, form, seed=1)
    rng, Co, yraw = c["rng"], c["Co"], ref_output(c["I"], c["scale"])
    od, oidx, odelta = grid(rng, Co, 3, delta=float(np.abs(yraw).max()) / 6)
    bias, phi = (rng.normal(0, 0.3 * odelta, Co).astype(F32) for _ in range(2))
    gamma = rng.uniform(0.8, 1.2, Co).astype(F32)
    if zero:
        od[Co - 1], bias[Co - 1] = 0.0, 4 * np.abs(yraw).max()
    vecs, bad, ocs = (dev(bias), dev(gamma), dev(phi)), word(), K.ChannelScale(dev(od))
    codes = K.qconv_codes(c["x"], c["prep"], dev(c["scale"]), **c["conv"], **c["act"], act_delta=c["cs"],
                          bias=vecs[0], gamma=vecs[1], phi=vecs[2], relu=int(not zero), out_delta=ocs,
                          out_zp=ZA, out_bits=AB, bad=bad)
    if zero:
        assert int(bad.item()) == yraw.size // Co + 1
        return
    q = code_ref(yraw, bias, gamma, phi, None, 1, od)
    assert int(bad.item()) == 0 and len(np.unique(q)) > 4
    assert np.array_equal(host(codes), stored(q)) and not host(codes)[..., Co:].any()
    chain = fake_quant_chain(K, dev(yraw), *vecs, None, 1, oidx, odelta, 3)
    back = K.act_decode(codes, Co, ocs, ZA, AB)
    assert torch.equal(back.view(torch.int32), chain.view(torch.int32))


@pytest.mark.gpu
def test_model_shifted_inverted_residuals():
    """Stem, a stride-2 and an identity-add InvertedResidual, pool, fc; every conv of the blocks on
    int8, bounded layer by layer, the carried plan and three graph replays bit-equal to the stripped."""
    from shiftedscalequantization_amd import drivers as D, nets, quant as Q
    from test_actshift_recon_gpu import log_parity
    from test_qinfer_colscale_model_gpu import (assert_teacher_forced_bound, capture_raw, logits_of,
                                                strip_carries)
    torch.manual_seed(5)
    net = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8), nn.ReLU6(),
                        nets.InvertedResidual(8, 16, 2, 2), nets.InvertedResidual(16, 16, 1, 2),
                        nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(16, 10)).eval()
    net.stem_chain = lambda: [net[i] for i in range(4)]
    qnn = Q.QuantModel(net, {"n_bits": 4, "channel_wise": True, "scale_method": "max"},
                       {"n_bits": 4, "channel_wise": False, "scale_method": "mse",
                        "leaf_param": True}).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    x = torch.randn(16, 3, 16, 16, generator=torch.Generator().manual_seed(21)).cuda()
    qnn.set_quant_state(True, True)
    with torch.no_grad():
        qnn(x)
    qnn.disable_network_output_quantization()
    torch.manual_seed(1005)
    D.act_shift_recon(qnn, x, 8, x.device, targets=(1.0, 0.5), iters=3, verbose=False)
    for m in [m for b in (3, 4) for m in list(net[b].conv)[:-1]]:
        if not isinstance(m.act_quantizer, Q.ChannelQuantAct):      # the driver left it: set by hand
            q = Q.ChannelQuantAct(m.act_quantizer, shiftTarget=[1.0, 0.5])
            q.alpha = nn.Parameter(5.0 * torch.eye(2, device="cuda")[torch.arange(m.weight.shape[0]) % 2])
            q.opt_mode, q.hard_targets, q.shiftedDone = "shiftFeature", True, True
            m.act_quantizer = q
    mode = dict(grouped=True, carry_stem=True, act_shift=True)
    with torch.no_grad():
        want = qnn(x).clone()
    try:
        report = Q.enable_integer_inference(qnn, x[:4], **mode)
        convs = [n for n in report if ".conv." in n]
        assert len(convs) == 6 and [report[n] for n in convs] == ["int8"] * 6, report
        strip_carries(Q, qnn)
        got, restore = capture_raw(qnn, convs)
        with torch.no_grad():
            base = qnn(x).clone()
        restore()
        assert Q.integer_report(qnn)["off_grid"] == 0
        assert_teacher_forced_bound(qnn, got, "actshift-inverted-residual", bound=9.0)
        plan, logits, rep = logits_of(Q, qnn, x, **mode)
        assert plan == report and rep["off_grid"] == 0
        assert torch.equal(logits.view(torch.int32), base.view(torch.int32))
        calls = Q.carry_report(qnn)["calls"]        # 1x1 -> depthwise and depthwise -> 1x1, once each
        assert all(calls[f"model.{b}.conv.{i}"] == 1 for b in (3, 4) for i in (0, 1)), calls
        graph = Q.IntegerGraph(qnn)
        for _ in range(3):
            assert torch.equal(graph(x).view(torch.int32), logits.view(torch.int32))
        log_parity({"test": "int_infer_actshift_inverted_residual", "max_logit": float(want.abs().max()),
                    "max_logit_diff": float((logits - want).abs().max())})
    finally:
        Q.disable_integer_inference(qnn)


def test_weight_operand_folds_a_shifted_grid_by_kind():
    """Host arithmetic: kind 2 takes k_a of co's own group per (co, ci), times the weight's own
    factors; kind 1 takes k_a per channel beside its column factors."""
    from shiftedscalequantization_amd.quant import integer as I
    from test_qinfer_operand_host import col, fields, ints, shifted_act
    on = I.PlanFlags(grouped=True, colscale=True, per_ci=True, act_shift=True)
    ka = np.array([3, 4, 5, 4, 3, 5], np.int64)
    act, want = shifted_act(4, ka.tolist()), np.repeat(ka.reshape(2, 1, 3), 2, axis=1).reshape(4, 3)
    kcol, kfac, L, _ = I.weight_operand(fields(4), (4, 3, 3, 3), 2, act, False, on, "grouped")
    assert kcol is None and L == 4 and np.array_equal(ints(kfac).reshape(4, 3), want)
    f = fields(4, col_scale=col([0.5, 1.0, 0.5]), kind="channelquantmse")
    kcol, kfac, L, _ = I.weight_operand(f, (4, 3, 1, 1), 2, act, False, on, "grouped")
    assert kcol is None and L == 8 and np.array_equal(ints(kfac).reshape(4, 3), want * np.array([1, 2, 1]))
    f = fields(4, col_scale=torch.tensor([0.5, 1.0] * 6), kind="channelquantmse")
    assert "varies over (r, s)" in I.weight_operand(f, (4, 3, 2, 2), 2, act, False, on, "grouped")
    f = fields(6, col_scale=torch.tensor([0.5, 1.0, 0.5, 1.0]), kind="channelquantmse")
    kcol, kfac, L, _ = I.weight_operand(f, (6, 1, 2, 2), 6, act, False, on, "depthwise")
    assert L == 8 and np.array_equal(ints(kcol), [1, 2, 1, 2]) and np.array_equal(ints(kfac), ka)
