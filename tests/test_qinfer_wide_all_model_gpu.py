"""Integer inference of whole models whose scaled weights leave int8 on grouped convs, depthwise
convs and the fc (quant/integer.py, wide=True, wide_all=True), on a (2, 3, 32, 32) batch with random
weights.

RegNetX-600M at W4A8 with EVERY QuantModule -- stem and fc included, as the shiftedScale drivers
leave them -- in the finished per-(co, ci) ChannelQuant state (the recipe of
test_qinfer_perci_model_gpu.py extended to bare layers): with grouped, per_ci, wide and wide_all
every layer the plain-weight plan takes is planned, the grouped layers on the two-plane blob, each
within 9 * 2^-24 of the fp64 convolution of its own input (teacher-forced); the carried plan has the
plain-weight model's 15 tail edges and the uncarried logits; under carry_head the fc runs on K30 with
the wide blob, its logits the host restatement of the head from the carried codes bit for bit and
within the derived bound of the decoded head; a graph replay and an export / load round trip
reproduce the plan; with wide_all off the reasons and the decoded logits are the earlier ones.

MobileNetV2 with ChannelQuantMSE column scales at W4 on the grid L = 16: every depthwise layer is
planned (|m| up to 15 * 16 leaves int8), bounded, and the carried logits are the uncarried ones."""
import numpy as np
import pytest
import torch

from test_qinfer_colscale_model_gpu import (assert_teacher_forced_bound, is_colscaled, logits_of,
                                            same_bits, shrink_columns)
from test_qinfer_model_gpu import capture_raw, host, parity_log

pytestmark = pytest.mark.gpu
BATCH = (2, 3, 32, 32)
SHIFT = [31 / 32, 33 / 32, 1.0]
MODE = dict(grouped=True, per_ci=True, wide=True, wide_all=True)
HEAD = ("model.s4.b7", "model.avgpool", "model.fc")
DENSE_ONLY = "; the wide operand is dense only, the grouped kernels (K26) read int8"
LEAVES = ("scaled weight (q - z) * k leaves int8 (|m| > 127), or a zero point is not an integer "
          "code")
PLAIN_FC = ("weight scale is per (co, ci) (channelquant:adaround): the pooled-operand fc takes plain "
            "weights only")


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


def build(seed, wb=4, ab=8, arch="regnetx_600m"):
    from shiftedscalequantization_amd import drivers as D
    torch.manual_seed(seed)
    return D.build_qnn(arch, wb, ab, w_scale_method="max", device="cuda")


def shifted_all(Q, seed=21):
    """(model, sample): weight-quant init, then EVERY QuantModule's quantizer brought to the
    finished per-(co, ci) state; act quantization on and initialised on the sample."""
    from shiftedscalequantization_amd import drivers as D
    qnn = build(seed)
    x = torch.randn(*BATCH, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(x)
    g = torch.Generator().manual_seed(seed + 2)
    for n, m in qnn.named_modules():
        if not isinstance(m, Q.QuantModule):
            continue
        D.build_ShiftedChannelQuantLayer(qnn, "." + n, m, 1.0, shiftTarget=list(SHIFT))
        q = m.weight_quantizer
        q.init_v(x=m.org_weight.data.clone().detach())
        q.alpha.data.copy_(torch.randn(q.alpha.shape, generator=g).to(q.alpha.device))
        q.hard_targets = True
        q.update_delta()
        q.init_beta(x=m.org_weight.data.clone().detach())
        q.opt_mode = "adaround"
        q.hard_round = True
    qnn.set_quant_state(True, True)
    with torch.no_grad():
        qnn(x)
    return qnn.eval(), x


@pytest.fixture(scope="module")
def plain_plan(Q):
    """What the plain-weight model of the same architecture plans: (grouped plan, tail edges)."""
    qnn = build(21)
    x = torch.randn(*BATCH, generator=torch.Generator().manual_seed(22)).cuda()
    qnn.set_quant_state(True, True)
    with torch.no_grad():
        qnn(x)
    qnn.eval()
    try:
        plan = Q.enable_integer_inference(qnn, x, grouped=True, carry_blocks=True)
        edges = Q.block_carry_report(qnn)["edges"]
        head = Q.enable_integer_inference(qnn, x, grouped=True, carry_head=True)
    finally:
        Q.disable_integer_inference(qnn)
    assert len(edges) == 15 and head["model.fc"] == "int8"
    return plan, edges, head


@pytest.fixture(scope="module")
def net(Q):
    qnn, x = shifted_all(Q)
    with torch.no_grad():
        decoded = qnn(x).clone()
    return qnn, x, decoded


def grouped_names(Q, qnn):
    return [n for n, m in qnn.named_modules() if isinstance(m, Q.QuantModule)
            and m.weight.dim() == 4 and m.fwd_kwargs.get("groups", 1) != 1]


def test_regnetx_every_layer_scaled_is_planned_and_bounded(Q, net, plain_plan):
    qnn, x, decoded = net
    mods = dict(qnn.named_modules())
    want = [n for n, v in plain_plan[0].items() if v == "int8"]
    grouped = grouped_names(Q, qnn)
    assert len(grouped) == 16 and set(grouped) <= set(want)
    assert all(Q.dequant_form(mods[n])[1]["per_ci"] for n in plain_plan[0])
    try:
        plan = Q.enable_integer_inference(qnn, x, **MODE)
        assert all(plan[n] == "int8" for n in want), {n: plan[n] for n in want if plan[n] != "int8"}
        int8 = [n for n in plan if plan[n] == "int8"]
        preps = {n: mods[n]._int_plan.prepared for n in int8}
        # conditions of the setup: W4 on the L = 32 grid leaves int8, every grouped layer holds the
        # two-plane blob and every dense one the dense wide blob
        assert all(preps[n].wide and preps[n].wide_all and mods[n]._int_plan.kind == "grouped"
                   for n in grouped)
        assert all(preps[n].wide and not preps[n].wide_all for n in int8 if n not in grouped)
        got, restore = capture_raw(qnn, int8)
        with torch.no_grad():
            logits = qnn(x)
        restore()
        rep = Q.integer_report(qnn)
        assert rep["off_grid"] == 0 and rep["calls"] == {n: 1 for n in int8}
        worst = assert_teacher_forced_bound(qnn, got, "regnetx_600m-wide-all-W4A8")
        parity_log({"test": "int_infer_wide_all_model", "arch": "regnetx_600m", "w_bits": 4, "a_bits": 8,
                    "int8_layers": len(int8), "grouped_wide_layers": len(grouped),
                    "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 9.0,
                    "max_logit_diff": float((logits - decoded).abs().max()),
                    "max_logit": float(decoded.abs().max())})
    finally:
        Q.disable_integer_inference(qnn)


def test_regnetx_wide_all_off_keeps_todays_reasons_and_the_decoded_logits(Q, net, plain_plan):
    qnn, x, decoded = net
    grouped = grouped_names(Q, qnn)
    try:
        plan, logits, rep = logits_of(Q, qnn, x)
        assert not any(v == "int8" for v in plan.values()) and rep == {"off_grid": 0, "calls": {}}
        assert same_bits(logits, decoded)
        off = dict(MODE, wide_all=False)
        plan = Q.enable_integer_inference(qnn, x, **off)
        assert all(plan[n] == LEAVES + DENSE_ONLY for n in grouped), {n: plan[n] for n in grouped}
        # the keyword alone (without `wide`) changes nothing either
        assert Q.enable_integer_inference(qnn, x, grouped=True, per_ci=True, wide_all=True) == \
            Q.enable_integer_inference(qnn, x, grouped=True, per_ci=True)
        # no tail edge survives a grouped conv on the decoded path, and the fc is refused as before
        plan = Q.enable_integer_inference(qnn, x, carry_head=True, **off)
        assert Q.block_carry_report(qnn)["edges"] == [] and plan["model.fc"] == PLAIN_FC
        assert Q.head_carry_report(qnn)["edges"] == []
    finally:
        Q.disable_integer_inference(qnn)


def test_regnetx_carried_plan_has_the_plain_models_edges_and_the_uncarried_logits(Q, net, plain_plan):
    qnn, x, _ = net
    try:
        plan0, base, rep0 = logits_of(Q, qnn, x, **MODE)
        plan1, carried, rep1 = logits_of(Q, qnn, x, carry_blocks=True, **MODE)
        assert plan1 == plan0 and rep0["off_grid"] == 0 and rep1["off_grid"] == 0
        edges = Q.block_carry_report(qnn)["edges"]
        assert len(edges) == 15 and edges == plain_plan[1]
        assert same_bits(carried, base)
        graph = Q.IntegerGraph(qnn)
        first, again = graph(x).clone(), graph(x).clone()
        assert same_bits(first, carried) and same_bits(again, carried)
        assert Q.integer_report(qnn)["off_grid"] == 0
    finally:
        Q.disable_integer_inference(qnn)


def host_head(K, Q, fc, codes, p):
    """The whole head restated on the host from the carried codes and the fc's stored floats:
    (raw fp32 (N, Co), the decoded head in fp64, its absolute-value companion)."""
    what, f = Q.dequant_form(fc)
    Co, Ci = fc.weight.shape
    L, base, k = K.perci_grid(f["scale"], Co, Ci, K.QWIDE_MAX)
    scale = host(f["scale"]).reshape(Co, Ci)
    w = host(what).reshape(Co, Ci)
    centred = np.rint(w.astype(np.float64) / scale).astype(np.int64)            # q - z
    assert np.array_equal((centred.astype(np.float32) * scale).view(np.int32), w.view(np.int32))
    m = centred * k.numpy().reshape(Co, Ci).astype(np.int64)
    N, H, W, _ = codes.shape
    q = host(codes).astype(np.int64)[..., :Ci] + K.code_offset(p.n_bits, p.sym)
    P = (q - int(p.zp)).reshape(N, H * W, Ci).sum(1)
    I = P @ m.T
    s0 = np.float32(p.delta) * base.numpy()
    assert s0.dtype == np.float32
    sh = s0 / np.float32(L * H * W)
    xhat = ((q - p.zp).astype(np.float32) * np.float32(p.delta)).astype(np.float64)
    mean, amean = xhat.reshape(N, H * W, Ci).mean(1), np.abs(xhat).reshape(N, H * W, Ci).mean(1)
    w64 = w.astype(np.float64)
    return I.astype(np.float32) * sh.reshape(1, -1), mean @ w64.T, amean @ np.abs(w64).T, int(np.abs(m).max())


def test_regnetx_scaled_fc_runs_on_k30_with_the_wide_blob(Q, net, plain_plan, monkeypatch):
    """The bound: 10 * 2^-24 * sum_c mean_hw|x_hat| |W_hat|, the plain head's 8 units plus the 2
    roundings the grid adds to the decoded weight ("The wide operand everywhere")."""
    from shiftedscalequantization_amd import kernels as K
    qnn, x, _ = net
    mods = dict(qnn.named_modules())
    fc = mods["model.fc"]
    try:
        fed, real = [], K.avgpool_codes
        monkeypatch.setattr(K, "avgpool_codes", lambda c: (fed.append(c), real(c))[1])
        plan, logits, rep = logits_of(Q, qnn, x, carry_head=True, **MODE)
        monkeypatch.setattr(K, "avgpool_codes", real)
        assert [n for n, v in plan.items() if v == "int8"] == [n for n, v in plain_plan[2].items() if v == "int8"]
        head = Q.head_carry_report(qnn)
        assert head == {"edges": [HEAD], "calls": {HEAD[0]: 1}, "pooled": {HEAD[1]: 1}, "fc": {HEAD[2]: 1}}
        assert rep["off_grid"] == 0
        p = fc._int_plan
        assert p.prepared.wide and p.prepared.centred and p.head_grid is not None and p.head_grid[1] == 32
        assert len(fed) == 2 and torch.equal(fed[0], fed[1])
        raw, ref64, A, mmax = host_head(K, Q, fc, fed[1], p)
        assert 127 < mmax <= K.QWIDE_MAX
        exp = torch.from_numpy(raw).cuda()
        exp = exp if fc.bias is None else exp + fc.bias.view(1, -1)
        gamma, phi = fc.affine()
        if gamma is not None:
            exp = exp * gamma + phi
        with torch.no_grad():
            exp = fc.activation_function(exp)
            if fc.use_act_quant and not fc.disable_act_quant:
                exp = fc.act_quantizer(exp)
        assert same_bits(logits, exp)
        err = np.abs(raw.astype(np.float64) - ref64)
        worst = float((err[A > 0] / A[A > 0]).max())
        parity_log({"test": "int_infer_wide_all_head", "arch": "regnetx_600m", "fc_max_m": mmax,
                    "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 10.0})
        assert np.all(err <= 10 * 2.0 ** -24 * A), worst * 2 ** 24
    finally:
        Q.disable_integer_inference(qnn)


def test_regnetx_export_round_trip_plans_the_same_layers_with_equal_blobs(Q, net):
    qnn, x, decoded = net
    try:
        plan, logits, rep = logits_of(Q, qnn, x, carry_head=True, **MODE)
        Q.disable_integer_inference(qnn)
        src = Q.export_quantized(qnn)
        fresh = build(99)
        Q.load_quantized(fresh, src)
        fresh.set_quant_state(True, True)
        fresh.eval()
        with torch.no_grad():
            assert same_bits(fresh(x), decoded)
        plan_f, logits_f, rep_f = logits_of(Q, fresh, x, carry_head=True, **MODE)
        assert plan_f == plan and rep_f["off_grid"] == 0 and rep["off_grid"] == 0
        assert same_bits(logits_f, logits)
        Q.enable_integer_inference(qnn, x, carry_head=True, **MODE)
        mods, fmods = dict(qnn.named_modules()), dict(fresh.named_modules())
        for n, v in plan.items():
            if v == "int8":
                a, b = mods[n]._int_plan, fmods[n]._int_plan
                assert (a.prepared.wide, a.prepared.wide_all) == (b.prepared.wide, b.prepared.wide_all)
                assert torch.equal(a.prepared.blob, b.prepared.blob) and same_bits(a.scale, b.scale)
        Q.disable_integer_inference(fresh)
    finally:
        Q.disable_integer_inference(qnn)


# ---------------------------------------------------------------- MobileNetV2, column scales
def test_mobilenetv2_w4_column_scaled_depthwise_layers(Q):
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd import kernels as K
    qnn = build(31, 4, 8, "mobilenetv2")
    shrink_columns(Q, qnn)
    x = torch.randn(*BATCH, generator=torch.Generator().manual_seed(32)).cuda()
    fc = [n for n, m in qnn.named_modules() if isinstance(m, Q.QuantModule)][-1]
    D.channelShift_wMSE(qnn, x, level=16, threshold=2.0, layerDisabled=["." + fc])
    qnn.set_quant_state(True, True)
    with torch.no_grad():
        qnn(x)
    qnn.eval()
    mods = dict(qnn.named_modules())
    dw = [n for n, m in mods.items() if isinstance(m, Q.QuantModule) and m.weight.dim() == 4
          and m.fwd_kwargs.get("groups", 1) != 1]
    assert len(dw) == 17 and all(is_colscaled(Q, mods[n]) for n in dw)
    mode = dict(grouped=True, colscale=True, wide=True)
    try:
        before = Q.enable_integer_inference(qnn, x, **mode)
        lost = [n for n in dw if before[n] != "int8"]
        plan0, base, rep0 = logits_of(Q, qnn, x, wide_all=True, **mode)
        assert all(plan0[n] == "int8" for n in dw), {n: plan0[n] for n in dw if plan0[n] != "int8"}
        wide = [n for n in dw if mods[n]._int_plan.prepared.wide_all]
        # conditions of the setup: the keyword gains depthwise layers, and they run the wide form
        print({"depthwise_lost_without_wide_all": len(lost), "on_the_wide_blob": len(wide)})
        assert lost and set(lost) <= set(wide)
        assert all(mods[n]._int_plan.kind == "depthwise" for n in dw)
        grids = [K.colscale_grid(mods[n].weight_quantizer.inp_scale, K.QWIDE_MAX_L, K.QWIDE_MAX)
                 for n in wide]
        assert all(g is not None and g[0] <= 16 for g in grids)
        int8 = [n for n, v in plan0.items() if v == "int8" and mods[n].weight.dim() == 4]
        got, restore = capture_raw(qnn, int8)
        with torch.no_grad():
            qnn(x)
        restore()
        assert Q.integer_report(qnn)["off_grid"] == 0
        worst = assert_teacher_forced_bound(qnn, got, "mobilenetv2-wide-all-W4A8")
        plan1, carried, rep1 = logits_of(Q, qnn, x, carry_blocks=True, wide_all=True, **mode)
        assert plan1 == plan0 and rep0["off_grid"] == 0 and rep1["off_grid"] == 0
        assert Q.block_carry_report(qnn)["edges"] and same_bits(carried, base)
        parity_log({"test": "int_infer_wide_all_model", "arch": "mobilenetv2", "w_bits": 4, "a_bits": 8,
                    "depthwise": len(dw), "depthwise_gained": len(lost), "depthwise_wide": len(wide),
                    "grid_L": sorted({g[0] for g in grids}),
                    "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 9.0})
    finally:
        Q.disable_integer_inference(qnn)
