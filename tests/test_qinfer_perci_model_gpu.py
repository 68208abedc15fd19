"""Integer inference of whole models whose weights are scaled per (co, ci) (quant/integer.py,
per_ci=True, wide=True): a random ResNet-18 on a (2, 3, 32, 32) batch whose block convs carry a
ChannelQuant in the state layer_recon_shiftedScale leaves (init_v on the default shift targets,
hard targets, update_delta, hard AdaRound), once at W2A4 (the operand fits int8) and once at W4A8
(it does not: every planned layer takes the wide blob).  The 18 layers the plain route plans are
planned, each within 9 * 2^-24 of the fp64 convolution of its own input (teacher-forced); with
the flags off the report strings are the earlier ones and the logits the decoded model's; an
export / load round trip plans the same layers with equal logits; carried plans and an
IntegerGraph replay give the eager integer forward's logits bit for bit."""
import numpy as np
import pytest
import torch

from test_qinfer_colscale_model_gpu import (assert_teacher_forced_bound, logits_of,
                                            plain_int8_names, same_bits)
from test_qinfer_model_gpu import capture_raw, parity_log

pytestmark = pytest.mark.gpu
BATCH = (2, 3, 32, 32)
SHIFT = [31 / 32, 33 / 32, 1.0]
FORMS = [(2, 4), (4, 8)]                     # (n_bits_w, n_bits_a)
PER_CI = "weight scale is per (co, ci) (channelquant:adaround)"
LEAVES = ("scaled weight (q - z) * k leaves int8 (|m| > 127), or a zero point is not an integer "
          "code")


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


def shifted(Q, wb, ab, seed=21):
    """(model, sample): weight-quant init, then every block conv's quantizer brought to the
    finished per-(co, ci) state; act quantization on and initialised on the sample."""
    from shiftedscalequantization_amd import drivers as D
    torch.manual_seed(seed)
    qnn = D.build_qnn("resnet18", wb, ab, w_scale_method="max", device="cuda")
    x = torch.randn(*BATCH, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(x)
    g = torch.Generator().manual_seed(seed + 2)
    for bn, blk in qnn.named_modules():
        if not isinstance(blk, Q.BaseQuantBlock):
            continue
        for n, m in blk.named_modules():
            if isinstance(m, Q.QuantModule):
                D.build_ShiftedChannelQuantLayer(qnn, f".{bn}.{n}", m, 1.0, shiftTarget=list(SHIFT))
                q = m.weight_quantizer
                q.init_v(x=m.org_weight.data.clone().detach())
                # what the reconstruction would learn: a target of its own per (co, ci) (init_v
                # alone starts nearly every channel on the same one)
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


@pytest.fixture(scope="module", params=FORMS, ids=lambda f: f"W{f[0]}A{f[1]}")
def net(Q, request):
    wb, ab = request.param
    qnn, x = shifted(Q, wb, ab)
    with torch.no_grad():
        decoded = qnn(x).clone()
    return qnn, x, decoded, wb, ab


def layer_names(Q, qnn):
    names = [n for n, m in qnn.named_modules() if isinstance(m, Q.QuantModule)]
    want = plain_int8_names(names)
    assert len(names) == 21 and len(want) == 18
    return names, want


def test_per_ci_layers_are_planned_and_bounded(Q, net):
    from shiftedscalequantization_amd import kernels as K
    qnn, x, decoded, wb, ab = net
    mods = dict(qnn.named_modules())
    names, want = layer_names(Q, qnn)
    forms = {n: Q.dequant_form(mods[n])[1] for n in want}
    assert all(f["per_ci"] and f["col_scale"] is None for f in forms.values())
    try:
        plan = Q.enable_integer_inference(qnn, x, per_ci=True, wide=True)
        assert all(plan[n] == "int8" for n in want), {n: plan[n] for n in want if plan[n] != "int8"}
        int8 = [n for n in names if plan[n] == "int8"]
        # conditions of the setup, not measurements: real shift grids are on the route, on the
        # int8 blob at W2 and on the wide one at W4
        grids = {n: K.perci_grid(forms[n]["scale"], *mods[n].weight.shape[:2]) for n in want}
        print({n: (g[0], sorted(set(g[2].tolist()))) for n, g in grids.items()})
        assert all(g is not None and g[0] == 32 and not K.perci_plain(g) for g in grids.values())
        wide = {n: mods[n]._int_plan.prepared.wide for n in want}
        assert all(mods[n]._int_plan.prepared.centred for n in want)
        assert all(wide.values()) if wb == 4 else not any(wide.values())
        got, restore = capture_raw(qnn, int8)
        with torch.no_grad():
            logits = qnn(x)
        restore()
        rep = Q.integer_report(qnn)
        assert rep["off_grid"] == 0
        assert rep["calls"] == {n: 1 for n in int8}
        worst = assert_teacher_forced_bound(qnn, got, f"resnet18-perci-W{wb}A{ab}")
        parity_log({"test": "int_infer_perci_model", "arch": "resnet18", "w_bits": wb, "a_bits": ab,
                    "int8_layers": len(int8), "wide_layers": sum(wide.values()),
                    "grids": sorted({(g[0], tuple(sorted(set(g[2].tolist())))) for g in grids.values()}),
                    "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 9.0,
                    "max_logit_diff": float((logits - decoded).abs().max()),
                    "max_logit": float(decoded.abs().max())})
    finally:
        Q.disable_integer_inference(qnn)


def test_flags_off_keep_the_report_and_the_decoded_logits(Q, net):
    qnn, x, decoded, wb, ab = net
    names, want = layer_names(Q, qnn)
    try:
        plan, logits, rep = logits_of(Q, qnn, x)
        assert all(plan[n] == PER_CI for n in want), plan
        assert not any(v == "int8" for v in plan.values())
        assert rep == {"off_grid": 0, "calls": {}}
        assert same_bits(logits, decoded)
        # wide alone plans nothing more; per_ci alone refuses what leaves int8 as before
        plan = Q.enable_integer_inference(qnn, x, wide=True)
        assert all(plan[n] == PER_CI for n in want)
        plan = Q.enable_integer_inference(qnn, x, per_ci=True)
        if wb == 4:
            assert all(plan[n] == LEAVES for n in want), plan
        else:
            assert all(plan[n] == "int8" for n in want), plan
    finally:
        Q.disable_integer_inference(qnn)


def test_carried_plans_and_graph_replay_give_the_eager_logits(Q, net):
    qnn, x, _, wb, ab = net
    try:
        plan0, base, rep0 = logits_of(Q, qnn, x, per_ci=True, wide=True)
        plan1, carried, rep1 = logits_of(Q, qnn, x, per_ci=True, wide=True, carry_blocks=True)
        assert plan1 == plan0 and rep0["off_grid"] == 0 and rep1["off_grid"] == 0
        assert len(Q.block_carry_report(qnn)["edges"]) == 7 and len(Q.carry_report(qnn)["pairs"]) == 7
        assert same_bits(carried, base)
        graph = Q.IntegerGraph(qnn)
        first = graph(x).clone()
        again = graph(x).clone()
        assert same_bits(first, carried) and same_bits(again, carried)
        assert Q.integer_report(qnn)["off_grid"] == 0
        # split-K is never asked of a wide layer
        plan2, split, _ = logits_of(Q, qnn, x, per_ci=True, wide=True, splitk=True)
        mods = dict(qnn.named_modules())
        assert plan2 == plan0 and same_bits(split, base)
        assert all(not mods[n]._int_plan.splitk for n in plan2
                   if plan2[n] == "int8" and mods[n]._int_plan.prepared.wide)
    finally:
        Q.disable_integer_inference(qnn)


def test_export_round_trip_plans_the_same_layers(Q, net):
    from shiftedscalequantization_amd import drivers as D
    qnn, x, decoded, wb, ab = net
    try:
        plan, logits, rep = logits_of(Q, qnn, x, per_ci=True, wide=True)
        Q.disable_integer_inference(qnn)
        src = Q.export_quantized(qnn)
        torch.manual_seed(99)
        fresh = D.build_qnn("resnet18", wb, ab, w_scale_method="max", device="cuda")
        Q.load_quantized(fresh, src)
        fresh.set_quant_state(True, True)
        fresh.eval()
        with torch.no_grad():
            assert same_bits(fresh(x), decoded)
        plan_f, logits_f, rep_f = logits_of(Q, fresh, x, per_ci=True, wide=True)
        assert plan_f == plan and rep_f["off_grid"] == 0 and rep["off_grid"] == 0
        assert same_bits(logits_f, logits)
        mods, fmods = dict(qnn.named_modules()), dict(fresh.named_modules())
        # the restored plan is the live one: the same blobs and scales
        Q.enable_integer_inference(qnn, x, per_ci=True, wide=True)
        for n, v in plan.items():
            if v == "int8":
                a, b = mods[n]._int_plan, fmods[n]._int_plan
                assert a.prepared.wide == b.prepared.wide and torch.equal(a.prepared.blob, b.prepared.blob)
                assert same_bits(a.scale, b.scale)
        plan_off = Q.enable_integer_inference(fresh, x)
        assert all(plan_off[n].startswith("weight scale is per (co, ci)") for n in plan if plan[n] == "int8")
        Q.disable_integer_inference(fresh)
    finally:
        Q.disable_integer_inference(qnn)
