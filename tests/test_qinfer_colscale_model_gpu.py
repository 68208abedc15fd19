"""Integer inference of whole column-scaled models (quant/integer.py, colscale=True): a random
ResNet-18 at W2A4 on a (2, 3, 64, 64) batch whose block convs have every second input channel
scaled by 0.25 before the weight-quant init, so that channelShift_wMSE(level=4, threshold=2.0)
picks column scales below 1.  With colscale=True the 18 layers the plain form plans are planned,
each within 9 * 2^-24 of the fp64 convolution of its own input (teacher-forced); with it off the
report strings and the logits are the decoded model's; carried plans give the uncarried logits
bit for bit; an all-ones scale (level = 1) takes the plain K22 blob; an export / load round trip
plans the same layers with equal logits; MobileNetV2 with grouped=True plans its depthwise and
1x1 column-scaled layers."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_qinfer_model_gpu import capture_raw, host, parity_log

pytestmark = pytest.mark.gpu
BATCH = (2, 3, 64, 64)


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


def same_bits(a, b):
    return np.array_equal(host(a).view(np.int32), host(b).view(np.int32))


def shrink_columns(Q, qnn):
    """Every second input channel of the block convs times 0.25 (the first kernel row of a
    depthwise conv, whose columns are its taps): the range test then fits a smaller scale."""
    for blk in qnn.modules():
        if not isinstance(blk, Q.BaseQuantBlock):
            continue
        for m in blk.modules():
            if isinstance(m, Q.QuantModule) and m.weight.dim() == 4:
                for w in (m.weight.data, m.org_weight):
                    if w.shape[1] == 1:
                        w[:, :, 0, :] *= 0.25
                    else:
                        w[:, 1::2] *= 0.25


def column_scaled(Q, arch, seed, level, batch=BATCH, shrink=True):
    """channelShift_wMSE on a seeded random model, act quantization on and initialised on the
    seeded sample; (model, sample)."""
    from shiftedscalequantization_amd import drivers as D
    torch.manual_seed(seed)
    qnn = D.build_qnn(arch, 2, 4, w_scale_method="max", device="cuda")
    if shrink:
        shrink_columns(Q, qnn)
    x = torch.randn(*batch, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    fc = [n for n, m in qnn.named_modules() if isinstance(m, Q.QuantModule)][-1]
    D.channelShift_wMSE(qnn, x, level=level, threshold=2.0, layerDisabled=["." + fc])
    qnn.set_quant_state(True, True)
    with torch.no_grad():
        qnn(x)
    return qnn.eval(), x


def is_colscaled(Q, m):
    from shiftedscalequantization_amd.quant.channelQuantMSE import ChannelQuantMSE
    q = m.weight_quantizer
    return isinstance(q, ChannelQuantMSE) or getattr(q, "col_scale", None) is not None


def plain_int8_names(names):
    """The layers the plain form plans at ResNet-18 (test_qinfer_model_gpu.py)."""
    return [n for n in names if n.endswith("conv2") or n.endswith("downsample")
            or (n.endswith("conv1") and "layer" in n and not n.endswith("layer1.0.conv1"))]


def assert_teacher_forced_bound(qnn, got, tag, bound=9.0):
    """|raw - conv64(input, W_hat)| <= 9 * 2^-24 * conv64(|input|, |W_hat|) for every captured
    layer (the bound of test_qinfer_colscale_gpu.py); returns the worst ratio."""
    mods = dict(qnn.named_modules())
    worst = 0.0
    for n, (inp, raw) in got.items():
        m = mods[n]
        w = m.weight_quantizer(m.weight).detach().double().cpu()
        xd = inp.double().cpu()
        kw = dict(stride=m.fwd_kwargs["stride"], padding=m.fwd_kwargs["padding"],
                  groups=m.fwd_kwargs.get("groups", 1))
        ref = F.conv2d(xd, w, **kw).numpy()
        A = F.conv2d(xd.abs(), w.abs(), **kw).numpy()
        err = np.abs(host(raw).astype(np.float64) - ref)
        nz = A > 0
        ratio = float((err[nz] / A[nz]).max()) if nz.any() else 0.0
        print({"layer": n, "err_over_A_in_2^-24": ratio * 2 ** 24})
        assert np.all(err <= bound * 2.0 ** -24 * A), (tag, n, ratio * 2 ** 24)
        worst = max(worst, ratio)
    return worst


def logits_of(Q, qnn, x, **mode):
    plan = Q.enable_integer_inference(qnn, x, **mode)
    with torch.no_grad():
        out = qnn(x).clone()
    return plan, out, Q.integer_report(qnn)


def strip_carries(Q, qnn):
    """The installed plan with every layer on its own: no codes carried anywhere."""
    for e in qnn._int_edges:
        e.install(False)
    del qnn._int_edges[:]


@pytest.fixture(scope="module")
def r18(Q):
    qnn, x = column_scaled(Q, "resnet18", 11, 4)
    with torch.no_grad():
        decoded = qnn(x).clone()
    return qnn, x, decoded


def test_resnet18_column_scaled_layers_are_planned_and_bounded(Q, r18):
    from shiftedscalequantization_amd import kernels as K
    qnn, x, decoded = r18
    mods = dict(qnn.named_modules())
    names = [n for n, m in mods.items() if isinstance(m, Q.QuantModule)]
    want = plain_int8_names(names)
    assert len(names) == 21 and len(want) == 18
    assert all(is_colscaled(Q, mods[n]) for n in want)
    try:
        plan = Q.enable_integer_inference(qnn, x, colscale=True)
        assert all(plan[n] == "int8" for n in want), {n: plan[n] for n in want if plan[n] != "int8"}
        int8 = [n for n in names if plan[n] == "int8"]
        # conditions of the setup, not measurements: a real column grid is on the route
        ks = {n: mods[n]._int_plan.prepared.centred for n in int8}
        grids = {n: K.colscale_grid(mods[n].weight_quantizer.inp_scale) for n in int8
                 if is_colscaled(Q, mods[n])}
        assert any(g is not None and len(set(g[1].tolist())) >= 2 for g in grids.values())
        assert any(ks.values())
        got, restore = capture_raw(qnn, int8)
        with torch.no_grad():
            logits = qnn(x)
        restore()
        rep = Q.integer_report(qnn)
        assert rep["off_grid"] == 0
        assert rep["calls"] == {n: 1 for n in int8}
        worst = assert_teacher_forced_bound(qnn, got, "resnet18-colscale")
        parity_log({"test": "int_infer_colscale_model", "arch": "resnet18", "int8_layers": len(int8),
                    "centred_layers": sum(ks.values()),
                    "grids": {n: (g[0], sorted(set(g[1].tolist()))) for n, g in grids.items()
                              if g is not None},
                    "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 9.0,
                    "max_logit_diff": float((logits - decoded).abs().max()),
                    "max_logit": float(decoded.abs().max())})
    finally:
        Q.disable_integer_inference(qnn)


def test_colscale_off_keeps_the_report_and_the_decoded_logits(Q, r18):
    qnn, x, decoded = r18
    mods = dict(qnn.named_modules())
    names = [n for n, m in mods.items() if isinstance(m, Q.QuantModule)]
    try:
        plan, logits, rep = logits_of(Q, qnn, x)
        for n in plain_int8_names(names):
            assert plan[n] == "weight has a column scale (channelquantmse)", (n, plan[n])
        assert not any(v == "int8" for v in plan.values())
        assert rep == {"off_grid": 0, "calls": {}}
        assert same_bits(logits, decoded)
    finally:
        Q.disable_integer_inference(qnn)


def test_carried_plans_give_the_uncarried_logits(Q, r18):
    """The carried plans' logits are those of the uncarried colscale=True plan.  carry_blocks
    adds no layer to it; carry_stem also plans the layer behind the max-pool, so it is compared
    with its own plan with every carry taken out as well."""
    qnn, x, _ = r18
    try:
        plan0, base, rep0 = logits_of(Q, qnn, x, colscale=True)
        plan1, carried, rep1 = logits_of(Q, qnn, x, colscale=True, carry_blocks=True)
        assert plan1 == plan0 and rep0["off_grid"] == 0 and rep1["off_grid"] == 0
        assert len(Q.block_carry_report(qnn)["edges"]) == 7 and len(Q.carry_report(qnn)["pairs"]) == 7
        assert same_bits(carried, base)
        plan2, stem, rep2 = logits_of(Q, qnn, x, colscale=True, carry_stem=True)
        assert Q.stem_carry_report(qnn)["calls"] == {"model.conv1": 1}
        assert rep2["off_grid"] == 0
        gained = [n for n in plan2 if plan2[n] == "int8" and plan0[n] != "int8"]
        assert gained == ["model.layer1.0.conv1"]
        print({"stem_carried_logits_differing_from_the_18_layer_plan":
               int((host(stem).view(np.int32) != host(base).view(np.int32)).sum())})
        assert same_bits(stem, base)
        strip_carries(Q, qnn)
        with torch.no_grad():
            alone = qnn(x).clone()
        assert Q.integer_report(qnn)["off_grid"] == 0
        assert Q.integer_report(qnn)["calls"]["model.layer1.0.conv1"] == 2
        assert same_bits(stem, alone)
    finally:
        Q.disable_integer_inference(qnn)


def test_all_ones_scale_takes_the_plain_route(Q):
    """level = 1: every column scale is 1, the layers take K22's blob (not centred), and the
    logits equal those of the same model with plain weights of the same codes."""
    from shiftedscalequantization_amd import kernels as K
    qnn, x = column_scaled(Q, "resnet18", 11, 1)
    mods = dict(qnn.named_modules())
    names = [n for n, m in mods.items() if isinstance(m, Q.QuantModule)]
    try:
        plan, logits, rep = logits_of(Q, qnn, x, colscale=True)
        int8 = [n for n in names if plan[n] == "int8"]
        assert set(plain_int8_names(names)) <= set(int8) and rep["off_grid"] == 0
        assert not any(mods[n]._int_plan.prepared.centred for n in int8)
        Q.disable_integer_inference(qnn)
        # the same codes as plain weights
        for n in names:
            m = mods[n]
            if not is_colscaled(Q, m):
                continue
            what, f = Q.dequant_form(m)
            assert bool((f["col_scale"] == 1).all())
            packed, bad = K.pack_encode(what, f["zero_point"], f["scale"], False, None, f["n_bits"],
                                        f["qmin"], f["qmax"])
            assert bad == 0
            m.weight_quantizer = Q.PackedWeight(packed, tuple(m.weight.shape), f["zero_point"],
                                                f["scale"], False, None, f["n_bits"], f["qmin"],
                                                f["qmax"], "test:plain")
        plan_p, logits_p, rep_p = logits_of(Q, qnn, x)
        assert [n for n in names if plan_p[n] == "int8"] == int8 and rep_p["off_grid"] == 0
        assert same_bits(logits, logits_p)
    finally:
        Q.disable_integer_inference(qnn)


def test_export_round_trip_plans_the_same_layers(Q, r18):
    from shiftedscalequantization_amd import drivers as D
    qnn, x, decoded = r18
    try:
        plan, logits, rep = logits_of(Q, qnn, x, colscale=True)
        Q.disable_integer_inference(qnn)
        src = Q.export_quantized(qnn)
        torch.manual_seed(99)
        fresh = D.build_qnn("resnet18", 2, 4, w_scale_method="max", device="cuda")
        Q.load_quantized(fresh, src)
        fresh.set_quant_state(True, True)
        fresh.eval()
        with torch.no_grad():
            assert same_bits(fresh(x), decoded)
        plan_f, logits_f, rep_f = logits_of(Q, fresh, x, colscale=True)
        assert plan_f == plan and rep_f["off_grid"] == 0 and rep["off_grid"] == 0
        assert same_bits(logits_f, logits)
        # and off, the restored model reports the column scale too
        plan_off = Q.enable_integer_inference(fresh, x)
        assert all("column scale" in plan_off[n] for n in plan if plan[n] == "int8")
        Q.disable_integer_inference(fresh)
    finally:
        Q.disable_integer_inference(qnn)


def test_a_scale_off_the_grid_keeps_the_decoded_path(Q, r18):
    """A column scale that is on no grid k / L, L <= 127, is refused with colscale=True as well,
    the reason naming the column scale; a W4 layer whose scaled weight leaves int8 is refused
    with a reason that says so."""
    qnn, x, _ = r18
    name = "model.layer2.0.conv2"
    m = dict(qnn.named_modules())[name]
    q = m.weight_quantizer
    keep = q.inp_scale
    try:
        g = torch.Generator().manual_seed(5)
        q.inp_scale = (torch.rand(keep.shape, generator=g) + 0.5).cuda()
        plan = Q.enable_integer_inference(qnn, x, colscale=True)
        assert plan[name] != "int8" and "column scale" in plan[name]
        assert plan["model.layer2.0.conv1"] == "int8"
        # (q - z) up to 3 at W2: k = 127 makes |m| = 381
        q.inp_scale = torch.where(torch.rand(keep.shape, generator=g).cuda() < 0.5, 1.0, 1.0 / 127.0)
        plan = Q.enable_integer_inference(qnn, x, colscale=True)
        assert plan[name] != "int8" and "leaves int8" in plan[name]
    finally:
        q.inp_scale = keep
        Q.disable_integer_inference(qnn)


def test_mobilenetv2_grouped_column_scaled_layers(Q):
    qnn, x = column_scaled(Q, "mobilenetv2", 31, 4, batch=(2, 3, 32, 32))
    mods = dict(qnn.named_modules())
    try:
        plan = Q.enable_integer_inference(qnn, x, grouped=True, colscale=True)
        int8 = [n for n, v in plan.items() if v == "int8"]
        dw = [n for n in int8 if mods[n].fwd_kwargs.get("groups", 1) != 1]
        pw = [n for n in int8 if mods[n].weight.dim() == 4 and tuple(mods[n].weight.shape[2:]) == (1, 1)]
        assert dw and pw and all(is_colscaled(Q, mods[n]) for n in dw + pw)
        # conditions of the setup: column grids with two values on both kinds of layer
        assert any(mods[n]._int_plan.prepared.centred for n in dw)
        assert any(mods[n]._int_plan.prepared.centred for n in pw)
        assert all(mods[n]._int_plan.kind == "depthwise" for n in dw)
        refused = {n: v for n, v in plan.items() if v != "int8" and "column scale" in v}
        assert not refused, refused
        got, restore = capture_raw(qnn, int8)
        with torch.no_grad():
            qnn(x)
        restore()
        rep = Q.integer_report(qnn)
        assert rep["off_grid"] == 0 and rep["calls"] == {n: 1 for n in int8}
        worst = assert_teacher_forced_bound(qnn, got, "mobilenetv2-colscale")
        parity_log({"test": "int_infer_colscale_model", "arch": "mobilenetv2", "grouped": True,
                    "int8_layers": len(int8), "depthwise": len(dw),
                    "centred_layers": sum(mods[n]._int_plan.prepared.centred for n in int8),
                    "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 9.0})
    finally:
        Q.disable_integer_inference(qnn)


def test_driver_test_branch_runs_the_route(Q, capsys):
    """`main_imagenet.py --test True --int_infer_colscale`: channelShift_wMSE, then the act
    quantizers, the plan printed and one batch on the integer route; without the flag the
    --test branch returns after channelShift_wMSE as before."""
    import main_imagenet
    argv = ["--arch", "resnet18", "--test", "True", "--num_samples", "16", "--mse_level", "4",
            "--mse_threshold", "2.0", "--w_scale_method", "max"]
    qnn = main_imagenet.main(argv)
    out = capsys.readouterr().out
    assert "channelShift_wMSE (level 4" in out and "integer inference" not in out
    assert all(getattr(m, "_int_plan", None) is None for m in qnn.modules())
    qnn = main_imagenet.main(argv + ["--int_infer_colscale", "--int_infer_carry_stem"])
    out = capsys.readouterr().out
    assert "channelShift_wMSE (level 4" in out
    assert "integer inference: 19 of 21 layers on int8 codes" in out
    assert "integer inference: 0 off-grid activations" in out
    assert "column scale" not in out
    planned = [m for m in qnn.modules() if getattr(m, "_int_plan", None) is not None]
    assert len(planned) == 19 and Q.stem_carry_report(qnn)["calls"] == {"model.conv1": 1}
