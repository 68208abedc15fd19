"""Integer inference of whole models (quant/integer.py): planning marks the interior layers
"int8" and gives every other layer a reason, the integer forward calls each planned layer once
with nothing off the grid, every planned layer's raw output stays within the derived fp32 bound
of the fp64 convolution of its own captured input (teacher-forced), ineligible weight forms keep
the decoded path bit for bit, and disabling restores the decoded outputs bit for bit."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


def host(t):
    return t.detach().cpu().numpy()


def parity_log(rec):
    """Print the figure and append it to $SSQ_PARITY_LOG (jsonl) when set."""
    print(json.dumps(rec))
    path = os.environ.get("SSQ_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def calibrated(arch, seed, batch):
    """A QuantModel with weight and act quantization on and every quantizer initialised by one
    forward of a seeded batch (no reconstruction), and that batch."""
    from shiftedscalequantization_amd import drivers as D
    torch.manual_seed(seed)
    qnn = D.build_qnn(arch, 2, 4, device="cuda")
    qnn.set_quant_state(True, True)
    x = torch.randn(*batch, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    with torch.no_grad():
        qnn(x)
    return qnn, x


def restored(Q, arch, seed, batch):
    """export_quantized -> load_quantized into a fresh model of the same architecture."""
    from shiftedscalequantization_amd import drivers as D
    qnn, x = calibrated(arch, seed, batch)
    src = Q.export_quantized(qnn)
    torch.manual_seed(seed + 77)
    fresh = D.build_qnn(arch, 2, 4, device="cuda")
    Q.load_quantized(fresh, src)
    fresh.set_quant_state(True, True)
    return fresh.eval(), x


def capture_raw(qnn, names):
    """Record (input, raw conv output) of the named QuantModules' next forward_raw."""
    got, undo = {}, []
    mods = dict(qnn.named_modules())
    for n in names:
        m, orig = mods[n], mods[n].forward_raw

        def wrapped(inp, _n=n, _orig=orig):
            out, bias = _orig(inp)
            got[_n] = (inp.detach().clone(), out.detach().clone())
            return out, bias
        m.forward_raw = wrapped
        undo.append(m)

    def restore():
        for m in undo:
            del m.forward_raw
    return got, restore


def assert_teacher_forced_bound(qnn, got, tag):
    """|raw - conv64(input, W_hat)| <= 2^-21 * conv64(|input|, |W_hat|) for every captured
    layer (the bound of test_qinfer_gpu.py's fp-path test); returns the worst ratio."""
    mods = dict(qnn.named_modules())
    worst = 0.0
    for n, (inp, raw) in got.items():
        m = mods[n]
        w = m.weight_quantizer(m.weight).detach().double().cpu()
        xd = inp.double().cpu()
        kw = dict(stride=m.fwd_kwargs["stride"], padding=m.fwd_kwargs["padding"])
        ref = F.conv2d(xd, w, **kw).numpy()
        A = F.conv2d(xd.abs(), w.abs(), **kw).numpy()
        err = np.abs(host(raw).astype(np.float64) - ref)
        nz = A > 0
        ratio = float((err[nz] / A[nz]).max()) if nz.any() else 0.0
        assert np.all(err <= 2.0 ** -21 * A), (tag, n, ratio * 2 ** 24)
        worst = max(worst, ratio)
    return worst


@pytest.fixture(scope="module")
def r18(Q):
    qnn, x = restored(Q, "resnet18", 11, (8, 3, 64, 64))
    with torch.no_grad():
        decoded = qnn(x).clone()
    return qnn, x, decoded


def test_resnet18_plan_and_forward(Q, r18):
    qnn, x, decoded = r18
    report = Q.enable_integer_inference(qnn, x)
    try:
        names = [n for n, m in qnn.named_modules() if isinstance(m, Q.QuantModule)]
        assert set(report) == set(names) and len(names) == 21
        int8 = [n for n in names if report[n] == "int8"]
        for n in names:
            if n.endswith("conv2") or n.endswith("downsample") or \
                    (n.endswith("conv1") and "layer" in n and not n.endswith("layer1.0.conv1")):
                assert report[n] == "int8", (n, report[n])
        assert len(int8) >= 18
        stem, fc = names[0], names[-1]
        for n in (stem, fc):
            assert report[n] != "int8" and isinstance(report[n], str) and report[n]
        got, restore = capture_raw(qnn, int8)
        with torch.no_grad():
            logits = qnn(x)
        restore()
        rep = Q.integer_report(qnn)
        assert rep["off_grid"] == 0
        assert rep["calls"] == {n: 1 for n in int8}
        assert set(got) == set(int8)
        worst = assert_teacher_forced_bound(qnn, got, "resnet18")
        # logits are logged, not asserted: a one-ulp conv difference can flip an act code
        flips = []
        got_d, restore_d = capture_raw(qnn, int8)
        Q.disable_integer_inference(qnn)
        with torch.no_grad():
            qnn(x)
        restore_d()
        for n in int8:
            a, b = got[n][0], got_d[n][0]
            flips.append(float((a != b).float().mean()))
        parity_log({"test": "int_infer_model", "arch": "resnet18", "int8_layers": len(int8),
                    "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 8.0,
                    "max_logit_diff": float((logits - decoded).abs().max()),
                    "max_logit": float(decoded.abs().max()),
                    "share_of_differing_act_inputs": max(flips),
                    "share_by_layer": [round(f, 6) for f in flips]})
    finally:
        Q.disable_integer_inference(qnn)


def test_disable_restores_decoded_path_bit_exactly(Q, r18):
    qnn, x, decoded = r18
    Q.enable_integer_inference(qnn, x)
    with torch.no_grad():
        qnn(x)
    Q.disable_integer_inference(qnn)
    with torch.no_grad():
        again = qnn(x)
    np.testing.assert_array_equal(host(again).view(np.int32), host(decoded).view(np.int32))
    assert Q.integer_report(qnn) == {"off_grid": 0, "calls": {}}


def test_live_model_is_planned_through_pack_encode(Q):
    """A live calibrated model (UniformAffineQuantizer weights, not PackedWeight) takes its
    codes through dequant_form + pack_encode and meets the same per-layer bound."""
    qnn, x = calibrated("resnet18", 23, (2, 3, 64, 64))
    qnn.eval()
    report = Q.enable_integer_inference(qnn, x)
    int8 = [n for n, v in report.items() if v == "int8"]
    assert len(int8) >= 18
    got, restore = capture_raw(qnn, int8)
    with torch.no_grad():
        qnn(x)
    restore()
    assert Q.integer_report(qnn)["off_grid"] == 0
    assert_teacher_forced_bound(qnn, got, "resnet18-live")


@pytest.mark.parametrize("form", ["per_ci", "col_scale"])
def test_ineligible_weight_forms_keep_the_decoded_path(Q, r18, form):
    from shiftedscalequantization_amd import kernels as K
    qnn, x, _ = r18
    name = "model.layer2.0.conv2"
    m = dict(qnn.named_modules())[name]
    keep = m.weight_quantizer
    Co, Ci, k = m.weight.shape[0], m.weight.shape[1], m.weight.shape[2] * m.weight.shape[3]
    g = torch.Generator().manual_seed(5)
    q = torch.randint(0, 4, tuple(m.weight.shape), generator=g).float().cuda()
    zp = torch.randint(0, 4, (Co,), generator=g).float().cuda()
    if form == "per_ci":
        d1 = (torch.rand(Co, Ci, generator=g) * 0.01 + 1e-3).cuda()
        d2 = None
        what = (q - zp.view(-1, 1, 1, 1)) * d1.view(Co, Ci, 1, 1)
    else:
        d1 = (torch.rand(Co, generator=g) * 0.01 + 1e-3).cuda()
        d2 = (torch.rand(Ci * k, generator=g) + 0.5).cuda()
        what = ((q - zp.view(-1, 1, 1, 1)) * d1.view(Co, 1, 1, 1)) * d2.view(1, Ci, *m.weight.shape[2:])
    packed, bad = K.pack_encode(what, zp, d1, form == "per_ci", d2, 2, 0, 3)
    assert bad == 0
    m.weight_quantizer = Q.PackedWeight(packed, tuple(m.weight.shape), zp, d1.reshape(-1),
                                        form == "per_ci", d2, 2, 0, 3, "test:" + form)
    try:
        with torch.no_grad():
            decoded = qnn(x).clone()
        report = Q.enable_integer_inference(qnn, x)
        assert report[name] != "int8" and ("co, ci" in report[name] or "column" in report[name])
        assert report["model.layer2.0.conv1"] == "int8"
        # the layer itself stays on the decoded path: its raw output is the decoded model's
        got, restore = capture_raw(qnn, [name])
        with torch.no_grad():
            qnn(x)
        restore()
        inp, raw = got[name]
        want = F.conv2d(inp, m.weight_quantizer(m.weight), **m.fwd_kwargs)
        np.testing.assert_array_equal(host(raw).view(np.int32), host(want).view(np.int32))
        assert name not in Q.integer_report(qnn)["calls"]
        Q.disable_integer_inference(qnn)
        with torch.no_grad():
            again = qnn(x)
        np.testing.assert_array_equal(host(again).view(np.int32), host(decoded).view(np.int32))
    finally:
        Q.disable_integer_inference(qnn)
        m.weight_quantizer = keep


def test_mobilenetv2_grouped_layers_stay_decoded(Q):
    qnn, _ = restored(Q, "mobilenetv2", 31, (2, 3, 64, 64))
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(32)).cuda()
    report = Q.enable_integer_inference(qnn, x)
    mods = dict(qnn.named_modules())
    dw = [n for n, m in mods.items() if isinstance(m, Q.QuantModule)
          and m.fwd_kwargs.get("groups", 1) != 1]
    assert dw and all("group" in report[n] for n in dw)
    int8 = [n for n, v in report.items() if v == "int8"]
    assert int8 and all(tuple(mods[n].weight.shape[2:]) == (1, 1) for n in int8)
    # every 1x1 conv that reads a block's or a layer's act quantizer output is planned
    one_by_one = [n for n, m in mods.items() if isinstance(m, Q.QuantModule)
                  and m.weight.dim() == 4 and tuple(m.weight.shape[2:]) == (1, 1)]
    assert len(int8) >= len(one_by_one) - 2
    got, restore = capture_raw(qnn, int8)
    with torch.no_grad():
        qnn(x)
    restore()
    rep = Q.integer_report(qnn)
    assert rep["off_grid"] == 0 and rep["calls"] == {n: 1 for n in int8}
    worst = assert_teacher_forced_bound(qnn, got, "mobilenetv2")
    bits = sorted({mods[n]._int_plan.n_bits for n in int8})
    parity_log({"test": "int_infer_model", "arch": "mobilenetv2", "int8_layers": len(int8),
                "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 8.0,
                "act_bits_seen": bits})
    Q.disable_integer_inference(qnn)
