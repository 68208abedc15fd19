"""Integer inference of whole models with grouped=True (quant/integer.py, K24-K26): MobileNetV2's
depthwise convs and RegNetX's grouped f.b convs are planned "int8" with their kind, the integer
forward calls each planned layer once with nothing off the grid, every planned layer's raw
output stays within the derived fp32 bound of the fp64 grouped convolution of its own captured
input (teacher-forced), disabling restores the decoded outputs bit for bit, and the default
arguments refuse the grouped layers as before."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_qinfer_model_gpu import capture_raw, host, parity_log, restored

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


def teacher_forced_bound(qnn, got, tag):
    """|raw - conv64(input, W_hat)| <= 2^-21 * conv64(|input|, |W_hat|) for every captured
    layer, `groups` passed to the fp64 conv; returns the worst ratio."""
    mods = dict(qnn.named_modules())
    worst = 0.0
    for n, (inp, raw) in got.items():
        m = mods[n]
        w = m.weight_quantizer(m.weight).detach().double().cpu()
        xd = inp.double().cpu()
        kw = dict(stride=m.fwd_kwargs["stride"], padding=m.fwd_kwargs["padding"],
                  groups=m.fwd_kwargs["groups"])
        ref = F.conv2d(xd, w, **kw).numpy()
        A = F.conv2d(xd.abs(), w.abs(), **kw).numpy()
        err = np.abs(host(raw).astype(np.float64) - ref)
        nz = A > 0
        ratio = float((err[nz] / A[nz]).max()) if nz.any() else 0.0
        assert np.all(err <= 2.0 ** -21 * A), (tag, n, ratio * 2 ** 24)
        worst = max(worst, ratio)
    return worst


def grouped_layers(Q, qnn):
    return [n for n, m in qnn.named_modules() if isinstance(m, Q.QuantModule)
            and m.fwd_kwargs.get("groups", 1) != 1]


def integer_forward(Q, qnn, x, int8, arch, decoded):
    """One integer forward: calls, off-grid count and the per-layer bound asserted; the logit
    drift and the share of differing act codes per layer logged, not asserted (a one-ulp conv
    difference can flip an act code)."""
    got, restore = capture_raw(qnn, int8)
    with torch.no_grad():
        logits = qnn(x)
    restore()
    rep = Q.integer_report(qnn)
    assert rep["off_grid"] == 0
    assert rep["calls"] == {n: 1 for n in int8}
    assert set(got) == set(int8)
    worst = teacher_forced_bound(qnn, got, arch)
    got_d, restore_d = capture_raw(qnn, int8)
    Q.disable_integer_inference(qnn)
    with torch.no_grad():
        again = qnn(x)
    restore_d()
    flips = [float((got[n][0] != got_d[n][0]).float().mean()) for n in int8]
    return logits, again, worst, flips


def test_mobilenetv2_depthwise_layers_run_on_codes(Q):
    qnn, _ = restored(Q, "mobilenetv2", 31, (2, 3, 64, 64))
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(32)).cuda()
    with torch.no_grad():
        decoded = qnn(x).clone()
    mods = dict(qnn.named_modules())
    dw = grouped_layers(Q, qnn)
    assert len(dw) == 17
    report = Q.enable_integer_inference(qnn, x, grouped=True)
    try:
        assert not any("group" in v for v in report.values())
        for n in dw:
            assert report[n] == "int8", (n, report[n])
            plan = mods[n]._int_plan
            assert plan.kind == "depthwise" and plan.groups == mods[n].fwd_kwargs["groups"]
        int8 = [n for n, v in report.items() if v == "int8"]
        kinds = {n: mods[n]._int_plan.kind for n in int8}
        assert set(kinds.values()) == {"dense", "depthwise"}
        assert all(kinds[n] == "dense" for n in int8 if n not in dw)
        logits, again, worst, flips = integer_forward(Q, qnn, x, int8, "mobilenetv2", decoded)
        # disabled inside integer_forward: the decoded logits are back bit for bit
        np.testing.assert_array_equal(host(again).view(np.int32), host(decoded).view(np.int32))
        assert Q.integer_report(qnn) == {"off_grid": 0, "calls": {}}
        parity_log({"test": "int_infer_grouped_model", "arch": "mobilenetv2",
                    "int8_layers": len(int8), "depthwise_layers": len(dw),
                    "layers": len(report),
                    "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 8.0,
                    "max_logit_diff": float((logits - decoded).abs().max()),
                    "max_logit": float(decoded.abs().max()),
                    "share_of_differing_act_inputs": max(flips),
                    "share_by_layer": [round(f, 6) for f in flips]})
        # the default arguments keep refusing the grouped layers
        report = Q.enable_integer_inference(qnn, x)
        assert all("group" in report[n] for n in dw)
        assert all(mods[n]._int_plan is None for n in dw)
    finally:
        Q.disable_integer_inference(qnn)


def test_regnetx_600m_grouped_layers_run_on_codes(Q):
    qnn, _ = restored(Q, "regnetx_600m", 41, (2, 3, 64, 64))
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(42)).cuda()
    with torch.no_grad():
        decoded = qnn(x).clone()
    mods = dict(qnn.named_modules())
    gl = grouped_layers(Q, qnn)
    conv2 = [n for n, m in mods.items() if isinstance(m, Q.QuantModule) and n.endswith(".conv2")]
    assert conv2 and set(conv2) == set(gl)
    assert {mods[n].fwd_kwargs["groups"] for n in gl} == {2, 4, 10, 22}
    assert {mods[n].weight.shape[1] for n in gl} == {24}
    report = Q.enable_integer_inference(qnn, x, grouped=True)
    try:
        assert not any("group" in v for v in report.values())
        for n in conv2:
            assert report[n] == "int8", (n, report[n])
            plan = mods[n]._int_plan
            assert plan.kind == "grouped" and plan.groups == mods[n].fwd_kwargs["groups"]
        int8 = [n for n, v in report.items() if v == "int8"]
        logits, again, worst, flips = integer_forward(Q, qnn, x, int8, "regnetx_600m", decoded)
        np.testing.assert_array_equal(host(again).view(np.int32), host(decoded).view(np.int32))
        parity_log({"test": "int_infer_grouped_model", "arch": "regnetx_600m",
                    "int8_layers": len(int8), "grouped_layers": len(gl), "layers": len(report),
                    "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 8.0,
                    "max_logit_diff": float((logits - decoded).abs().max()),
                    "max_logit": float(decoded.abs().max()),
                    "share_of_differing_act_inputs": max(flips),
                    "share_by_layer": [round(f, 6) for f in flips]})
    finally:
        Q.disable_integer_inference(qnn)
