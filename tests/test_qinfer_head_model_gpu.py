"""The carried pooling head in whole models (quant/integer.py, carry_head=True), restored from
packed exports.  Per model: (a) the codes that enter the pool are act_encode of the carry_stem
route's last-block output with nothing off the grid, (b) the logits are, bit for bit,
qlinear_pooled(avgpool_codes(those codes)) plus the fc's bias / affine (and what else the module
applies behind its linear: its output act quantizer where that is on; the model's own K30 output
is compared with the recomputed one directly, too), (c) the raw fc output
lies within 2^-21 * sum_c mean_hw|x_hat| |W_hat| of the decoded head computed in fp64 on the host
from those codes.  The logits are NOT compared with the fp32 head's bit for bit: the head has
a numerics contract of its own.  A hook on the pool, the fc or the last block keeps the head on
the fp32 route, whose logits are carry_stem's bit for bit; disabling restores the decoded path."""
import numpy as np
import pytest
import torch

from test_qinfer_carry_model_gpu import host, parity_log, restored

pytestmark = pytest.mark.gpu
EMPTY = {"edges": [], "calls": {}, "pooled": {}, "fc": {}}


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


def same_bits(a, b):
    return np.array_equal(host(a).view(np.int32), host(b).view(np.int32))


def forward(Q, qnn, x, grouped=False, hook=None, **mode):
    """(plan, logits, integer_report, head_carry_report) of one forward; `hook`: the name of a
    module that carries a no-op forward hook during it."""
    plan = Q.enable_integer_inference(qnn, x, grouped=grouped, **mode)
    h = None
    if hook is not None:
        h = dict(qnn.named_modules())[hook].register_forward_hook(lambda m, a, out: None)
    try:
        with torch.no_grad():
            logits = qnn(x).clone()
    finally:
        if h is not None:
            h.remove()
    return plan, logits, Q.integer_report(qnn), Q.head_carry_report(qnn)


def pool_input(qnn, pool, x):
    """The tensor the pool receives in one forward (a pre-hook on a pool that no plan marks)."""
    seen = []
    h = pool.register_forward_pre_hook(lambda m, a: seen.append(a[0]))
    try:
        with torch.no_grad():
            qnn(x)
    finally:
        h.remove()
    assert len(seen) == 1
    return seen[0]


def check_model(Q, qnn, x, arch, grouped, edge, monkeypatch):
    from shiftedscalequantization_amd import kernels as K
    mods = dict(qnn.named_modules())
    prod, pool, fc = (mods[n] for n in edge)
    try:
        # the parent's best route: the fc behind the pool is refused, the head runs in fp32
        plan_s, logits_s, rep_s, head_s = forward(Q, qnn, x, grouped, carry_stem=True)
        assert head_s == EMPTY and plan_s[edge[2]] != "int8" and rep_s["off_grid"] == 0
        last_out = pool_input(qnn, pool, x)
        if getattr(last_out, "_ssq_codes", None) is not None:
            last_out = K.materialize_epi(last_out)
        assert last_out.dtype == torch.float32 and last_out.dim() == 4

        fed = []
        real = K.avgpool_codes
        monkeypatch.setattr(K, "avgpool_codes", lambda c: (fed.append(c), real(c))[1])
        raws, real_fc = [], K.qlinear_pooled
        monkeypatch.setattr(K, "qlinear_pooled", lambda *a: (raws.append(real_fc(*a)), raws[-1])[1])
        plan, logits, rep, head = forward(Q, qnn, x, grouped, carry_head=True)
        monkeypatch.setattr(K, "avgpool_codes", real)
        monkeypatch.setattr(K, "qlinear_pooled", real_fc)
        assert plan == {**plan_s, edge[2]: "int8"}
        assert head == {"edges": [edge], "calls": {edge[0]: 1}, "pooled": {edge[1]: 1},
                        "fc": {edge[2]: 1}}
        assert rep["off_grid"] == 0 and rep["calls"][edge[2]] == 1
        # (the dry forward of the planning call and the one forward above)
        assert len(fed) == 2 and torch.equal(fed[0], fed[1])
        codes = fed[1]
        p = fc._int_plan
        # (a) the carried codes are the ones act_encode derives from the carry_stem route's output
        want, bad = K.act_encode(last_out, p.delta, p.zp, p.n_bits, p.sym)
        assert int(bad.item()) == 0 and torch.equal(codes, want)
        # (b) the logits from those codes, bit for bit
        N, H, W, _ = codes.shape
        hi, lo, sp = K.avgpool_codes(codes)
        raw = K.qlinear_pooled(hi, lo, sp, p.prepared, K.head_scale(p.scale, H * W), H * W,
                               p.zp, p.n_bits, p.sym)
        # (the model's own K30 output is that raw tensor: the fc's act quantizer, where it is
        # on, does not hide a difference)
        assert len(raws) == 2 and same_bits(raws[1], raw) and fc.se_module is None
        exp = raw if fc.bias is None else raw + fc.bias.view(1, -1)
        gamma, phi = fc.affine()
        if gamma is not None:
            exp = exp * gamma + phi
        with torch.no_grad():       # the rest of QuantModule.forward behind the linear
            exp = fc.activation_function(exp)
            if fc.use_act_quant and not fc.disable_act_quant:
                exp = fc.act_quantizer(exp)
        assert tuple(logits.shape) == tuple(exp.shape) == (N, fc.weight.shape[0])
        assert same_bits(logits, exp)
        # (c) the raw fc output against the decoded head in fp64, from the codes alone
        Cc = fc.weight.shape[1]
        q = host(codes).astype(np.int64)[..., :Cc] + K.code_offset(p.n_bits, p.sym)
        xhat = ((q - p.zp).astype(np.float32) * np.float32(p.delta)).astype(np.float64)
        w64 = host(fc.weight_quantizer(fc.weight)).astype(np.float64)
        ref64 = xhat.reshape(N, H * W, Cc).mean(1) @ w64.T
        A = np.abs(xhat).reshape(N, H * W, Cc).mean(1) @ np.abs(w64).T
        err = np.abs(host(raw).astype(np.float64) - ref64)
        worst = float((err[A > 0] / A[A > 0]).max())
        drift = float((logits - logits_s).abs().max())
        parity_log({"test": "int_infer_head_model", "arch": arch, "grouped": grouped,
                    "batch": N, "plane": [H, W], "channels": Cc, "head_edge": list(edge),
                    "int8_layers": sum(v == "int8" for v in plan.values()), "layers": len(plan),
                    "worst_err_over_A_in_2^-24": worst * 2 ** 24, "bound_in_2^-24": 8.0,
                    "max_logit_drift_from_fp32_head": drift,
                    "max_logit": float(logits.abs().max()), "off_grid": rep["off_grid"]})
        assert np.all(err <= 2.0 ** -21 * A), worst * 2 ** 24
        return logits_s, logits
    finally:
        Q.disable_integer_inference(qnn)


R18_EDGE = ("model.layer4.1", "model.avgpool", "model.fc")


@pytest.fixture(scope="module")
def r18(Q):
    qnn, x = restored(Q, "resnet18", 11, (8, 3, 64, 64))
    with torch.no_grad():
        decoded = qnn(x).clone()
    return qnn, x, decoded


def test_resnet18_head_on_codes(Q, r18, monkeypatch):
    qnn, x, _ = r18
    check_model(Q, qnn, x, "resnet18", False, R18_EDGE, monkeypatch)
    # the last block's identity residual arrives as codes and its tail emits them
    try:
        Q.enable_integer_inference(qnn, x, carry_head=True)
        with torch.no_grad():
            qnn(x)
        blk = Q.block_carry_report(qnn)
        assert blk["residual"]["model.layer4.0"] == "fp32" and "model.layer4.1" not in blk["calls"]
        assert qnn.model.layer4[1]._int_tail.residual == "codes"
    finally:
        Q.disable_integer_inference(qnn)


def test_resnet50_head_on_codes(Q, monkeypatch):
    """Bottleneck tail, 2048 channels."""
    qnn, x = restored(Q, "resnet50", 51, (2, 3, 64, 64))
    check_model(Q, qnn, x, "resnet50", False, ("model.layer4.2", "model.avgpool", "model.fc"),
                monkeypatch)


def test_mobilenetv2_head_on_codes(Q, monkeypatch):
    qnn, _ = restored(Q, "mobilenetv2", 31, (2, 3, 64, 64))
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(32)).cuda()
    check_model(Q, qnn, x, "mobilenetv2", True,
                ("model.features.18.0", "model.pool", "model.classifier.1"), monkeypatch)


def test_regnetx600m_grouped_head_on_codes(Q, monkeypatch):
    qnn, x = restored(Q, "regnetx_600m", 41, (2, 3, 64, 64))
    check_model(Q, qnn, x, "regnetx_600m", True, ("model.s4.b7", "model.avgpool", "model.fc"),
                monkeypatch)


@pytest.mark.parametrize("hooked", ["model.avgpool", "model.fc", "model.layer4.1"])
def test_hook_keeps_the_head_on_the_fp32_route(Q, r18, hooked):
    qnn, x, _ = r18
    try:
        logits_s = forward(Q, qnn, x, carry_stem=True)[1]
        logits = forward(Q, qnn, x, carry_head=True)[1]
        _, logits_h, rep_h, head_h = forward(Q, qnn, x, carry_head=True, hook=hooked)
        assert head_h["edges"] == [R18_EDGE]
        assert head_h["pooled"] == {"model.avgpool": 0} and head_h["fc"] == {"model.fc": 0}
        assert rep_h["off_grid"] == 0 and rep_h["calls"]["model.fc"] == 0
        assert same_bits(logits_h, logits_s)
        # without the hook the head is back on codes
        with torch.no_grad():
            again = qnn(x)
        assert Q.head_carry_report(qnn)["fc"] == {"model.fc": 1} and same_bits(again, logits)
    finally:
        Q.disable_integer_inference(qnn)


def test_hook_on_the_pool_sees_fp32(Q, r18):
    qnn, x, _ = r18
    try:
        Q.enable_integer_inference(qnn, x, carry_head=True)
        seen = []
        h = qnn.model.avgpool.register_forward_hook(
            lambda m, a, out: seen.append((out.dtype, tuple(out.shape), hasattr(out, "_ssq_pooled"))))
        try:
            with torch.no_grad():
                qnn(x)
        finally:
            h.remove()
        assert seen == [(torch.float32, (8, 512, 1, 1), False)]
    finally:
        Q.disable_integer_inference(qnn)


def test_hooked_model_at_plan_time_gets_no_head_edge(Q, r18):
    qnn, x, _ = r18
    h = qnn.model.fc.register_forward_hook(lambda m, a, out: None)
    try:
        plan = Q.enable_integer_inference(qnn, x, carry_head=True)
        assert plan["model.fc"].startswith("no head edge: a forward hook")
        assert Q.head_carry_report(qnn) == EMPTY and qnn.model.fc._int_plan is None
        plan_s = Q.enable_integer_inference(qnn, x, carry_stem=True)
        assert {k: v for k, v in plan.items() if k != "model.fc"} == \
            {k: v for k, v in plan_s.items() if k != "model.fc"}
    finally:
        h.remove()
        Q.disable_integer_inference(qnn)


def test_disable_restores_decoded_path_and_empties_the_report(Q, r18):
    qnn, x, decoded = r18
    Q.enable_integer_inference(qnn, x, carry_head=True)
    with torch.no_grad():
        qnn(x)
    assert Q.head_carry_report(qnn)["edges"] and qnn.model.avgpool._int_head is not None
    Q.disable_integer_inference(qnn)
    with torch.no_grad():
        again = qnn(x)
    assert same_bits(again, decoded)
    assert Q.head_carry_report(qnn) == EMPTY and qnn.model.avgpool._int_head is None
    assert qnn.model.layer4[1]._int_tail is None and qnn.model.fc._int_plan is None
    assert Q.integer_report(qnn) == {"off_grid": 0, "calls": {}}


def test_existing_modes_leave_the_head_report_empty(Q, r18):
    qnn, x, _ = r18
    try:
        for mode in ({}, {"carry": True}, {"carry_blocks": True}, {"carry_stem": True},
                     {"carry_head": False}):
            plan, _, rep, head = forward(Q, qnn, x, **mode)
            assert head == EMPTY and rep["off_grid"] == 0
            assert plan["model.fc"] != "int8" and qnn.model.layer4[1]._int_tail is None
    finally:
        Q.disable_integer_inference(qnn)
