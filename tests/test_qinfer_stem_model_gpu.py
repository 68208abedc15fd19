"""The carried stem in whole models (quant/integer.py, carry_stem=True), restored from packed
exports: the plan is the carry_blocks plan plus the layers behind the stem's max-pool, the one
stem edge emits once and its pool pools codes once, and the logits equal, bit for bit and with
nothing off the grid, the logits of the same plan with the stem on the fp32 route (K13, fp32
pool, K21) -- the route a forward hook on the stem, on the pool, or a caching first block puts
the forward back on.  Models without a pool keep the carry_blocks plan and its logits."""
import numpy as np
import pytest
import torch

from test_qinfer_carry_model_gpu import host, parity_log, restored

pytestmark = pytest.mark.gpu
EMPTY = {"edges": [], "calls": {}, "pooled": {}}


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


def forward(Q, qnn, x, grouped=False, hook=None, **mode):
    """(plan, logits, integer_report, stem_carry_report, block_carry_report) of one forward;
    `hook`: the name of a module that carries a no-op forward hook during it."""
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
    return plan, logits, Q.integer_report(qnn), Q.stem_carry_report(qnn), Q.block_carry_report(qnn)


def same_bits(a, b):
    return np.array_equal(host(a).view(np.int32), host(b).view(np.int32))


def log(arch, grouped, x, plan, stem, rep, differing, logits):
    parity_log({"test": "int_infer_stem_model", "arch": arch, "grouped": grouped,
                "batch": int(x.shape[0]), "int8_layers": sum(v == "int8" for v in plan.values()),
                "layers": len(plan), "stem_edges": stem["edges"], "stem_calls": stem["calls"],
                "pooled": stem["pooled"], "logits_differing_from_fp32_stem": differing,
                "off_grid": rep["off_grid"], "max_logit": float(logits.abs().max())})


@pytest.fixture(scope="module")
def r18(Q):
    qnn, x = restored(Q, "resnet18", 11, (8, 3, 64, 64))
    with torch.no_grad():
        decoded = qnn(x).clone()
    return qnn, x, decoded


@pytest.fixture(scope="module")
def mbv2(Q):
    qnn, _ = restored(Q, "mobilenetv2", 31, (2, 3, 64, 64))
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(32)).cuda()
    return qnn, x


def check_pooled_model(Q, qnn, x, arch, gained):
    """A ResNet: the plan gains `gained`, the edge is carried, and the logits equal those of the
    same plan with a hooked stem (the fp32 route)."""
    try:
        plan_b = forward(Q, qnn, x, carry_blocks=True)[0]
        plan, logits, rep, stem, blk = forward(Q, qnn, x, carry_stem=True)
        assert all(plan_b[n] != "int8" for n in gained)
        assert plan == {**plan_b, **{n: "int8" for n in gained}}
        assert stem == {"edges": [("model.conv1", ["model.maxpool"], "model.layer1")],
                        "calls": {"model.conv1": 1}, "pooled": {"model.maxpool": 1}}
        plan_h, logits_h, rep_h, stem_h, _ = forward(Q, qnn, x, carry_stem=True, hook="model.conv1")
        assert plan_h == plan and stem_h["edges"] == stem["edges"]
        assert stem_h["calls"] == {"model.conv1": 0} and stem_h["pooled"] == {"model.maxpool": 0}
        assert rep["off_grid"] == 0 and rep_h["off_grid"] == 0
        # the layers behind the pool run on the integer route either way
        assert all(rep["calls"][n] == 1 and rep_h["calls"][n] == 1 for n in gained)
        differing = int((host(logits).view(np.int32) != host(logits_h).view(np.int32)).sum())
        log(arch, False, x, plan, stem, rep, differing, logits)
        assert differing == 0
        return plan, logits, blk
    finally:
        Q.disable_integer_inference(qnn)


def test_resnet18_stem_carried_logits_equal_fp32_stem(Q, r18):
    qnn, x, _ = r18
    plan, _, blk = check_pooled_model(Q, qnn, x, "resnet18", ["model.layer1.0.conv1"])
    assert len(plan) == 21 and sum(v == "int8" for v in plan.values()) == 19
    # layer1.0's identity residual arrives as codes
    assert blk["residual"]["model.layer1.0"] == "codes" and blk["calls"]["model.layer1.0"] == 1


def test_resnet50_stem_carried_logits_equal_fp32_stem(Q):
    qnn, x = restored(Q, "resnet50", 51, (2, 3, 64, 64))
    check_pooled_model(Q, qnn, x, "resnet50",
                       ["model.layer1.0.conv1", "model.layer1.0.downsample"])


@pytest.mark.parametrize("hooked", ["model.maxpool", "model.layer1", "model.layer1.0",
                                    "model.layer1.0.conv1"])
def test_hook_behind_the_stem_keeps_it_on_the_fp32_route(Q, r18, hooked):
    qnn, x, _ = r18
    try:
        logits = forward(Q, qnn, x, carry_stem=True)[1]
        _, logits_h, rep_h, stem_h, _ = forward(Q, qnn, x, carry_stem=True, hook=hooked)
        assert stem_h["calls"] == {"model.conv1": 0} and stem_h["pooled"] == {"model.maxpool": 0}
        assert rep_h["off_grid"] == 0 and same_bits(logits_h, logits)
        # without the hook the stem emits again
        with torch.no_grad():
            again = qnn(x)
        assert Q.stem_carry_report(qnn)["calls"] == {"model.conv1": 1}
        assert same_bits(again, logits)
    finally:
        Q.disable_integer_inference(qnn)


def test_hook_on_the_stem_sees_fp32(Q, r18):
    qnn, x, _ = r18
    try:
        Q.enable_integer_inference(qnn, x, carry_stem=True)
        seen = []
        h = qnn.model.conv1.register_forward_hook(
            lambda m, a, out: seen.append((out.dtype, tuple(out.shape), hasattr(out, "_ssq_codes"))))
        try:
            with torch.no_grad():
                qnn(x)
        finally:
            h.remove()
        assert seen == [(torch.float32, (8, 64, 32, 32), False)]
    finally:
        Q.disable_integer_inference(qnn)


def test_first_block_that_caches_its_input_gets_fp32(Q, r18):
    qnn, x, _ = r18
    try:
        Q.enable_integer_inference(qnn, x, carry_stem=True)
        blk = dict(qnn.named_modules())["model.layer1.0"]
        blk.cache_features = 'if'
        try:
            with torch.no_grad():
                cached_run = qnn(x).clone()
            cached = blk.cached_inp_features
        finally:
            blk.cache_features = 'none'
            blk.clear_cached_features()
        assert len(cached) == 1 and cached[0].dtype == torch.float32
        assert tuple(cached[0].shape) == (x.shape[0], 64, 16, 16)
        rep = Q.stem_carry_report(qnn)
        assert rep["calls"] == {"model.conv1": 0} and rep["pooled"] == {"model.maxpool": 0}
        with torch.no_grad():
            logits = qnn(x)
        assert Q.stem_carry_report(qnn)["calls"] == {"model.conv1": 1}
        assert Q.integer_report(qnn)["off_grid"] == 0 and same_bits(cached_run, logits)
    finally:
        Q.disable_integer_inference(qnn)


def test_disable_restores_decoded_path_and_empties_the_report(Q, r18):
    qnn, x, decoded = r18
    Q.enable_integer_inference(qnn, x, carry_stem=True)
    with torch.no_grad():
        qnn(x)
    assert Q.stem_carry_report(qnn)["edges"] and qnn.model.maxpool._int_stem is not None
    Q.disable_integer_inference(qnn)
    with torch.no_grad():
        again = qnn(x)
    assert same_bits(again, decoded)
    assert Q.stem_carry_report(qnn) == EMPTY and qnn.model.maxpool._int_stem is None
    assert Q.block_carry_report(qnn) == {"edges": [], "calls": {}, "residual": {}}
    assert Q.integer_report(qnn) == {"off_grid": 0, "calls": {}}


def test_existing_modes_leave_the_stem_report_empty(Q, r18):
    qnn, x, _ = r18
    try:
        for mode in ({}, {"carry": True}, {"carry_blocks": True}, {"carry_stem": False}):
            plan, _, rep, stem, blk = forward(Q, qnn, x, **mode)
            assert stem == EMPTY and rep["off_grid"] == 0
            assert plan["model.layer1.0.conv1"] != "int8"
            if mode.get("carry_blocks"):
                assert blk["residual"]["model.layer1.0"] == "fp32"
    finally:
        Q.disable_integer_inference(qnn)


def check_poolless_model(Q, qnn, x, arch, grouped, edge):
    """No pool: the carry_blocks plan unchanged; `edge` (or no edge) and the carry_blocks
    logits."""
    try:
        plan_b, logits_b, rep_b, stem_b, blk_b = forward(Q, qnn, x, grouped, carry_blocks=True)
        plan, logits, rep, stem, blk = forward(Q, qnn, x, grouped, carry_stem=True)
        assert plan == plan_b and stem_b == EMPTY
        assert rep["off_grid"] == 0 and rep_b["off_grid"] == 0 and rep["calls"] == rep_b["calls"]
        assert blk["edges"] == blk_b["edges"] and blk["calls"] == blk_b["calls"]
        if edge is None:
            assert stem == EMPTY and blk == blk_b
        else:
            assert stem == {"edges": [edge], "calls": {edge[0]: 1}, "pooled": {}}
        differing = int((host(logits).view(np.int32) != host(logits_b).view(np.int32)).sum())
        log(arch, grouped, x, plan, stem, rep, differing, logits)
        assert differing == 0
    finally:
        Q.disable_integer_inference(qnn)


def test_mobilenetv2_grouped_stem_carried_logits_equal_carry_blocks(Q, mbv2):
    qnn, x = mbv2
    check_poolless_model(Q, qnn, x, "mobilenetv2", True,
                         ("model.features.0.0", [], "model.features.1"))


def test_mobilenetv2_ungrouped_has_no_stem_edge(Q, mbv2):
    """features.1's reader is a depthwise conv left on the decoded path."""
    qnn, x = mbv2
    check_poolless_model(Q, qnn, x, "mobilenetv2", False, None)


def test_regnetx600m_grouped_stem_carried_logits_equal_carry_blocks(Q):
    qnn, x = restored(Q, "regnetx_600m", 41, (2, 3, 64, 64))
    check_poolless_model(Q, qnn, x, "regnetx_600m", True, ("model.stem.0", [], "model.s1"))
