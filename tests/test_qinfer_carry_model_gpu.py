"""Carried int8 codes in whole models (quant/integer.py, carry=True): the carried pairs are the
blocks' interior chains whose two layers are planned, every producer emits codes once with
nothing off the grid, and the logits equal the uncarried integer forward's bit for bit -- a
carried code is the code the consumer's act_encode re-derives whenever that counts nothing
off-grid.  A hook on a producer puts that forward back on the uncarried route; disabling
restores the decoded path."""
import json
import os

import numpy as np
import pytest
import torch

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


def expected_pairs(Q, qnn, report):
    """The interior_chain() pairs whose two modules are planned "int8", as names."""
    from shiftedscalequantization_amd.quant.quant_block import BaseQuantBlock
    names = {m: n for n, m in qnn.named_modules() if isinstance(m, Q.QuantModule)}
    pairs = []
    for blk in qnn.modules():
        if isinstance(blk, BaseQuantBlock):
            for prod, cons in blk.interior_chain():
                if report[names[prod]] == "int8" and report[names[cons]] == "int8":
                    pairs.append((names[prod], names[cons]))
    return pairs


def integer_logits(Q, qnn, x, grouped, carry):
    """(plan, logits, integer_report, carry_report) of one integer forward."""
    plan = Q.enable_integer_inference(qnn, x, grouped=grouped, carry=carry)
    with torch.no_grad():
        logits = qnn(x).clone()
    return plan, logits, Q.integer_report(qnn), Q.carry_report(qnn)


def check_model(Q, qnn, x, arch, grouped):
    try:
        plan0, plain, rep0, car0 = integer_logits(Q, qnn, x, grouped, False)
        assert car0 == {"pairs": [], "calls": {}} and rep0["off_grid"] == 0
        plan, logits, rep, car = integer_logits(Q, qnn, x, grouped, True)
        assert plan == plan0
        want = expected_pairs(Q, qnn, plan)
        assert sorted(car["pairs"]) == sorted(want)
        assert car["calls"] == {p: 1 for p, _ in want}          # every producer emitted once
        assert rep["off_grid"] == 0 and rep["calls"] == rep0["calls"]
        assert np.array_equal(host(logits).view(np.int32), host(plain).view(np.int32))
        parity_log({"test": "int_infer_carry_model", "arch": arch, "grouped": grouped,
                    "int8_layers": sum(v == "int8" for v in plan.values()),
                    "carried_pairs": len(want), "logits_differing_from_uncarried": 0,
                    "off_grid": rep["off_grid"], "max_logit": float(plain.abs().max())})
        return want
    finally:
        Q.disable_integer_inference(qnn)


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


def test_resnet18_carried_logits_equal_uncarried(Q, r18):
    qnn, x, _ = r18
    pairs = check_model(Q, qnn, x, "resnet18", False)
    # one per BasicBlock but layer1.0, whose conv1 reads the max pool, not an act quantizer
    assert len(pairs) == 7 and all(p.endswith("conv1") and c.endswith("conv2") for p, c in pairs)
    assert not any("layer1.0" in p for p, _ in pairs)


def test_mobilenetv2_grouped_carried_logits_equal_uncarried(Q, mbv2):
    qnn, x = mbv2
    pairs = check_model(Q, qnn, x, "mobilenetv2", True)
    mods = dict(qnn.named_modules())
    dw = {n for n, m in mods.items() if isinstance(m, Q.QuantModule)
          and m.fwd_kwargs.get("groups", 1) != 1}
    # the depthwise convs appear as consumers and as producers
    assert {c for _, c in pairs} & dw and {p for p, _ in pairs} & dw


def test_mobilenetv2_ungrouped_carries_nothing(Q, mbv2):
    qnn, x = mbv2
    assert check_model(Q, qnn, x, "mobilenetv2", False) == []


def test_regnetx600m_grouped_carried_logits_equal_uncarried(Q):
    qnn, x = restored(Q, "regnetx_600m", 41, (2, 3, 64, 64))
    pairs = check_model(Q, qnn, x, "regnetx_600m", True)
    grouped = {n for n, m in qnn.named_modules() if isinstance(m, Q.QuantModule)
               and m.fwd_kwargs.get("groups", 1) != 1}
    assert {c for _, c in pairs} & grouped and {p for p, _ in pairs} & grouped


def test_hook_on_a_producer_takes_the_uncarried_route(Q, r18):
    qnn, x, _ = r18
    try:
        _, plain, _, _ = integer_logits(Q, qnn, x, False, False)
        Q.enable_integer_inference(qnn, x, carry=True)
        pairs = Q.carry_report(qnn)["pairs"]
        name = pairs[2][0]
        prod = dict(qnn.named_modules())[name]
        seen = []
        h = prod.register_forward_hook(lambda m, a, out: seen.append((out.dtype, tuple(out.shape))))
        try:
            with torch.no_grad():
                logits = qnn(x)
        finally:
            h.remove()
        calls = Q.carry_report(qnn)["calls"]
        assert calls[name] == 0 and all(calls[p] == 1 for p, _ in pairs if p != name)
        # the hook saw the fp32 NCHW activation, not codes
        assert len(seen) == 1 and seen[0][0] == torch.float32 and seen[0][1][0] == x.shape[0]
        assert Q.integer_report(qnn)["off_grid"] == 0
        assert np.array_equal(host(logits).view(np.int32), host(plain).view(np.int32))
        # without the hook the producer carries again
        with torch.no_grad():
            again = qnn(x)
        assert Q.carry_report(qnn)["calls"][name] == 1
        assert np.array_equal(host(again).view(np.int32), host(plain).view(np.int32))
    finally:
        Q.disable_integer_inference(qnn)


def test_disable_restores_decoded_path_and_empties_reports(Q, r18):
    qnn, x, decoded = r18
    Q.enable_integer_inference(qnn, x, carry=True)
    with torch.no_grad():
        qnn(x)
    assert Q.carry_report(qnn)["pairs"]
    Q.disable_integer_inference(qnn)
    with torch.no_grad():
        again = qnn(x)
    assert np.array_equal(host(again).view(np.int32), host(decoded).view(np.int32))
    assert Q.carry_report(qnn) == {"pairs": [], "calls": {}}
    assert Q.integer_report(qnn) == {"off_grid": 0, "calls": {}}
