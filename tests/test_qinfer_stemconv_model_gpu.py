"""The fused stem in whole models (quant/integer.py, fused_stem=True): random-init ResNet-18,
MobileNetV2 and RegNetX-600M, restored from packed exports, on a (2, 3, 32, 32) batch with
carry_head=True.

The stem edge is fused and counts one fused forward per call, the stem module's conv is never
entered, the emitted bytes are K27's of K31's fp32 form, and everything behind the stem is exact:
the logits equal, bit for bit, those of the same plan without `fused_stem` whose stem conv is made
to return K31's fp32 output.  Without the keyword nothing changes.  What depends on the library
conv's summation order (how many stem codes differ from the carry_stem route's) is recorded, not
asserted."""
import numpy as np
import pytest
import torch

from test_qinfer_carry_model_gpu import host, parity_log, restored

pytestmark = pytest.mark.gpu
# arch: (seed, grouped, the stem module)
ARCHS = {"resnet18": (211, False, "model.conv1"),
         "mobilenetv2": (231, True, "model.features.0.0"),
         "regnetx_600m": (241, True, "model.stem.0")}
BATCH = (2, 3, 32, 32)


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


@pytest.fixture(scope="module", params=sorted(ARCHS))
def net(Q, request):
    arch = request.param
    seed, grouped, stem = ARCHS[arch]
    qnn, x = restored(Q, arch, seed, BATCH)
    with torch.no_grad():
        decoded = qnn(x).clone()
    yield arch, qnn, x, grouped, stem, decoded
    Q.disable_integer_inference(qnn)


def same_bits(a, b):
    return np.array_equal(host(a).view(np.int32), host(b).view(np.int32))


def run(qnn, x):
    with torch.no_grad():
        return qnn(x).clone()


def stem_edge(qnn):
    from shiftedscalequantization_amd.quant.integer import StemEdge
    edge, = [e for e in qnn._int_edges if type(e) is StemEdge]
    return edge


def test_fused_stem_forward(Q, net, monkeypatch):
    from shiftedscalequantization_amd import kernels as K
    arch, qnn, x, grouped, stem, _ = net
    plan = Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, fused_stem=True)
    mod = dict(qnn.named_modules())[stem]
    edge = stem_edge(qnn)
    assert edge.at is mod and plan[stem] != "int8"
    rep = Q.stem_carry_report(qnn)
    assert rep["fused"] == {stem: 0} and rep["unfused"] == {stem: {}} and rep["calls"] == {stem: 0}
    # the stem module's conv (F.conv2d / kernels.conv2d, both behind QuantModule._conv) is never entered
    entered = []
    conv = mod._conv
    monkeypatch.setattr(mod, "_conv", lambda *a, **k: entered.append(1) or conv(*a, **k))
    conv2d = K.conv2d
    monkeypatch.setattr(K, "conv2d", lambda inp, *a, **k: (entered.append(2) if inp is x else None)
                        or conv2d(inp, *a, **k))
    logits = run(qnn, x)
    again = run(qnn, x)
    rep = Q.stem_carry_report(qnn)
    assert rep["fused"] == {stem: 2} and rep["calls"] == {stem: 2} and rep["unfused"] == {stem: {}}
    assert not entered and same_bits(logits, again)
    assert Q.integer_report(qnn)["off_grid"] == 0 and bool(torch.isfinite(logits).all())
    assert len(Q.head_carry_report(qnn)["edges"]) == 1
    # the emitted bytes: K27 on K31's fp32 form
    with torch.no_grad():
        codes = edge.emit(x)
        y = K.stem_conv(x, edge.blob, edge.stride, edge.padding)
        gamma, phi = mod.affine()
        want = K.epilogue_codes(y, mod.bias, gamma, phi, mod.act_code(), *edge.grid, edge.counter)
    assert codes.dtype == torch.int8 and codes._ssq_codes.shape == tuple(y.shape)
    assert torch.equal(codes, want) and not entered
    # K27's route for the same edge, from the library conv: recorded, not asserted
    with torch.no_grad():
        lib_codes = type(edge).emit(edge, x)
        w = mod._weight_bias()[0]
        y_lib = mod._conv(x, w)
        mag = K.stem_conv(x.abs(), K.stem_weight_prepare(w.abs()), edge.stride, edge.padding)
    assert len(entered) == 2                     # (the counter does see the unfused route)
    diff = (codes.to(torch.int32) - lib_codes.to(torch.int32)).abs()
    parity_log({"test": "int_infer_fused_stem_parity", "arch": arch, "batch": list(BATCH),
                "stem": stem, "stem_code_bytes": int(codes.numel()),
                "share_differing_from_carry_stem": float((diff != 0).float().mean()),
                "max_code_difference": int(diff.max()),
                "max_abs_err_over_mag_in_2^-24": float(((y - y_lib).abs() / mag.clamp_min(1e-30)).max()
                                                       * 2.0 ** 24),
                "logits_max": float(logits.abs().max())})
    Q.disable_integer_inference(qnn)


def test_everything_behind_the_stem_is_exact(Q, net, monkeypatch):
    from shiftedscalequantization_amd import kernels as K
    arch, qnn, x, grouped, stem, _ = net
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, fused_stem=True)
    edge = stem_edge(qnn)
    blob, stride, padding = edge.blob, edge.stride, edge.padding
    fused = run(qnn, x)
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, fused_stem=False)
    mod = dict(qnn.named_modules())[stem]
    assert "fused" not in Q.stem_carry_report(qnn) and "emit" not in stem_edge(qnn).__dict__
    monkeypatch.setattr(mod, "forward_raw",
                        lambda inp: (K.stem_conv(inp, blob, stride, padding), mod._weight_bias()[1]))
    unfused = run(qnn, x)
    assert Q.stem_carry_report(qnn)["calls"] == {stem: 1}
    assert same_bits(fused, unfused)
    Q.disable_integer_inference(qnn)


def test_without_the_keyword_nothing_changes(Q, net):
    arch, qnn, x, grouped, stem, decoded = net
    plan0 = Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True)
    parent, rep0 = run(qnn, x), Q.stem_carry_report(qnn)
    plan1 = Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, fused_stem=False)
    off, rep1 = run(qnn, x), Q.stem_carry_report(qnn)
    assert plan0 == plan1 and rep0 == rep1 and set(rep1) == {"edges", "calls", "pooled"}
    assert same_bits(parent, off)
    # fused_stem alone plans no edge
    Q.enable_integer_inference(qnn, x, grouped=grouped, fused_stem=True)
    rep = Q.stem_carry_report(qnn)
    assert rep["edges"] == [] and rep["fused"] == {} and rep["unfused"] == {}
    # disable restores the module
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, fused_stem=True)
    run(qnn, x)
    Q.disable_integer_inference(qnn)
    assert dict(qnn.named_modules())[stem]._int_stem is None
    assert set(Q.stem_carry_report(qnn)) == {"edges", "calls", "pooled"}
    assert same_bits(run(qnn, x), decoded)


def test_graph_replay_equals_eager(Q, net):
    arch, qnn, x, grouped, stem, _ = net
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, fused_stem=True)
    eager = run(qnn, x)
    assert Q.stem_carry_report(qnn)["fused"] == {stem: 1}
    graph = Q.IntegerGraph(qnn)
    first = graph(x).clone()
    second = graph(x).clone()
    assert same_bits(first, eager) and same_bits(second, eager)
    rep = Q.stem_carry_report(qnn)
    assert rep["fused"] == {stem: 3} and rep["calls"] == {stem: 3}
    assert Q.integer_report(qnn)["off_grid"] == 0
    Q.disable_integer_inference(qnn)


def test_runtime_reasons_keep_a_forward_on_k27(Q, net, monkeypatch):
    arch, qnn, x, grouped, stem, _ = net
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, fused_stem=True)
    fused = run(qnn, x)
    strided = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)      # same values
    assert not strided.is_contiguous() and torch.equal(strided, x)
    run(qnn, strided)
    monkeypatch.setenv("SSQ_STEM_FUSED", "0")
    run(qnn, x)
    monkeypatch.setenv("SSQ_STEM_FUSED", "1")
    assert same_bits(run(qnn, x), fused)
    rep = Q.stem_carry_report(qnn)
    assert rep["fused"] == {stem: 2} and rep["calls"] == {stem: 4}
    why = rep["unfused"][stem]
    assert sorted(why.values()) == [1, 1] and any("non-contiguous" in k for k in why)
    assert any("shape rule" in k for k in why)
    Q.disable_integer_inference(qnn)
