"""uint8 images in whole models (quant/integer.py, image_u8=(mean, std)): random-init ResNet-18,
MobileNetV2 and RegNetX-600M, restored from packed exports, on a (2, 3, 32, 32) uint8 batch with
carry_head=True.

A uint8 forward runs the stem on K32 and is counted; its stem codes are, byte for byte, those of
the numpy restatement of the contract (test_qinfer_stemu8_host.u8_stem_ref + the epilogue's
restatement) from the stem's own packed codes, and the logits equal, bit for bit, those of the
same plan fed those codes.  An fp32 input gives the logits of the plan without the keyword.  A
column-scaled stem is reported as refused and still runs.  How many stem codes differ from the
fp32 routes' is recorded, not asserted.  The host shape rule is taken out of the way with its A/B
knob (SSQ_STEM_U8=1): it takes K32 for ResNet's 7x7 stem at this size and not for the 3x3 stems,
which the last test asserts."""
import numpy as np
import pytest
import torch

from test_qinfer_carry_host import quant_codes, ref_pre_quant, stored
from test_qinfer_carry_model_gpu import host, parity_log, restored
from test_qinfer_stemu8_host import u8_stem_ref

pytestmark = pytest.mark.gpu
# arch: (seed, grouped, the stem module)
ARCHS = {"resnet18": (311, False, "model.conv1"),
         "mobilenetv2": (331, True, "model.features.0.0"),
         "regnetx_600m": (341, True, "model.stem.0")}
BATCH = (2, 3, 32, 32)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


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
    u = torch.randint(0, 256, BATCH, generator=torch.Generator().manual_seed(seed + 2),
                      dtype=torch.uint8).cuda()
    yield arch, qnn, x, u, grouped, stem
    Q.disable_integer_inference(qnn)


@pytest.fixture(autouse=True)
def k32_whatever_the_shape_rule(monkeypatch):
    monkeypatch.setenv("SSQ_STEM_U8", "1")


def same_bits(a, b):
    return np.array_equal(host(a).view(np.int32), host(b).view(np.int32))


def run(qnn, x):
    with torch.no_grad():
        return qnn(x).clone()


def stem_edge(qnn):
    from shiftedscalequantization_amd.quant.integer import StemEdge
    edge, = [e for e in qnn._int_edges if type(e) is StemEdge]
    return edge


def normalised(u):
    mean = torch.tensor(MEAN, device=u.device).reshape(1, 3, 1, 1)
    std = torch.tensor(STD, device=u.device).reshape(1, 3, 1, 1)
    return (u.float() / 255 - mean) / std


def restated_codes(mod, edge, u):
    """The stem's codes for the uint8 batch from the numpy restatement alone."""
    f = mod.weight_quantizer.fields()
    assert f["n_bits"] == 8 and f["col_scale"] is None
    Co, Ci, R, S = (int(v) for v in mod.weight.shape)
    qw = host(mod.weight_quantizer.packed)[:Co * Ci * R * S].astype(np.int64) + f["qmin"]
    qw = qw.reshape(Co, Ci, R, S)
    zw = np.rint(host(f["zero_point"]).reshape(-1)).astype(np.int64)
    kw = mod.fwd_kwargs
    y = u8_stem_ref(host(u), qw, zw, f["qmin"], host(f["scale"]), MEAN, STD, tuple(kw["stride"]),
                    tuple(kw["padding"]))
    gamma, phi = mod.affine()
    opt = lambda t: None if t is None else host(t).reshape(-1)
    t = ref_pre_quant(y, opt(mod.bias), opt(gamma), opt(phi), mod.act_code())
    delta, zp, n_bits, sym = edge.grid
    q, nbad = quant_codes(t, delta, zp, n_bits, sym)
    assert nbad == 0
    return stored(q, n_bits, sym), y.shape


def test_u8_forward_runs_k32_and_everything_behind_it_is_exact(Q, net, monkeypatch):
    from shiftedscalequantization_amd import kernels as K
    arch, qnn, x, u, grouped, stem = net
    plan = Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, image_u8=(MEAN, STD))
    mod = dict(qnn.named_modules())[stem]
    edge = stem_edge(qnn)
    assert edge.at is mod and plan[stem] != "int8" and qnn._int_u8 == {stem: None}
    rep = Q.stem_carry_report(qnn)
    assert rep["u8"] == {stem: 0} and rep["un_u8"] == {stem: {}} and "fused" not in rep
    logits = run(qnn, u)
    again = run(qnn, u)
    rep = Q.stem_carry_report(qnn)
    assert rep["u8"] == {stem: 2} and rep["calls"] == {stem: 2} and rep["un_u8"] == {stem: {}}
    assert same_bits(logits, again) and bool(torch.isfinite(logits).all())
    assert Q.integer_report(qnn)["off_grid"] == 0
    assert len(Q.head_carry_report(qnn)["edges"]) == 1
    # the emitted bytes are the numpy restatement's
    with torch.no_grad():
        codes = edge.emit(u)
    want, yshape = restated_codes(mod, edge, u)
    assert codes.dtype == torch.int8 and codes._ssq_codes.shape == yshape
    assert np.array_equal(host(codes), want)
    # the same plan fed the restatement's codes: the same logits, bit for bit
    fed = K.carried(torch.as_tensor(want).cuda(), yshape, *edge.grid)
    monkeypatch.setattr(edge, "emit", lambda inp: fed)
    assert same_bits(run(qnn, u), logits)
    monkeypatch.undo()
    # against the fp32 pipeline through the same plan: recorded, not asserted
    with torch.no_grad():
        f32_codes = edge.emit(normalised(u))
    f32_logits = run(qnn, normalised(u))
    diff = (codes.to(torch.int32) - f32_codes.to(torch.int32)).abs()
    parity_log({"test": "int_infer_u8_stem_model_parity", "arch": arch, "batch": list(BATCH),
                "stem": stem, "stem_code_bytes": int(codes.numel()),
                "share_differing_from_fp32_route": float((diff != 0).float().mean()),
                "max_code_difference": int(diff.max()),
                "max_abs_logit_difference": float((logits - f32_logits).abs().max()),
                "logits_max": float(logits.abs().max())})
    Q.disable_integer_inference(qnn)


def test_an_fp32_input_takes_the_plan_without_the_keyword(Q, net):
    arch, qnn, x, u, grouped, stem = net
    for fused in (False, True):
        plan0 = Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, fused_stem=fused)
        parent, rep0 = run(qnn, x), Q.stem_carry_report(qnn)
        plan1 = Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True,
                                           fused_stem=fused, image_u8=(MEAN, STD))
        with_kw, rep1 = run(qnn, x), Q.stem_carry_report(qnn)
        assert plan0 == plan1 and same_bits(parent, with_kw)
        assert rep1["u8"] == {stem: 0} and rep1["un_u8"] == {stem: {}}
        assert {k: v for k, v in rep1.items() if k not in ("u8", "un_u8")} == rep0
        # a uint8 sample plans the same route
        plan2 = Q.enable_integer_inference(qnn, u, grouped=grouped, carry_head=True,
                                           fused_stem=fused, image_u8=(MEAN, STD))
        assert plan2 == plan1
    with pytest.raises(ValueError, match="stem edge"):
        Q.enable_integer_inference(qnn, x, grouped=grouped, carry_blocks=True, image_u8=(MEAN, STD))
    Q.disable_integer_inference(qnn)
    assert set(Q.stem_carry_report(qnn)) == {"edges", "calls", "pooled"}
    assert dict(qnn.named_modules())[stem]._int_stem is None and qnn._int_u8 is None


def test_runtime_reasons_normalise_on_the_device(Q, net, monkeypatch):
    arch, qnn, x, u, grouped, stem = net
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, image_u8=(MEAN, STD))
    on_k32 = run(qnn, u)
    f32 = run(qnn, normalised(u))
    strided = u.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)      # same values
    assert not strided.is_contiguous() and torch.equal(strided, u)
    assert same_bits(run(qnn, strided), f32)
    nhwc = u.contiguous(memory_format=torch.channels_last)
    assert same_bits(run(qnn, nhwc), f32)
    monkeypatch.setenv("SSQ_STEM_U8", "0")
    assert same_bits(run(qnn, u), f32)
    monkeypatch.setenv("SSQ_STEM_U8", "1")
    assert same_bits(run(qnn, u), on_k32)
    rep = Q.stem_carry_report(qnn)
    assert rep["u8"] == {stem: 2}
    why = rep["un_u8"][stem]
    assert sorted(why.values()) == [1, 1, 1]
    assert any("non-contiguous" in k for k in why) and any("channels-last" in k for k in why)
    assert any("shape rule" in k for k in why)
    Q.disable_integer_inference(qnn)


def test_graph_replay_of_a_uint8_forward(Q, net):
    arch, qnn, x, u, grouped, stem = net
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, image_u8=(MEAN, STD))
    eager = run(qnn, u)
    graph = Q.IntegerGraph(qnn)
    first = graph(u).clone()
    second = graph(u).clone()
    assert same_bits(first, eager) and same_bits(second, eager)
    rep = Q.stem_carry_report(qnn)
    assert rep["u8"] == {stem: 3} and rep["calls"] == {stem: 3}
    assert Q.integer_report(qnn)["off_grid"] == 0
    Q.disable_integer_inference(qnn)


def test_without_an_installed_stem_edge_the_keyword_is_an_error_and_leaves_no_plan(Q, net, monkeypatch):
    """A model that declares no stem chain gets no stem edge: the keyword says so instead of
    leaving a uint8 batch to fail inside the conv."""
    arch, qnn, x, u, grouped, stem = net
    monkeypatch.setattr(qnn.model, "stem_chain", lambda: [], raising=False)
    with pytest.raises(ValueError, match="no stem edge installed"):
        Q.enable_integer_inference(qnn, x, grouped=grouped, carry_stem=True, image_u8=(MEAN, STD))
    assert qnn._int_edges == [] and qnn._int_u8 is None
    assert all(m._int_plan is None for m in qnn.modules() if isinstance(m, Q.QuantModule))
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_stem=True)     # without it: no error
    assert Q.stem_carry_report(qnn)["edges"] == []
    Q.disable_integer_inference(qnn)


def test_normalised_forwards_are_counted_under_graph_replay(Q, net, monkeypatch):
    arch, qnn, x, u, grouped, stem = net
    from shiftedscalequantization_amd.quant.integer import U8_SHAPE_RULE
    monkeypatch.setenv("SSQ_STEM_U8", "0")
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, image_u8=(MEAN, STD))
    eager = run(qnn, normalised(u))
    graph = Q.IntegerGraph(qnn)
    first = graph(u).clone()
    second = graph(u).clone()
    assert same_bits(first, eager) and same_bits(second, eager)
    rep = Q.stem_carry_report(qnn)
    assert rep["u8"] == {stem: 0} and rep["un_u8"] == {stem: {U8_SHAPE_RULE: 2}}
    assert rep["calls"] == {stem: 3}
    Q.disable_integer_inference(qnn)


def test_the_fp32_emit_is_asked_once_per_normalised_forward(Q, net, monkeypatch):
    """A fused edge that declines the normalised batch (a hook on the stem: the edge does not
    carry) counts its own reason once, and the module's fp32 forward runs."""
    arch, qnn, x, u, grouped, stem = net
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, fused_stem=True,
                               image_u8=(MEAN, STD))
    mod = dict(qnn.named_modules())[stem]
    monkeypatch.setenv("SSQ_STEM_U8", "0")
    monkeypatch.setenv("SSQ_STEM_FUSED", "0")
    h = mod.register_forward_hook(lambda *a: None)
    try:
        out = run(qnn, u)
        want = run(qnn, normalised(u))
    finally:
        h.remove()
    rep = Q.stem_carry_report(qnn)
    assert same_bits(out, want) and rep["calls"] == {stem: 0} and rep["u8"] == {stem: 0}
    assert list(rep["un_u8"][stem].values()) == [1]
    assert list(rep["unfused"][stem].values()) == [2]        # one per forward: the uint8, the fp32
    Q.disable_integer_inference(qnn)


def test_a_column_scaled_stem_is_refused_and_still_runs(Q):
    """The export's form of a ChannelQuantMSE stem: a PackedWeight with a column scale (the
    calibration drivers leave the 8-bit stem on its own quantizer, so the scale is set here)."""
    from test_qinfer_colscale_model_gpu import is_colscaled
    qnn, x = restored(Q, "resnet18", 351, BATCH)
    stem = "model.conv1"
    mod = dict(qnn.named_modules())[stem]
    q = mod.weight_quantizer
    col = torch.ones(3 * 7 * 7, device=x.device)
    col[1::2] = 0.5
    q.col_scale, q.kind, q._w = col, "channelquantmse", None
    assert is_colscaled(Q, mod) and q.fields()["col_scale"] is col
    u = torch.randint(0, 256, BATCH, generator=torch.Generator().manual_seed(353),
                      dtype=torch.uint8).cuda()
    Q.enable_integer_inference(qnn, x, carry_head=True, image_u8=(MEAN, STD))
    edge = stem_edge(qnn)
    assert edge.at is mod and "column scale" in qnn._int_u8[stem]
    rep = Q.stem_carry_report(qnn)
    (why, n), = rep["un_u8"][stem].items()
    assert "column scale" in why and n == 0 and rep["u8"] == {stem: 0}
    out = run(qnn, u)
    rep = Q.stem_carry_report(qnn)
    assert rep["un_u8"][stem] == {why: 1} and rep["u8"] == {stem: 0} and rep["calls"] == {stem: 1}
    # it ran the fp32 route on the batch normalised on the device
    assert same_bits(out, run(qnn, normalised(u)))
    Q.disable_integer_inference(qnn)


def test_the_shape_rule_decides_without_the_knob(Q, net, monkeypatch):
    arch, qnn, x, u, grouped, stem = net
    monkeypatch.delenv("SSQ_STEM_U8")
    Q.enable_integer_inference(qnn, x, grouped=grouped, carry_head=True, image_u8=(MEAN, STD))
    run(qnn, u)
    rep = Q.stem_carry_report(qnn)
    if arch == "resnet18":                      # 7x7 taps on 2 x 16 x 16 output pixels
        assert rep["u8"] == {stem: 1} and rep["un_u8"] == {stem: {}}
    else:                                       # a 3x3 stem: 9 of the k step's 64 taps
        (why, n), = rep["un_u8"][stem].items()
        assert "shape rule" in why and n == 1 and rep["u8"] == {stem: 0}
    assert rep["calls"] == {stem: 1}
    Q.disable_integer_inference(qnn)
