"""uint8 image views in a whole model (quant/integer.py, StemEdge.emit_u8 on a view that is not
dense NCHW): a random-init ResNet-18 restored from its packed export, on a (2, 3, 32, 32) uint8
batch with carry_head=True.

An interleaved batch, an RGBA batch's first three channels and a crop of a larger frame give,
eagerly and through IntegerGraph, the logits of the dense NCHW batch bit for bit, and
`integer_report()["u8_form"]` counts how each was staged.  The two shape rules are taken out of
the way with their A/B knobs (SSQ_STEM_U8=1, SSQ_STEM_U8_STRIDED=1); SSQ_STEM_U8_STRIDED=0 copies
every view dense for the same logits, and auto leaves this unmeasured plane on the route it had."""
import pytest
import torch

from test_qinfer_carry_model_gpu import restored
from test_qinfer_stemu8_model_gpu import MEAN, STD, normalised, run, same_bits

pytestmark = pytest.mark.gpu
BATCH = (2, 3, 32, 32)
STEM = "model.conv1"


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


@pytest.fixture(scope="module")
def net(Q):
    qnn, x = restored(Q, "resnet18", 511, BATCH)
    u = torch.randint(0, 256, BATCH, generator=torch.Generator().manual_seed(513),
                      dtype=torch.uint8).cuda()
    yield qnn, x, u
    Q.disable_integer_inference(qnn)


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("SSQ_STEM_U8", "1")
    monkeypatch.setenv("SSQ_STEM_U8_STRIDED", "1")


def views(u):
    """{name: (the view, its staging form)}; everything around the image is 255."""
    N, C, H, W = u.shape
    px = u.permute(0, 2, 3, 1)
    rgba = torch.cat([px, torch.full_like(px[..., :1], 255)], dim=3).contiguous()
    fr = torch.full((N, C, H + 5, W + 7), 255, dtype=torch.uint8, device=u.device)
    fr[:, :, 2:2 + H, 3:3 + W] = u
    hfr = torch.full((N, H + 5, W + 7, C), 255, dtype=torch.uint8, device=u.device)
    hfr[:, 2:2 + H, 3:3 + W, :] = px
    out = {"hwc": (px.contiguous().permute(0, 3, 1, 2), "interleaved"),
           "rgba": (rgba[..., :3].permute(0, 3, 1, 2), "interleaved"),
           "crop": (fr[:, :, 2:2 + H, 3:3 + W], "planar"),
           "hwc crop": (hfr[:, 2:2 + H, 3:3 + W, :].permute(0, 3, 1, 2), "interleaved"),
           "swapped": (u.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), "generic")}
    for v, _ in out.values():
        assert torch.equal(v, u) and not v.is_contiguous()
    return out


def enable(Q, qnn, x):
    Q.enable_integer_inference(qnn, x, carry_head=True, image_u8=(MEAN, STD))


def test_every_view_gives_the_dense_logits_eagerly(Q, net):
    qnn, x, u = net
    enable(Q, qnn, x)
    assert Q.integer_report(qnn)["u8_form"] == {STEM: {}}
    dense = run(qnn, u)
    assert Q.integer_report(qnn)["u8_form"] == {STEM: {"planar": 1}}
    want = {"planar": 1}
    for name, (v, form) in views(u).items():
        assert same_bits(run(qnn, v), dense), name
        want[form] = want.get(form, 0) + 1
        assert Q.integer_report(qnn)["u8_form"] == {STEM: want}, name
    rep = Q.stem_carry_report(qnn)
    assert rep["u8"] == {STEM: 6} and rep["un_u8"] == {STEM: {}} and rep["calls"] == {STEM: 6}
    assert want == {"planar": 2, "interleaved": 3, "generic": 1}
    assert Q.integer_report(qnn)["off_grid"] == 0
    Q.disable_integer_inference(qnn)
    assert "u8_form" not in Q.integer_report(qnn)


def test_every_view_gives_the_dense_logits_through_the_graph(Q, net):
    qnn, x, u = net
    enable(Q, qnn, x)
    dense, other = run(qnn, u), run(qnn, 255 - u)
    enable(Q, qnn, x)                                # the counters from zero
    graph = Q.IntegerGraph(qnn)
    vs = views(u)
    # the static input keeps the sample's dimension order: a dense HWC batch replays interleaved,
    # 4-byte pixels and a crop from a dense buffer of their own order
    staged = {"hwc": "interleaved", "rgba": "interleaved", "crop": "planar",
              "hwc crop": "interleaved"}
    assert len(staged) == graph.MAX_SHAPES
    want = {}
    for name, form in staged.items():
        first = graph(vs[name][0]).clone()
        second = graph(vs[name][0]).clone()
        assert same_bits(first, dense) and same_bits(second, dense), name
        want[form] = want.get(form, 0) + 2
        assert Q.integer_report(qnn)["u8_form"] == {STEM: want}, name
    # the same shape under other strides is another key; another batch of a layout replays its capture
    assert graph.shapes() == [BATCH] * 4
    hwc2 = (255 - u).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert same_bits(graph(hwc2).clone(), other) and same_bits(graph(vs["hwc"][0]).clone(), dense)
    assert graph.shapes() == [BATCH] * 4
    rep = Q.stem_carry_report(qnn)
    assert rep["un_u8"] == {STEM: {}} and rep["u8"] == {STEM: 10} and rep["calls"] == {STEM: 10}
    assert Q.integer_report(qnn)["u8_form"] == {STEM: {"interleaved": 8, "planar": 2}}
    assert Q.integer_report(qnn)["off_grid"] == 0
    Q.disable_integer_inference(qnn)


def test_strided_knob_0_copies_every_view(Q, net, monkeypatch):
    qnn, x, u = net
    enable(Q, qnn, x)
    dense = run(qnn, u)
    monkeypatch.setenv("SSQ_STEM_U8_STRIDED", "0")
    n = 0
    for name, (v, _) in views(u).items():
        assert same_bits(run(qnn, v), dense), name
        n += 1
    assert same_bits(run(qnn, u), dense)
    assert Q.integer_report(qnn)["u8_form"] == {STEM: {"planar": 2, "copied": n}}
    rep = Q.stem_carry_report(qnn)
    assert rep["u8"] == {STEM: n + 2} and rep["un_u8"] == {STEM: {}}
    Q.disable_integer_inference(qnn)


def test_auto_leaves_an_unmeasured_plane_on_the_route_it_had(Q, net, monkeypatch):
    """No in-place form was measured at 32 x 32: auto normalises the view for the fp32 emit, by
    the reasons it gave before views were read in place."""
    qnn, x, u = net
    monkeypatch.delenv("SSQ_STEM_U8_STRIDED")
    enable(Q, qnn, x)
    f32 = run(qnn, normalised(u))
    vs = views(u)
    for name in ("hwc", "crop"):
        assert same_bits(run(qnn, vs[name][0]), f32), name
    rep = Q.stem_carry_report(qnn)
    why = rep["un_u8"][STEM]
    assert rep["u8"] == {STEM: 0} and sorted(why.values()) == [1, 1]
    assert any("channels-last" in k for k in why) and any("non-contiguous" in k for k in why)
    assert Q.integer_report(qnn)["u8_form"] == {STEM: {}}
    Q.disable_integer_inference(qnn)
