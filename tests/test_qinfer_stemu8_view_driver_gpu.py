"""main_imagenet.run_integer_inference under --int_infer_u8_layout and --int_infer_u8_frame: a
restored random-init ResNet-18 on the one synthetic (2, 3, 32, 32) uint8 batch, handed to the
plan as an interleaved view, as the first three channels of 4-byte pixels, and as the centre crop
of larger frames.  The run goes to the end and prints the count of K32 forwards by staging form.
The shape rules are taken out of the way with their A/B knobs; without the view's knob the run
goes to the end all the same, on the route an unmeasured plane had."""
import pytest
import torch

from test_qinfer_carry_model_gpu import restored

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
    qnn, x = restored(Q, "resnet18", 611, BATCH)
    yield qnn, x
    Q.disable_integer_inference(qnn)


def drive(qnn, x, flags):
    import main_imagenet as M
    from shiftedscalequantization_amd.cli import parse_args
    args = parse_args(["--arch", "resnet18", "--int_infer_carry_head", "--int_infer_u8_images", *flags])
    M.run_integer_inference(qnn, args, x, None, bs=BATCH[0])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("flags,form", [
    (["--int_infer_u8_layout", "nhwc"], "interleaved"),
    (["--int_infer_u8_layout", "rgba"], "interleaved"),
    (["--int_infer_u8_frame", "40"], "planar"),
    (["--int_infer_u8_layout", "nhwc", "--int_infer_u8_frame", "37"], "interleaved"),
])
def test_layouts_and_frames_run_to_the_end(Q, net, capsys, monkeypatch, flags, form, graph):
    monkeypatch.setenv("SSQ_STEM_U8", "1")
    monkeypatch.setenv("SSQ_STEM_U8_STRIDED", "1")
    qnn, x = net
    drive(qnn, x, flags + (["--int_infer_graph"] if graph else []))
    out = capsys.readouterr().out
    assert f"stem conv on the int8 MFMA (K32): {STEM}: yes" in out
    assert "one uint8 batch of 2: max |logit difference|" in out
    assert "0 off-grid activations" in out
    rep = Q.stem_carry_report(qnn)
    assert rep["u8"] == {STEM: 1} and rep["un_u8"] == {STEM: {}} and rep["calls"] == {STEM: 2}
    forms = Q.integer_report(qnn)["u8_form"]
    assert forms == {STEM: {form: 1}}
    assert "uint8 stem forwards on K32 by staging form" in out and f"): {forms}" in out


def test_the_default_knob_runs_to_the_end_too(Q, net, capsys, monkeypatch):
    monkeypatch.setenv("SSQ_STEM_U8", "1")
    monkeypatch.delenv("SSQ_STEM_U8_STRIDED", raising=False)
    qnn, x = net
    drive(qnn, x, ["--int_infer_u8_layout", "nhwc"])
    out = capsys.readouterr().out
    rep = Q.stem_carry_report(qnn)
    (why, n), = rep["un_u8"][STEM].items()
    assert "channels-last" in why and n == 1 and rep["u8"] == {STEM: 0}
    assert f"by staging form (nhwc): {{'{STEM}': {{}}}}" in out
    assert "0 off-grid activations" in out


def test_a_frame_smaller_than_the_input_is_refused(Q, net):
    qnn, x = net
    with pytest.raises(SystemExit, match="smaller than the input"):
        drive(qnn, x, ["--int_infer_u8_frame", "16"])
