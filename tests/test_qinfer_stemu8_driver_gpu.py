"""main_imagenet.run_integer_inference under --int_infer_u8_images (the driver's own code path, not
only its flags): a restored random-init ResNet-18 on (2, 3, 32, 32) batches, with and without
--int_infer_fused_stem and --int_infer_graph, on the one synthetic uint8 batch and on a small
validation list.  The run prints the K32 line, the comparison with the normalised batch and the
report, and the report counts the uint8 forwards on K32."""
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
    qnn, x = restored(Q, "resnet18", 411, BATCH)
    yield qnn, x
    Q.disable_integer_inference(qnn)


def drive(qnn, x, flags, loader=None):
    import main_imagenet as M
    from shiftedscalequantization_amd.cli import parse_args
    args = parse_args(["--arch", "resnet18", "--int_infer_carry_head", "--int_infer_u8_images", *flags])
    M.run_integer_inference(qnn, args, x, loader, bs=BATCH[0])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("fused", [False, True])
def test_one_synthetic_uint8_batch(Q, net, capsys, fused, graph):
    qnn, x = net
    flags = (["--int_infer_fused_stem"] if fused else []) + (["--int_infer_graph"] if graph else [])
    drive(qnn, x, flags)
    out = capsys.readouterr().out
    assert f"stem conv on the int8 MFMA (K32): {STEM}: yes" in out
    assert ("stem conv emitting its own codes (K31)" in out) == fused
    assert "one uint8 batch of 2: max |logit difference|" in out
    assert "0 off-grid activations" in out
    rep = Q.stem_carry_report(qnn)
    # the uint8 forward took K32 (7x7/2 on 2 x 16 x 16 pixels), the normalised one the fp32 emit
    assert rep["u8"] == {STEM: 1} and rep["un_u8"] == {STEM: {}} and rep["calls"] == {STEM: 2}
    assert ("fused" in rep) == fused
    assert f"uint8 stem forwards on K32: {rep['u8']}" in out


@pytest.mark.parametrize("graph", [False, True])
def test_a_validation_list_of_float_and_uint8_batches(Q, net, capsys, graph):
    import main_imagenet as M
    qnn, x = net
    u = torch.randint(0, 256, BATCH, generator=torch.Generator().manual_seed(413), dtype=torch.uint8)
    labels = torch.tensor([1, 2])
    mean = torch.tensor(M.IMAGENET_MEAN).reshape(1, 3, 1, 1)
    std = torch.tensor(M.IMAGENET_STD).reshape(1, 3, 1, 1)
    as_float = (u.float() / 255 - mean) / std
    assert torch.equal(M.to_u8(as_float), u) and M.to_u8(u) is u     # the loader's grid, back
    drive(qnn, x, ["--int_infer_graph"] if graph else [], loader=[(u, labels), (as_float, labels)])
    out = capsys.readouterr().out
    assert "Integer inference on uint8 images (W2A4) accuracy:" in out
    assert "Integer inference on the same images normalised to fp32 (W2A4) accuracy:" in out
    rep = Q.stem_carry_report(qnn)
    assert rep["u8"] == {STEM: 2} and rep["un_u8"] == {STEM: {}} and rep["calls"] == {STEM: 4}
