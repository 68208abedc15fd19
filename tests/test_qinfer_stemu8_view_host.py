"""Strided views of the uint8 stem (K32, csrc/qinfer_stemu8.hip), host side.

`ssq_stem_u8_view_span` gives the lowest and highest byte offset a launch may read and the staging
form.  Both are checked against a numpy enumeration of every address the rule
n sN + c sC + h sH + w sW produces for the view, the views built with torch so that the strides are
the ones a caller hands over.  Then the refusals, the wrappers' form query, the shape rule and its
knob, the flags and the report's key."""
import ctypes as C

import numpy as np
import pytest
import torch

FORMS = ("planar", "interleaved", "generic")


def frame(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def hwc(u):
    """The caller's idiom for an interleaved batch (N, H, W, C)."""
    return u.permute(0, 3, 1, 2)


# name: (the (N, Ci, H, W) view, its form)
def views():
    return {
        "dense NCHW": (frame(2, 3, 5, 7), "planar"),
        "HWC-3": (hwc(frame(2, 5, 7, 3)), "interleaved"),
        "HWC-4": (hwc(frame(2, 5, 7, 4)), "interleaved"),
        "RGB in 4-byte pixels": (hwc(frame(2, 5, 7, 4)[..., :3]), "interleaved"),
        "planar crop": (frame(2, 3, 10, 14)[:, :, 2:7, 3:10], "planar"),
        # from row 1, column 3 of an HWC frame: the storage offset is (1 * 14 + 3) * 3 = 51, odd
        "HWC crop, odd offset": (hwc(frame(2, 10, 14, 3)[:, 1:6, 3:10, :]), "interleaved"),
        "u[::2]": (frame(4, 3, 5, 7)[::2], "planar"),
        "batch-expanded": (frame(1, 3, 5, 7).expand(4, 3, 5, 7), "planar"),
        "one channel, HWC": (hwc(frame(2, 5, 7, 1)), "planar"),
        "one channel of RGBA": (hwc(frame(2, 5, 7, 4)[..., 1:2]), "interleaved"),
        "W and H swapped in memory": (frame(2, 3, 7, 5).permute(0, 1, 3, 2), "generic"),
        "every other column": (frame(2, 3, 5, 14)[..., ::2], "generic"),
        "two of five interleaved bytes": (hwc(frame(2, 5, 7, 5)[..., :2]), "generic"),
    }


def span(lib, shape, strides):
    lo, hi, form = C.c_int64(-7), C.c_int64(-7), C.c_int(-7)
    rc = lib.ssq_stem_u8_view_span(*shape, *strides, C.byref(lo), C.byref(hi), C.byref(form))
    return rc, lo.value, hi.value, form.value


@pytest.mark.parametrize("name", sorted(views()))
def test_span_and_form_against_every_address(name):
    from shiftedscalequantization_amd import _capi
    from shiftedscalequantization_amd import kernels as K
    v, form = views()[name]
    shape, strides = tuple(v.shape), tuple(v.stride())
    idx = np.indices(shape).reshape(4, -1).astype(np.int64)
    addr = (idx * np.asarray(strides, np.int64).reshape(4, 1)).sum(0)
    rc, lo, hi, f = span(_capi.load(), shape, strides)
    assert rc == 0 and (lo, hi) == (int(addr.min()), int(addr.max())) and FORMS[f] == form
    # the span lies inside the storage the view was cut from
    off, size = v.storage_offset(), v.untyped_storage().nbytes()
    assert 0 <= off + lo and off + hi < size
    assert K.stem_u8_view_form(v) == form
    if name == "HWC crop, odd offset":
        assert off % 2 == 1
    # every address is one the view's own elements have: the storage positions torch reads
    flat = torch.arange(size, dtype=torch.int64)
    own = torch.as_strided(flat, shape, strides, off).reshape(-1).numpy()
    assert np.array_equal(np.sort(own), np.sort(addr + off))


def test_form_rule_edges():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    form = lambda shape, strides: FORMS[span(lib, shape, strides)[3]]
    # unit stride along W is planar whatever the others are
    assert form((2, 3, 5, 7), (0, 35, 7, 1)) == "planar"
    assert form((2, 3, 5, 7), (105, 1, 21, 1)) == "planar"
    # interleaved: unit channel stride and pixels of Ci .. 4 bytes
    assert form((2, 3, 5, 7), (105, 1, 21, 3)) == "interleaved"
    assert form((2, 3, 5, 7), (140, 1, 28, 4)) == "interleaved"
    assert form((2, 4, 5, 7), (140, 1, 28, 4)) == "interleaved"
    assert form((2, 2, 5, 7), (70, 1, 14, 2)) == "interleaved"
    # a pixel narrower than its channels, wider than 4 bytes, or channels apart: generic
    assert form((2, 3, 5, 7), (70, 1, 14, 2)) == "generic"
    assert form((2, 3, 5, 7), (175, 1, 35, 5)) == "generic"
    assert form((2, 3, 5, 7), (210, 2, 42, 6)) == "generic"
    assert form((2, 3, 5, 7), (105, 35, 7, 0)) == "generic"


def test_refusals():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    err = lib.ssq_last_error
    ok = ((2, 3, 5, 7), (105, 35, 7, 1))
    assert span(lib, *ok)[0] == 0
    for k in range(4):
        strides = list(ok[1])
        strides[k] = -strides[k]
        assert span(lib, ok[0], strides)[0] == -1 and b"negative stride" in err()
    # the channel reversal u.flip(1) as a raw view
    assert span(lib, (2, 3, 5, 7), (105, -35, 7, 1))[0] == -1
    # a span of 2^31 bytes or more: the last byte at offset 2^31 - 1 passes, one further does not
    assert span(lib, (1, 1, 1, 1 << 31), (0, 0, 0, 1))[0] == -1      # a size of 2^31
    rc, lo, hi, _ = span(lib, (1, 1, 2, (1 << 30)), (0, 0, 1 << 30, 1))
    assert (rc, lo, hi) == (0, 0, (1 << 31) - 1)
    assert span(lib, (1, 1, 3, (1 << 30)), (0, 0, 1 << 30, 1))[0] == -1 and b"2^31" in err()
    assert span(lib, (2, 3, 5, 7), (1 << 31, 35, 7, 1))[0] == -1 and b"2^31" in err()
    assert span(lib, (3, 3, 5, 7), (1 << 30, 35, 7, 1))[0] == -1 and b"2^31" in err()
    # sums that would wrap 64 bits are refused, not wrapped
    assert span(lib, ((1 << 31) - 1,) * 4, ((1 << 31) - 1,) * 4)[0] == -1 and b"2^31" in err()
    assert span(lib, (0, 3, 5, 7), ok[1])[0] == -1 and b"geometry" in err()
    assert lib.ssq_stem_u8_view_span(*ok[0], *ok[1], None, None, None) == -1 and b"null" in err()


def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


@pytest.mark.parametrize("codes", [False, True])
def test_strided_calls_refuse_before_any_launch_without_gpu(codes):
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    err = lib.ssq_last_error
    f = _fake
    nbytes = lib.ssq_stem_u8_weight_prepared_bytes(16, 3, 3, 3)

    def run(strides, u=True, geo=(1, 3, 8, 8, 16, 3, 3), pad=(1, 1)):
        head = (f() if u else None, f(), nbytes, f(), f(), *geo, 1, 1, *pad, *strides, 0)
        if codes:
            return lib.ssq_stem_conv_u8_strided_codes_fwd(*head, None, None, None, 1, 0.1, 0.0, 0,
                                                          255, f(), f(), None)
        return lib.ssq_stem_conv_u8_strided_fwd(*head, f(), None)

    assert run((192, 64, -8, 1)) == -1 and b"negative stride" in err()
    assert run((192, -1, 24, 3)) == -1 and b"negative stride" in err()
    assert run((192, 64, 1 << 30, 1)) == -1 and b"2^31" in err()
    # the existing refusals come first and read the same
    assert run((192, 64, 8, 1), u=False) == -1 and b"null" in err()
    assert run((192, 64, 8, 1), pad=(3, 1)) == -1 and b"padding" in err()
    assert run((192, 64, 8, 1), geo=(1, 5, 8, 8, 16, 3, 3)) == -1 and b"stem geometry" in err()


def test_view_form_of_the_wrapper():
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    # a view the ABI refuses is copied: here a span of 2^31 bytes, never allocated (meta device)
    big = torch.empty((1, 1, 3, 1 << 30), dtype=torch.uint8, device="meta")
    assert K.stem_u8_view_form(big) == "copied"
    assert K.stem_u8_view_form(big[:, :, :2]) == "planar"
    with pytest.raises(SSQError, match="4-D uint8"):
        K.stem_u8_view_form(torch.zeros(1, 3, 8, 8))
    with pytest.raises(SSQError, match="4-D uint8"):
        K.stem_u8_view_form(torch.zeros(3, 8, 8, dtype=torch.uint8))
    # the launch wrappers still refuse a host tensor, whatever its layout
    sw = K.StemU8Weight(torch.zeros(16, dtype=torch.uint8), (16, 3, 3, 3), None)
    with pytest.raises(SSQError, match="HIP"):
        K.stem_conv_u8(hwc(frame(1, 8, 8, 3)), sw, torch.zeros(3), torch.zeros(16, 3))


# ---------------------------------------------------------------- the shape rule and its knob
STEM7 = ((64, 3, 7, 7), (64, 3, 224, 224), (2, 2), (3, 3))
STEM3 = ((32, 3, 3, 3), (64, 3, 224, 224), (2, 2), (1, 1))


def test_shape_rule_knob(monkeypatch):
    from shiftedscalequantization_amd.quant import integer as I
    takes, route = I.stem_u8_takes, I.stem_u8_view_route
    monkeypatch.delenv("SSQ_STEM_U8", raising=False)
    monkeypatch.setenv("SSQ_STEM_U8_STRIDED", "1")
    for geo in (STEM7, STEM3):
        for form in FORMS:
            assert takes(*geo, form=form) is True and route(form, *geo) == form
        assert takes(*geo, form="copied") is False and route("copied", *geo) == "copied"
    monkeypatch.setenv("SSQ_STEM_U8_STRIDED", "0")
    for form in FORMS + ("copied",):
        assert takes(*STEM7, form=form) is False and route(form, *STEM7) == "copied"
    # the view knob does not touch the dense question, nor the other way round
    monkeypatch.setenv("SSQ_STEM_U8", "1")
    assert takes(*STEM7) is True and takes(*STEM7, form="interleaved") is False
    monkeypatch.setenv("SSQ_STEM_U8", "0")
    monkeypatch.setenv("SSQ_STEM_U8_STRIDED", "1")
    assert takes(*STEM7) is False and takes(*STEM7, form="interleaved") is True
    monkeypatch.delenv("SSQ_STEM_U8")
    # auto, set or unset: exactly the measured classes, each from its smallest measured batch up
    for env in ("auto", None):
        if env is None:
            monkeypatch.delenv("SSQ_STEM_U8_STRIDED")
        else:
            monkeypatch.setenv("SSQ_STEM_U8_STRIDED", env)
        for geo in (STEM7, STEM3):
            (_, _, R, S), (N, _, H, W), (sh, sw), _ = geo
            for form in FORMS:
                want = any((form, R, S, sh, sw) == tuple(c[:5]) and N * H * W >= c[5]
                           for c in I.U8_VIEW_CLASSES)
                assert takes(*geo, form=form) is want
                assert route(form, *geo) == (form if want else None)
            assert route("copied", *geo) is None
        # nothing unmeasured: the small planes of the suite, another kernel
        small = ((64, 3, 7, 7), (2, 3, 32, 32), (2, 2), (3, 3))
        other = ((64, 3, 5, 5), (64, 3, 224, 224), (2, 2), (2, 2))
        for form in FORMS:
            assert takes(*small, form=form) is False and route(form, *small) is None
            assert takes(*other, form=form) is False
    for c in I.U8_VIEW_CLASSES:
        assert c[0] in FORMS and len(c) == 6


def test_dense_rule_is_unchanged_by_the_form_argument(monkeypatch):
    from shiftedscalequantization_amd.quant.integer import stem_u8_takes
    monkeypatch.delenv("SSQ_STEM_U8", raising=False)
    monkeypatch.setenv("SSQ_STEM_U8_STRIDED", "1")
    assert stem_u8_takes(*STEM7) is False
    assert stem_u8_takes((64, 3, 7, 7), (64, 3, 32, 32), (2, 2), (3, 3)) is True
    assert stem_u8_takes(*STEM7, form=None) is False


# ---------------------------------------------------------------- flags, report, ABI
def test_cli_flags_need_u8_images():
    from shiftedscalequantization_amd.cli import parse_args
    a = parse_args(["--int_infer_carry_head", "--int_infer_u8_images"])
    assert a.int_infer_u8_layout == "nchw" and a.int_infer_u8_frame == 0
    a = parse_args(["--int_infer_carry_head", "--int_infer_u8_images", "--int_infer_u8_layout",
                    "rgba", "--int_infer_u8_frame", "256"])
    assert a.int_infer_u8_layout == "rgba" and a.int_infer_u8_frame == 256
    for bad in (["--int_infer_carry_head", "--int_infer_u8_layout", "nhwc"],
                ["--int_infer_carry_head", "--int_infer_u8_frame", "256"],
                ["--int_infer_carry_head", "--int_infer_u8_images", "--int_infer_u8_layout", "chw"],
                ["--int_infer_carry_head", "--int_infer_u8_images", "--int_infer_u8_frame", "-4"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_driver_views_hold_the_batch():
    import main_imagenet as D
    u = torch.randint(0, 256, (2, 3, 6, 8), dtype=torch.uint8)
    assert D.u8_view(u, "nchw") is u
    for layout, px in (("nhwc", 3), ("rgba", 4)):
        v = D.u8_view(u, layout)
        assert torch.equal(v, u) and v.stride() == (6 * 8 * px, 1, 8 * px, px)
    raw = torch.as_strided(D.u8_view(u, "rgba"), (2, 6, 8, 4), (192, 32, 4, 1))
    assert bool((raw[..., 3] == 255).all())


def test_report_key_only_under_image_u8():
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd import quant as Q
    qnn = D.build_qnn("resnet18", 2, 4, device="cpu")
    assert set(Q.integer_report(qnn)) == {"off_grid", "calls"}
    qnn._int_u8 = {}                      # what enable_integer_inference(image_u8=...) leaves
    rep = Q.integer_report(qnn)
    assert set(rep) == {"off_grid", "calls", "u8_form"} and rep["u8_form"] == {}
    assert set(Q.stem_carry_report(qnn)) == {"edges", "calls", "pooled", "u8", "un_u8"}
    Q.disable_integer_inference(qnn)
    assert set(Q.integer_report(qnn)) == {"off_grid", "calls"}


def test_integer_graph_static_input_keeps_the_dimension_order():
    from shiftedscalequantization_amd.quant.integer import IntegerGraph
    like = IntegerGraph._static_like
    u = torch.randint(0, 256, (2, 3, 6, 8), dtype=torch.uint8)
    for v, strides in ((u, (144, 48, 8, 1)),
                       (hwc(u.permute(0, 2, 3, 1).contiguous()), (144, 1, 24, 3)),
                       # a crop of an HWC frame: dense, in the same order
                       (hwc(frame(2, 10, 14, 3))[:, :, 2:8, 3:11], (144, 1, 24, 3)),
                       # 3 channels of 4-byte pixels: dense pixels of 3
                       (hwc(frame(2, 6, 8, 4)[..., :3]), (144, 1, 24, 3)),
                       (frame(2, 3, 10, 14)[:, :, 2:8, 3:11], (144, 48, 8, 1))):
        buf = like(v)
        assert buf.stride() == strides and torch.equal(buf, v)
        assert buf.untyped_storage().nbytes() == v.numel()
    x = torch.randn(2, 3, 4, 5)
    assert like(x).stride() == x.stride() and torch.equal(like(x), x)


def test_new_symbols_declared_exported_and_bound():
    import os
    import re
    from shiftedscalequantization_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ssq.h")).read(), flags=re.S)
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    lib = _capi.load()
    protos = {}
    for s in ("ssq_stem_u8_view_span", "ssq_stem_conv_u8_strided_fwd",
              "ssq_stem_conv_u8_strided_codes_fwd", "ssq_stem_conv_u8_fwd",
              "ssq_stem_conv_u8_codes_fwd"):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, src)
        assert m and hasattr(lib, s) and s in _capi.SIGNATURES and s in doc, s
        protos[s] = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert len(_capi.SIGNATURES[s][1]) == len(protos[s]), s
    # the strided calls are the dense ones plus four int64_t byte strides after pad_w
    four = ["int64_t sN", "int64_t sC", "int64_t sH", "int64_t sW"]
    for a, b in (("ssq_stem_conv_u8_fwd", "ssq_stem_conv_u8_strided_fwd"),
                 ("ssq_stem_conv_u8_codes_fwd", "ssq_stem_conv_u8_strided_codes_fwd")):
        k = protos[a].index("int64_t pad_w") + 1
        assert protos[b] == protos[a][:k] + four + protos[a][k:]
