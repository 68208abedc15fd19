"""K23 split along K (csrc/qinfer.hip), host side: the seven new entry points are declared,
exported and bound with their parents' argument lists plus (splits, ws, ws_bytes); the workspace
size is Z * (Co + 1) * M int32 words (Z * Co * M for a centred blob) and 0 where the split is
refused; the slice partition the partial kernel walks is a partition; every refusal is SSQ_E_ARG
before any launch (no GPU needed: the checks return first); the host rule K.qconv_splits leaves
ResNet-18 layer1 at batch 64 alone and never exceeds the k steps; the flags reach the planner."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("fwd", "codes_fwd", "codes_res_fwd")
SPLIT = tuple(f"ssq_qconv_i8_{c}splitk_{f}" for c in ("", "centred_") for f in FORMS)
NEW = SPLIT + ("ssq_qconv_i8_splitk_workspace_size",)


def _header():
    src = open(os.path.join(ROOT, "include", "ssq.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _params(src, name):
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


# ---------------------------------------------------------------- ABI
def test_new_symbols_declared_exported_and_bound():
    from shiftedscalequantization_amd import _capi
    src = _header()
    lib = _capi.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(NEW) == 7
    for s in NEW:
        assert hasattr(lib, s) and s in _capi.SIGNATURES, s
        assert len(_capi.SIGNATURES[s][1]) == len(_params(src, s)), s
        assert s in doc, s


def test_split_entry_points_mirror_their_parents():
    """The parent's parameter list, then (int splits, void* ws, size_t ws_bytes), then the stream;
    the ctypes signature likewise."""
    from shiftedscalequantization_amd import _capi
    src = _header()
    for s in SPLIT:
        parent = s.replace("splitk_", "")
        mine, theirs = _params(src, s), _params(src, parent)
        assert mine[:-4] == theirs[:-1], s
        assert mine[-4:] == ["int splits", "void* ws", "size_t ws_bytes", "ssq_stream_t stream"], s
        res, args = _capi.SIGNATURES[s]
        pres, pargs = _capi.SIGNATURES[parent]
        assert res is pres and args[:-4] == pargs[:-1], s
        assert args[-4:] == [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p], s


# ---------------------------------------------------------------- workspace size
def _ws(lib, Nb=3, H=9, W=9, Co=33, R=3, S=3, stride=2, pad=1, Cp=32, splits=2, centred=0):
    return lib.ssq_qconv_i8_splitk_workspace_size(Nb, H, W, Co, R, S, stride, pad, Cp, splits,
                                                  centred)


def test_workspace_size_formula():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    # k180_tails: OH = OW = 5, M = 75, Kp = 64 * ceil(9 * 32 / 64) = 320, nk = 5
    for Z in (2, 3, 5):
        assert _ws(lib, splits=Z) == Z * (33 + 1) * 75 * 4
        assert _ws(lib, splits=Z, centred=1) == Z * 33 * 75 * 4
    # H != W, stride 1, no padding
    assert _ws(lib, Nb=2, H=6, W=10, Co=48, stride=1, pad=0, Cp=16, splits=2) == 2 * 49 * (2 * 4 * 8) * 4
    # a linear: one pixel per row
    assert _ws(lib, Nb=5, H=1, W=1, Co=10, R=1, S=1, stride=1, pad=0, Cp=80, splits=2) == 2 * 11 * 5 * 4
    # refused: 0
    assert _ws(lib, splits=1) == 0 and _ws(lib, splits=0) == 0 and _ws(lib, splits=-2) == 0
    assert _ws(lib, splits=6) == 0                      # > nk = 5
    assert _ws(lib, Cp=4096, splits=17) == 0            # > 16 whatever nk
    assert _ws(lib, Cp=4096, splits=16) == 16 * 34 * 75 * 4
    assert _ws(lib, Cp=20) == 0 and _ws(lib, Cp=0) == 0   # not a padded channel count
    assert _ws(lib, Nb=0) == 0 and _ws(lib, Co=0) == 0 and _ws(lib, R=8) == 0
    assert _ws(lib, stride=0) == 0 and _ws(lib, pad=-1) == 0 and _ws(lib, H=1, pad=0) == 0
    assert _ws(lib, Nb=1 << 20, H=64, W=64, Co=64, stride=1) == 0     # 2^31 elements


def test_wrapper_workspace_bytes_matches_the_abi():
    import torch
    from shiftedscalequantization_amd import kernels as K
    prep = K.QPrepared(torch.empty(1, dtype=torch.uint8), (33, 20, 3, 3), None)
    assert K.qconv_split_workspace_bytes(prep, 3, 9, 9, 2, 1, 3) == 3 * 34 * 75 * 4
    prep.centred = True
    assert K.qconv_split_workspace_bytes(prep, 3, 9, 9, 2, 1, 3) == 3 * 33 * 75 * 4
    assert K.qconv_split_workspace_bytes(prep, 3, 9, 9, 2, 1, 6) == 0


# ---------------------------------------------------------------- slice partition
def test_slices_partition_the_k_steps():
    """Slice z walks [floor(z nk / Z), floor((z + 1) nk / Z)): for every nk in 2..80 and Z in
    2..min(16, nk) the slices are non-empty, disjoint and cover [0, nk) in order."""
    for nk in range(2, 81):
        for Z in range(2, min(16, nk) + 1):
            edges = [z * nk // Z for z in range(Z + 1)]
            assert edges[0] == 0 and edges[-1] == nk
            assert all(a < b for a, b in zip(edges[:-1], edges[1:])), (nk, Z)
            walked = [k for z in range(Z) for k in range(edges[z], edges[z + 1])]
            assert walked == list(range(nk)), (nk, Z)


# ---------------------------------------------------------------- refusals
def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


GEO = dict(Nb=3, Ci=20, H=9, W=9, Co=33, R=3, S=3, stride=2, pad=1, groups=1)
NEED = 2 * 34 * 75 * 4


def _call(lib, name, splits=2, ws=True, ws_bytes=NEED, z=0.0, **geo):
    g = dict(GEO, **geo)
    f = _fake
    args = [f(), f(), f(), g["Nb"], g["Ci"], g["H"], g["W"], g["Co"], g["R"], g["S"], g["stride"],
            g["pad"], g["groups"], z, 0, 15]
    if name.endswith("splitk_fwd"):
        args += [f()]
    else:
        args += [None, None, None, 1, 0.1, 0.0, 0, 15, f(), f()]
        if name.endswith("res_fwd"):
            args += [f(), None, 0.0, 0.0, 0, 0]
    return getattr(lib, name)(*args, splits, f() if ws else None, ws_bytes, None)


@pytest.mark.parametrize("name", SPLIT)
def test_split_refusals_without_gpu(name):
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    err = lib.ssq_last_error
    need = NEED if "centred" not in name else 2 * 33 * 75 * 4
    for Z in (1, 0, -1, 17, 6):                         # < 2, > 16, > nk = 5
        assert _call(lib, name, splits=Z) == -1 and b"splits" in err(), Z
    assert _call(lib, name, groups=2) == -1 and b"groups" in err()
    assert _call(lib, name, ws=False) == -1 and b"workspace" in err()
    assert _call(lib, name, ws_bytes=need - 1) == -1 and b"workspace" in err()
    assert _call(lib, name, ws_bytes=0) == -1 and b"workspace" in err()
    # what the parent refuses, with a valid split
    assert _call(lib, name, Nb=0) == -1 and b"geometry" in err()
    assert _call(lib, name, R=8) == -1 and b"geometry" in err()
    assert _call(lib, name, z=0.5) == -1 and b"zero point" in err()
    assert _call(lib, name, Ci=65536) == -1 and b"65536" in err()


def test_wrappers_refuse_without_gpu():
    import torch
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    codes = torch.zeros((1, 4, 4, 16), dtype=torch.int8)
    grouped = K.QPrepared(torch.empty(1, dtype=torch.uint8), (8, 16, 3, 3), None, groups=2)
    with pytest.raises(SSQError, match="dense"):
        K._qconv_split("qconv", grouped, 2, "fwd", 2, None, codes, 1, 1)
    ws = torch.empty(4096, dtype=torch.uint8)
    plain = K.QPrepared(None, (8, 16, 3, 3), None)
    fn, held, tail = K._qconv_split("qconv_codes", plain, 1, "codes_fwd", 2, ws, codes, 1, 1)
    assert fn == "ssq_qconv_i8_splitk_codes_fwd" and held is ws and tail[0] == 2 and tail[2] == 4096
    centred = K.QPrepared(None, (8, 16, 3, 3), None, centred=True)
    fn, _, _ = K._qconv_split("qconv_codes", centred, 1, "codes_res_fwd", 2, ws, codes, 1, 1)
    assert fn == ("ssq_qconv_i8_centred_splitk_codes_res_fwd" if K.QCONV_CENTRED else
                  "ssq_qconv_i8_splitk_codes_res_fwd")
    with pytest.raises(SSQError, match="workspace"):
        K._qconv_split("qconv", plain, 1, "fwd", 2, torch.empty(4096), codes, 1, 1)
    # the geometry of the workspace query comes from the codes, by name
    seen = {}
    real = K.qconv_split_workspace_bytes
    try:
        K.qconv_split_workspace_bytes = lambda prep, **kw: seen.update(kw) or 0
        K._qconv_split("qconv", plain, 1, "fwd", 3, None, torch.zeros((5, 6, 7, 16), dtype=torch.int8),
                       (2, 2), (1, 1))
    finally:
        K.qconv_split_workspace_bytes = real
    assert seen == dict(N=5, H=6, W=7, stride=2, padding=1, splits=3)


def test_a_mistyped_knob_is_refused_by_name(monkeypatch):
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    monkeypatch.setattr(K, "QCONV_SPLITK", "atuo")
    with pytest.raises(SSQError, match="SSQ_QCONV_SPLITK"):
        K.qconv_splits(392, 512, 4608)


# ---------------------------------------------------------------- the host rule
def test_qconv_splits_rule(monkeypatch):
    from shiftedscalequantization_amd import kernels as K
    monkeypatch.setattr(K, "QCONV_SPLITK", "auto")
    # ResNet-18 layer1 at batch 64: M = 64 * 56 * 56, Co = 64: 3136 workgroups, nk = 9
    assert -(-64 * 56 * 56 // 64) * 1 == 3136
    assert K.qconv_splits(64 * 56 * 56, 64, 576) == 1
    shapes = [(M, Co, 64 * nk) for M in (1, 50, 64, 392, 3136, 12544) for Co in (16, 64, 512, 2048)
              for nk in (1, 2, 3, 5, 8, 9, 16, 23, 72, 1024)]
    for knob in ("auto", "0", "1", "2", "3", "4", "8", "16"):
        monkeypatch.setattr(K, "QCONV_SPLITK", knob)
        for M, Co, Kp in shapes:
            Z = K.qconv_splits(M, Co, Kp)
            assert Z in (1, 2, 4, 8) and Z <= Kp // 64, (knob, M, Co, Kp, Z)
            if knob in ("0", "1"):
                assert Z == 1
            if knob in ("2", "3", "4", "8", "16"):      # forced: the largest of 1, 2, 4, 8 that fits
                assert Z == max(z for z in (1, 2, 4, 8) if z <= min(int(knob), Kp // 64))
    # the rule is a pure function of its arguments and the thresholds
    monkeypatch.setattr(K, "QCONV_SPLITK", "auto")
    monkeypatch.setattr(K, "QSPLIT_WORKGROUPS", 1024)
    monkeypatch.setattr(K, "QSPLIT_STEPS", 8)
    assert K.qconv_splits(3136, 512, 4608) == 2         # 392 workgroups, nk = 72: 784 <= 1024
    assert K.qconv_splits(392, 512, 4608) == 8          # 56 workgroups: 448 <= 1024, 72 / 8 = 9
    assert K.qconv_splits(392, 512, 2048) == 4          # nk = 32: 32 / 8 = 4 < 8 steps
    assert K.qconv_splits(392, 512, 512) == 1           # nk = 8: a slice would hold 4 steps
    assert K.qconv_splits(64 * 56 * 56, 64, 576) == 1
    monkeypatch.setattr(K, "QSPLIT_WORKGROUPS", 0)
    assert K.qconv_splits(392, 512, 4608) == 1


# ---------------------------------------------------------------- flags and reports
def test_cli_flags_imply_int_infer():
    from shiftedscalequantization_amd.cli import parse_args
    a = parse_args(["--int_infer_splitk"])
    assert a.int_infer and a.int_infer_splitk and not a.int_infer_graph
    a = parse_args(["--int_infer_graph"])
    assert a.int_infer and a.int_infer_graph and not a.int_infer_splitk
    a = parse_args([])
    assert not (a.int_infer or a.int_infer_splitk or a.int_infer_graph)


def test_split_report_and_graph_without_a_plan():
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd.quant import IntegerGraph, split_report
    qnn = D.build_qnn("resnet18", 2, 4, device="cpu")
    assert split_report(qnn) == {}
    with pytest.raises(ValueError, match="no integer plan"):
        IntegerGraph(qnn)
