"""Carried stem (quant/integer.py, carry_stem), host side: `stem_edges` decides from the
structure of a CPU-built model alone, the two new entry points (ssq_epilogue_codes_fwd,
ssq_maxpool_i8_fwd) are declared, exported, bound and refuse bad arguments without a GPU, and
--int_infer_carry_stem implies the flags below it."""
import ctypes as C
import os
import re

import pytest
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssq_epilogue_codes_fwd", "ssq_maxpool_i8_fwd")


def cpu_qnn(arch):
    from shiftedscalequantization_amd import drivers as D
    return D.build_qnn(arch, 2, 4, device="cpu")


def named(qnn):
    from shiftedscalequantization_amd.quant import stem_edges
    names = {m: n for n, m in qnn.named_modules()}
    return [(names[p], [names[m] for m in pools], names[s]) for p, pools, s in stem_edges(qnn)]


# ---------------------------------------------------------------- structure
@pytest.mark.parametrize("arch,edge", [
    ("resnet18", ("model.conv1", ["model.maxpool"], "model.layer1")),
    ("resnet50", ("model.conv1", ["model.maxpool"], "model.layer1")),
    ("mobilenetv2", ("model.features.0.0", [], "model.features.1")),
    ("regnetx_600m", ("model.stem.0", [], "model.s1"))])
def test_stem_edges_of_the_model_zoo(arch, edge):
    from shiftedscalequantization_amd.quant import QuantModule
    from shiftedscalequantization_amd.quant.integer import edge_readers
    qnn = cpu_qnn(arch)
    assert named(qnn) == [edge]
    mods = dict(qnn.named_modules())
    assert isinstance(mods[edge[0]], QuantModule) and not mods[edge[0]].disable_act_quant
    entry, readers, identity = edge_readers(mods[edge[2]])
    assert readers and all(isinstance(m, QuantModule) for m in readers)
    # ResNet-18's first block adds its input as the identity residual; the others project it
    # or have no residual
    assert identity == (arch == "resnet18")


def test_no_stem_edge_without_stem_chain():
    qnn = cpu_qnn("resnet18")
    assert callable(qnn.model.stem_chain) and len(qnn.model.stem_chain()) == 5
    qnn.model.stem_chain = None               # the instance no longer declares its stem
    assert named(qnn) == []


def test_no_stem_edge_when_the_pool_stays_torchs(monkeypatch):
    from shiftedscalequantization_amd import kernels as K
    monkeypatch.setattr(K, "MAXPOOL_HIP", False)
    qnn = cpu_qnn("resnet18")
    assert type(qnn.model.maxpool) is nn.MaxPool2d
    assert named(qnn) == []


def test_no_stem_edge_for_a_pool_the_code_kernel_cannot_run():
    qnn = cpu_qnn("resnet18")
    qnn.model.maxpool.ceil_mode = True
    assert qnn.model.maxpool._plan() is None and named(qnn) == []


@pytest.mark.parametrize("arch", ["resnet18", "mobilenetv2"])
def test_no_stem_edge_with_another_module_in_the_chain(arch):
    qnn = cpu_qnn(arch)
    if arch == "resnet18":
        qnn.model.relu = nn.Hardswish()       # between the stem conv and the pool
    else:
        qnn.model.features[0][2] = nn.Hardswish()     # behind the conv inside the stem
    assert named(qnn) == []
    qnn = cpu_qnn(arch)
    chain = qnn.model.stem_chain()
    qnn.model.stem_chain = lambda: chain[:-1] + [nn.Identity()]   # nothing to hand the codes to
    assert named(qnn) == []


# ---------------------------------------------------------------- ABI
def test_new_symbols_declared_exported_and_bound():
    from shiftedscalequantization_amd import _capi
    from shiftedscalequantization_amd.build import SOURCES
    src = open(os.path.join(ROOT, "include", "ssq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _capi.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, src)
        assert m and hasattr(lib, s) and s in _capi.SIGNATURES, s
        assert len(_capi.SIGNATURES[s][1]) == m.group(1).count(",") + 1, s
        assert s in doc, s
    assert "qinfer_stem.hip" in SOURCES


def _fake():
    return C.c_void_p(256)     # non-null, never dereferenced: the checks return before any launch


def _epi(lib, y=True, gamma=None, phi=None, act=1, d=0.1, z=0.0, qmin=0, qmax=15, out=True,
         bad=True, shape=(1, 16, 4, 4)):
    f = _fake
    return lib.ssq_epilogue_codes_fwd(f() if y else None, None, gamma, phi, *shape, act, d, z, qmin,
                                      qmax, f() if out else None, f() if bad else None, None)


def test_epilogue_codes_refuses_bad_arguments_without_gpu():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    err = lib.ssq_last_error
    f = _fake
    for kw in (dict(y=False), dict(out=False), dict(bad=False)):
        assert _epi(lib, **kw) == -1 and b"null" in err()
    assert _epi(lib, gamma=f()) == -1 and b"gamma and phi" in err()
    assert _epi(lib, phi=f()) == -1 and b"gamma and phi" in err()
    assert _epi(lib, act=3) == -1 and b"activation" in err()
    for z in (0.5, 256.0, -1.0, float("nan")):
        assert _epi(lib, z=z) == -1 and b"output zero point" in err()
    assert _epi(lib, qmin=0, qmax=256) == -1 and b"8-bit" in err()
    assert _epi(lib, qmin=3, qmax=3) == -1 and b"8-bit" in err()
    for d in (0.0, -1.0, float("inf"), float("nan")):
        assert _epi(lib, d=d) == -1 and b"delta" in err()
    assert _epi(lib, shape=(1, 0, 4, 4)) == -1 and b"geometry" in err()
    assert _epi(lib, shape=(0, 16, 4, 4)) == -1 and b"geometry" in err()
    assert _epi(lib, shape=(1 << 20, 64, 8, 8)) == -1 and b"2^31" in err()


def _pool(lib, codes=True, out=True, shape=(1, 16, 8, 8), k=3, stride=2, pad=1):
    f = _fake
    return lib.ssq_maxpool_i8_fwd(f() if codes else None, *shape, k, stride, pad,
                                  f() if out else None, None)


def test_maxpool_i8_refuses_bad_arguments_without_gpu():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    err = lib.ssq_last_error
    assert _pool(lib, codes=False) == -1 and b"null" in err()
    assert _pool(lib, out=False) == -1 and b"null" in err()
    assert _pool(lib, k=8, pad=0) == -1 and b"geometry" in err()
    assert _pool(lib, k=3, pad=2) == -1 and b"geometry" in err()          # 2 * pad > K
    assert _pool(lib, k=0, pad=0) == -1 and b"geometry" in err()
    assert _pool(lib, stride=0) == -1 and b"geometry" in err()
    assert _pool(lib, pad=-1) == -1 and b"geometry" in err()
    assert _pool(lib, shape=(1, 16, 0, 8)) == -1 and b"geometry" in err()
    assert _pool(lib, shape=(1, 16, 2, 8), k=5, pad=1) == -1 and b"empty output" in err()
    assert _pool(lib, shape=(1, 16, 8, 2), k=7, pad=0) == -1 and b"empty output" in err()
    assert _pool(lib, shape=(1 << 20, 64, 8, 8)) == -1 and b"2^31" in err()


def test_wrappers_refuse_without_gpu():
    import torch
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd._capi import SSQError
    y = torch.zeros(1, 4, 3, 3)
    with pytest.raises(SSQError, match="bad is required"):
        K.epilogue_codes(y, None, None, None, 1, 0.1, 0.0, 4, False, None)
    with pytest.raises(SSQError, match="gamma and phi"):
        K.epilogue_codes(y, None, torch.ones(4), None, 1, 0.1, 0.0, 4, False,
                         torch.zeros(1, dtype=torch.int32))
    with pytest.raises(SSQError):
        K.maxpool_codes(torch.zeros(1, 4, 4, 16), 3, 2, 1)                       # not int8
    with pytest.raises(SSQError):
        K.maxpool_codes(torch.zeros(1, 4, 4, 16, dtype=torch.int8), 3, 2, 1)     # a CPU tensor


# ---------------------------------------------------------------- CLI, API
def test_cli_int_infer_carry_stem_implies_the_flags_below_it():
    from shiftedscalequantization_amd.cli import parse_args
    a = parse_args(["--int_infer_carry_stem"])
    assert (a.int_infer_carry_stem and a.int_infer_carry_blocks and a.int_infer_carry
            and a.int_infer and not a.int_infer_grouped)
    a = parse_args(["--int_infer_carry_blocks"])
    assert a.int_infer_carry_blocks and not a.int_infer_carry_stem
    assert not parse_args([]).int_infer_carry_stem


def test_reports_are_empty_without_a_plan():
    from shiftedscalequantization_amd import quant as Q
    qnn = cpu_qnn("resnet18")
    assert Q.stem_carry_report(qnn) == {"edges": [], "calls": {}, "pooled": {}}
    Q.disable_integer_inference(qnn)
    assert Q.stem_carry_report(qnn) == {"edges": [], "calls": {}, "pooled": {}}
