"""BRECQ's Fisher-weighted losses, host side: the reference fixtures
(tests/golden/make_fisher_golden.py) against a restatement of both formulas, the --opt_mode
flag, and the K20 entry points of the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("recon_brecq_fisher_diag", "recon_brecq_fisher_full", "recon_layer_fisher_diag")
FISHER_ABI = ("ssq_fisher_loss_workspace_size", "ssq_fisher_diag_loss", "ssq_fisher_diag_loss_rows",
              "ssq_fisher_full_loss", "ssq_fisher_full_loss_rows")


def mode_of(name):
    return "fisher_full" if name.endswith("full") else "fisher_diag"


def diag_grad32(pred, tgt, fis):
    """d/d pred of sum (pred-tgt)^2 fis^2 / M as autograd evaluates it, every product rounded
    to fp32: ((1/M) * (fis*fis)) * (2*d)."""
    pred, tgt, fis = (np.asarray(a, np.float32) for a in (pred, tgt, fis))
    M = np.float32(pred.size // pred.shape[1])
    inv_m = np.float32(1.0) / M
    d = pred - tgt
    return (inv_m * (fis * fis)) * (np.float32(2.0) * d)


def loss64(pred, tgt, fis, mode):
    pred, tgt, fis = (np.asarray(a, np.float64) for a in (pred, tgt, fis))
    if mode == "fisher_diag":
        return ((pred - tgt) ** 2 * fis ** 2).sum() / (pred.size // pred.shape[1])
    a = np.abs(pred - tgt) * np.abs(fis)
    s = a.sum(axis=(1, 2, 3))
    return (s.reshape(-1, 1, 1, 1) * a).sum() / (100.0 * pred.size)


def full_grad64(pred, tgt, fis, s, n_total):
    """d/d pred of sum_n s_n * sum(a |fis|) / (100 n): 2 s_n |fis| sgn(d) / (100 n)."""
    pred, tgt, fis = (np.asarray(a, np.float64) for a in (pred, tgt, fis))
    s = np.asarray(s, np.float64).reshape((-1,) + (1,) * (pred.ndim - 1))
    return 2.0 * s * np.abs(fis) * np.sign(pred - tgt) / (100.0 * n_total)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_loads(golden, name):
    g = golden(name)
    iters = int(g["iters"][0])
    assert iters == 10 and len(g["w_total_loss"]) == iters and len(g["rec_loss"]) == iters
    assert g["w_perms"].shape == (iters, 16)
    cg = g["cached_grads"]
    assert cg.shape[0] == 16 and cg.dtype == np.float32
    assert cg.min() >= 1.0                      # |g| + 1 (data_utils.py:65)
    assert len(g["it_loss32"]) == 3 and len(g["it_loss64"]) == 3
    # warm-up (count < 0.2 * iters): no round term, the total is the reconstruction loss
    assert g["w_total_loss"][0] == g["rec_loss"][0]
    assert np.all(g["w_total_loss"][2:] > g["rec_loss"][2:])
    for k in range(3):
        shape = tuple(g[f"it{k}_shape"])
        assert shape[1:] == cg.shape[1:] and shape[0] == 8
        keep = g[f"it{k}_keep"]
        for t in ("pred", "tgt", "grad", "g32"):
            assert g[f"it{k}_{t}"].shape == (len(keep),) + shape[1:]
        # the operands are the cached rows of the iteration's batch
        np.testing.assert_array_equal(g[f"it{k}_grad"], cg[g["w_perms"][k][:8][keep]])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 600 * 1024


@pytest.mark.parametrize("name", FIXTURES)
def test_formulas_reproduce_reference(golden, name):
    """The stored fp32 losses and gradients are the two formulas' values: fisher_diag's
    gradient bit for bit in the stated operation order; the losses against the float64
    restatement (exactly the stored float64 values) and the fp32 ones within fp32
    summation error of it: torch's CPU reduction order depends on the host's vector width,
    so the fp32 sum of 16384 positive terms is bounded by its rounding, (log2(16384) + 3
    roundings per term) * 2^-24 < 2e-6 relative, instead of being replayed."""
    g = golden(name)
    mode = mode_of(name)
    for k in range(3):
        shape = tuple(g[f"it{k}_shape"])
        n_total = int(np.prod(shape))
        pred, tgt, fis = g[f"it{k}_pred"], g[f"it{k}_tgt"], g[f"it{k}_grad"]
        keep = g[f"it{k}_keep"]
        whole = len(keep) == shape[0]
        if whole:
            l64 = loss64(pred, tgt, fis, mode)
            np.testing.assert_allclose(l64, g["it_loss64"][k], rtol=1e-12)
            np.testing.assert_allclose(g["it_loss32"][k], l64, rtol=2e-6)
        np.testing.assert_allclose(g["rec_loss"][k], g["it_loss32"][k], rtol=0, atol=0)
        if mode == "fisher_diag":
            # M of the whole batch: the kept samples' gradients do not depend on the others
            full = np.zeros(shape, np.float32)
            fp, ft, ff = full.copy(), full.copy(), full.copy()
            fp[keep], ft[keep], ff[keep] = pred, tgt, fis
            np.testing.assert_array_equal(diag_grad32(fp, ft, ff)[keep].view(np.int32),
                                          g[f"it{k}_g32"].view(np.int32))
            g64 = (2.0 * (pred.astype(np.float64) - tgt) * fis.astype(np.float64) ** 2
                   / (n_total // shape[1]))
        else:
            g64 = full_grad64(pred, tgt, fis, g[f"it{k}_s64"][keep], n_total)
            if whole:
                a = np.abs(pred.astype(np.float64) - tgt) * np.abs(fis)
                np.testing.assert_allclose(a.sum(axis=(1, 2, 3)), g[f"it{k}_s64"], rtol=1e-12)
        if f"it{k}_g64_at" in g:
            g64 = g64.reshape(-1)[g[f"it{k}_g64_at"]]
        np.testing.assert_allclose(g64, g[f"it{k}_g64"], rtol=1e-12, atol=0)
        # the fp32 gradient is the float64 one up to a few fp32 roundings
        g32 = g[f"it{k}_g32"].astype(np.float64)
        ref = g[f"it{k}_g64"]
        if f"it{k}_g64_at" in g:
            g32 = g32.reshape(-1)[g[f"it{k}_g64_at"]]
        scale = np.abs(ref).max()
        assert np.abs(g32 - ref).max() <= 1e-5 * scale


def test_diag_formula_matches_torch_autograd():
    """The stated order is autograd's, bit for bit, at a 4-D, an odd and a 2-D shape."""
    gen = torch.Generator().manual_seed(5)
    for shape in ((8, 16, 5, 5), (4, 7, 3, 3), (8, 10)):
        pred = torch.randn(shape, generator=gen, requires_grad=True)
        tgt = torch.randn(shape, generator=gen)
        fis = torch.randn(shape, generator=gen).abs() + 1.0
        ((pred - tgt).pow(2) * fis.pow(2)).sum(1).mean().backward()
        ours = diag_grad32(pred.detach().numpy(), tgt.numpy(), fis.numpy())
        np.testing.assert_array_equal(ours.view(np.int32), pred.grad.numpy().view(np.int32))


def test_opt_mode_flag_reaches_recon_kwargs():
    from shiftedscalequantization_amd.cli import parse_args, recon_kwargs
    a = parse_args([])
    assert a.opt_mode == "mse"
    assert recon_kwargs(a, False)["opt_mode"] == "mse" and recon_kwargs(a, True)["opt_mode"] == "mse"
    for mode in ("fisher_diag", "fisher_full"):
        a = parse_args(["--opt_mode", mode])
        assert a.opt_mode == mode
        kw, ka = recon_kwargs(a, False), recon_kwargs(a, True)
        assert kw["opt_mode"] == mode and kw["act_quant"] is False and kw["iters"] == a.iters_w
        assert ka["opt_mode"] == mode and ka["act_quant"] is True and ka["p"] == a.p
    with pytest.raises(SystemExit):
        parse_args(["--opt_mode", "fisher"])


def test_recon_model_passes_opt_mode(monkeypatch):
    """drivers.recon_model hands the flag's keyword to every block / layer call."""
    import torch.nn as nn
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd.cli import parse_args, recon_kwargs
    seen = []
    monkeypatch.setattr(D, "layer_reconstruction", lambda qnn, m, **kw: seen.append(kw["opt_mode"]))
    monkeypatch.setattr(D, "block_reconstruction", lambda qnn, m, **kw: seen.append(kw["opt_mode"]))
    model = nn.Sequential(D.QuantModule(nn.Linear(4, 4), {"n_bits": 8}, {"n_bits": 8}))
    D.recon_model(model, model, cali_data=None,
                  **recon_kwargs(parse_args(["--opt_mode", "fisher_diag"]), False))
    assert seen == ["fisher_diag"]


def test_brecq_bench_has_the_flag():
    src = open(os.path.join(ROOT, "tools", "brecq_bench.py")).read()
    assert '"--opt_mode"' in src and "fisher_full" in src


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "ssq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ssq_[a-z0-9_]+)\s*\(", src)))


def test_fisher_entry_points_declared_exported_and_bound():
    """ssq.h's prototypes, libssq.so's exports and the ctypes signatures agree, the Fisher
    entry points among them."""
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    syms = declared_symbols()
    for s in FISHER_ABI:
        assert s in syms and hasattr(lib, s) and s in _capi.SIGNATURES
    assert not [s for s in syms if not hasattr(lib, s)]
    assert set(syms) == set(_capi.SIGNATURES)
    # one prototype argument per ctypes argument
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssq.h")).read(), flags=re.S)
    for s in FISHER_ABI:
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(proto.split(",")) == len(_capi.SIGNATURES[s][1]), s
    assert lib.ssq_fisher_loss_workspace_size(8 * 16 * 5 * 5, 8) >= 1024 * 8 + 8 * 8


def test_fisher_argument_errors_without_gpu():
    """Argument validation happens on the host before any launch: fisher_full on anything
    but a 4-D prediction, as the reference's torch.sum(..., (1, 2, 3)) raises."""
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    rc = lib.ssq_fisher_full_loss(None, None, None, 80, 8, 2, None, None, None, 0, None, 0, None)
    assert rc != 0 and b"4-D" in lib.ssq_last_error()
    rc = lib.ssq_fisher_diag_loss(None, None, None, 80, 8, None, None, None, 0, None, 0, None)
    assert rc != 0 and b"bad args" in lib.ssq_last_error()
