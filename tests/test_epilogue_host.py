"""The K13 epilogue family, host side (nothing here needs a device):

1. oracle.ssq_ref's epilogue_fwd / epilogue_bwd / epilogue_loss_bwd against an independent
   derivation: torch autograd, in float64, of the eager op sequence with
   oracle.torch_eager.uaq_fake_quant.
   (a) On the cases' own inputs the fp32 oracle and the float64 derivation round differently,
       so the elementwise outputs are compared after casting to fp32 where the masks agree
       (same integer code, same clamp decision, same activation decision), at the relative
       error of the handful of fp32 roundings each element passes through.
   (b) On inputs snapped to a dyadic grid (delta a power of two, M a power of two, p = 2)
       every fp32 operation of the oracle is exact: every mask agrees, the elementwise
       outputs are equal, and the sums agree at float64 tolerance.
2. The coverage conditions of tests/epilogue_cases.py for every case.
3. Every case lands in the form its entry names (ssq_epilogue_bwd_form, ssq_epilogue_fwd_form),
   and every form the default environment can reach is named by a case.
"""
import numpy as np
import pytest
import torch

import epilogue_cases as EC
from oracle import ssq_ref as R
from oracle.torch_eager import uaq_fake_quant

F32 = np.float32
HOST_LIMIT = 70000          # elements: the autograd derivation in seconds
SMALL = [c for c in EC.BWD + EC.TAIL if c.N * c.C * c.hw <= HOST_LIMIT]


def _t(a, grad=True):
    if a is None:
        return None
    return torch.from_numpy(np.asarray(a, np.float64).copy()).requires_grad_(grad)


def autograd64(c, x, M=None):
    """The eager op sequence (quant_layer.py:250-272, quant_block.py:105-109) in float64 and
    its autograd: dict of numpy float64 arrays plus the forward's decisions."""
    ch = lambda v: v.view(1, -1, 1, 1)
    y, bias, gamma, phi, res = _t(x.y), _t(x.bias, False), _t(x.gamma), _t(x.phi), _t(x.res)
    rb, rg, rp = _t(x.rbias, False), _t(x.rgamma), _t(x.rphi)
    delta, zp = _t(x.delta), _t(x.zp)
    pre = y + ch(bias) if bias is not None else y
    t = pre * ch(gamma) + ch(phi) if gamma is not None else pre
    if res is not None:
        rv = res + ch(rb) if rb is not None else res
        rv = rv * ch(rg) + ch(rp) if rg is not None else rv
        t = t + rv
    if c.act == 1:
        t = torch.relu(t)                          # nn.ReLU: threshold_backward
    elif c.act == 2:
        t = torch.nn.functional.relu6(t)           # nn.ReLU6: hardtanh_backward
    out = uaq_fake_quant(t, delta, zp, x.n_bits) if delta is not None else t
    o = {"t": t.detach().numpy(), "out": out.detach().numpy()}
    if c.kind == "tail":
        tgt = torch.from_numpy(x.tcache[x.idx].astype(np.float64))
        loss = (out - tgt).abs().pow(c.p).sum() / (x.M if M is None else M)
        loss.backward()
        o["loss"] = float(loss.detach())
    else:
        out.backward(torch.from_numpy(x.g.astype(np.float64)))
    g = lambda v: None if v is None or v.grad is None else v.grad.numpy()
    o.update(gy=g(y), gres=g(res), ggamma=g(gamma), gphi=g(phi), gdelta=g(delta), gzp=g(zp),
             gres_gamma=g(rg), gres_phi=g(rp))
    return o


def oracle(c, x, M=None):
    if c.kind == "tail":
        return R.epilogue_loss_bwd(x.tcache[x.idx], c.p, x.M if M is None else M, x.y, x.bias,
                                   x.gamma, x.phi, x.res, c.act, x.delta, x.zp, x.n_bits, False,
                                   x.res_epi)
    return R.epilogue_bwd(x.g, x.y, x.bias, x.gamma, x.phi, x.res, c.act, x.delta, x.zp, x.n_bits,
                          False)


def decisions(c, x, t):
    """(integer code before the clamp, activation blocks) of a pre-quant activation t."""
    t = np.asarray(t)
    code = np.zeros(t.shape)
    if x.delta is not None:
        with np.errstate(all="ignore"):
            code = np.rint(t / t.dtype.type(x.delta)) + t.dtype.type(x.zp)
    return code, R._act_blocks(t, c.act)


@pytest.mark.parametrize("c", SMALL, ids=EC.case_id)
def test_oracle_matches_float64_autograd_where_masks_agree(c):
    x = EC.inputs(c)
    ref, a = oracle(c, x), autograd64(c, x)
    t32 = R.epilogue_fwd(x.y, x.bias, x.gamma, x.phi, x.res, c.act, res_epi=x.res_epi)[0]
    out32 = R.epilogue_fwd(x.y, x.bias, x.gamma, x.phi, x.res, c.act, x.delta, x.zp, x.n_bits, False,
                           x.res_epi)[1]
    c32, b32 = decisions(c, x, t32)
    c64, b64 = decisions(c, x, a["t"])
    agree = (c32 == c64) & (b32 == b64)
    if c.kind == "tail":
        # the sign of out - tgt is a decision of the loss gradient too
        tgt = x.tcache[x.idx]
        agree &= np.sign(out32 - tgt) == np.sign(a["out"] - tgt.astype(np.float64))
    # a rounding flips a decision only within an ulp of its edge: nearly every element stays
    assert agree.mean() >= 0.999 or agree.size - agree.sum() <= 2, agree.mean()
    # <= 8 fp32 roundings on an element's path, plus the cancellation of out - tgt (the
    # tail): 1e-5 relative, and an absolute floor from that cancellation's fp32 ulp
    atol = 1e-6 * float(np.abs(ref["gy"]).max()) + 1e-30
    np.testing.assert_allclose(out32[agree], a["out"].astype(F32)[agree], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ref["gy"][agree], a["gy"].astype(F32)[agree], rtol=1e-5, atol=atol)
    if x.res is not None:
        np.testing.assert_allclose(ref["gres"][agree], a["gres"].astype(F32)[agree], rtol=1e-5, atol=atol)
    if c.kind == "tail":
        np.testing.assert_allclose(ref["loss"], a["loss"], rtol=1e-5)


def snapped(c, x):
    """The case's inputs on a dyadic grid on which every fp32 operation of the epilogue, its
    quantizer (delta = 1/2) and its backward is exact: values in multiples of 2^-5 below 8,
    per-channel operands in multiples of 1/8 (gamma: 1/4)."""
    import types
    grid = lambda a, k, lim: None if a is None else \
        (np.clip(np.rint(np.asarray(a, np.float64) * k), -lim * k, lim * k) / k).astype(F32)
    s = types.SimpleNamespace(**vars(x))
    s.y, s.res, s.g = grid(x.y, 32, 8), grid(x.res, 32, 8), grid(x.g, 32, 8)
    s.tcache = grid(x.tcache, 32, 8)
    s.bias, s.phi, s.rbias, s.rphi = (grid(v, 8, 2) for v in (x.bias, x.phi, x.rbias, x.rphi))
    s.gamma, s.rgamma = grid(x.gamma, 4, 2), grid(x.rgamma, 4, 2)
    s.res_epi = None if s.rbias is None else (s.rbias, s.rgamma, s.rphi)
    if x.delta is not None:
        s.delta = F32(0.5)
    return s


@pytest.mark.parametrize("c", [c for c in SMALL if c.p == 2.0], ids=EC.case_id)
def test_oracle_sums_match_float64_autograd_on_exact_inputs(c):
    x = snapped(c, EC.inputs(c))
    M = 256                         # a power of two: (1 / M) * (2 |d|) is exact in fp32
    ref, a = oracle(c, x, M), autograd64(c, x, M)
    for k in ("gy", "gres"):
        if a[k] is not None:
            np.testing.assert_array_equal(ref[k].astype(np.float64), a[k], err_msg=k)
    if c.kind == "tail":
        np.testing.assert_array_equal(ref["out"].astype(np.float64), a["out"])
        assert abs(ref["loss"] - a["loss"]) <= 1e-12 * abs(a["loss"])
    for name, nk in EC.sums_of(c):
        got, want = np.asarray(ref[name]), np.asarray(a[name]).reshape(-1)
        # the derivation's own float64 sum: n terms in torch's order
        tol = ref[nk] * 2.0 ** -52 * np.asarray(ref[name + "_abs"]) + 1e-300
        assert np.all(np.abs(got.reshape(-1) - want) <= tol.reshape(-1)), (name, got, want)


def test_oracle_forward_is_the_eager_fp32_sequence():
    """epilogue_fwd against the eager ops in torch fp32 (IEEE, one rounding per op): bit for
    bit, -0.0 and NaN included, on the planted special values and on an affine case."""
    for c in (EC.SPECIAL, EC.BY_ID["bwd-5x65x14x14-b1a1r1t1-q4z0"], EC.BY_ID["bwd-1x17x2x2-b1a1r1t2-q4z3"]):
        x = EC.inputs(c)
        ch = lambda v: torch.from_numpy(v.copy()).view(1, -1, 1, 1)
        t = torch.from_numpy(x.y.copy())
        if x.bias is not None:
            t = t + ch(x.bias)
        if x.gamma is not None:
            t = t * ch(x.gamma) + ch(x.phi)
        if x.res is not None:
            t = t + torch.from_numpy(x.res.copy())
        t = torch.relu(t) if c.act == 1 else (torch.nn.functional.relu6(t) if c.act == 2 else t)
        out = uaq_fake_quant(t, torch.tensor(x.delta), torch.tensor(x.zp), x.n_bits)
        ref = EC.reference(c)
        nan = np.isnan(ref.out)
        assert np.array_equal(nan, np.isnan(out.numpy())) and (not c.special or nan.any())
        np.testing.assert_array_equal(ref.pre_quant.view(np.int32), t.numpy().view(np.int32))
        np.testing.assert_array_equal(ref.out[~nan].view(np.int32), out.numpy()[~nan].view(np.int32))


@pytest.mark.parametrize("c", EC.CASES, ids=EC.case_id)
def test_case_meets_its_coverage_conditions(c):
    if c.special:
        ref = EC.reference(c)
        assert np.isnan(ref.out).any() and np.signbit(ref.pre_quant[ref.pre_quant == 0]).any()
        assert (ref.pre_quant == 6).any() and np.isnan(ref.gdelta)
        return
    s = EC.check_coverage(c)
    if c.kind == "tail" or c.view:
        x = EC.inputs(c)
        assert c.N < 2 or len(set(x.idx.tolist())) < c.N      # duplicate indices
    print(EC.case_id(c), s)


# ---------------------------------------------------------------- the form queries
@pytest.fixture(scope="module")
def K():
    # a library that is missing or does not load is a failure here, not a skip: these tests
    # are the only check that the cases reach the forms they name
    from shiftedscalequantization_amd import _capi, kernels
    _capi.load()
    return kernels


@pytest.mark.parametrize("c", EC.CASES + EC.WORKER, ids=EC.case_id)
def test_case_lands_in_the_form_it_names(K, c):
    if c.kind != "fwd":
        assert EC.bwd_form_of(K, c) == c.form, c.edge
    if c.kind != "tail":
        assert EC.fwd_form_of(K, c) == c.fwd, c.edge


def test_every_default_form_is_named_by_a_case(K):
    assert {c.form for c in EC.BWD} == {c.form for c in EC.TAIL} == {EC.G16S, EC.G16V, EC.R1V, EC.R1S}
    assert {c.fwd for c in EC.BWD + EC.FWD} == {0, 1, 2}
    # the query over a sweep of planes reaches nothing else in the default environment
    seen = {K.epilogue_bwd_form(hw, al, q, r2, ls) for hw in range(1, 1100) for al in (0, 1)
            for q in (0, 1) for r2 in (0, 1) for ls in (0, 1)}
    assert seen == {EC.G16S, EC.G16V, EC.R1V, EC.R1S}
    assert {K.epilogue_fwd_form(n, hw, al, r) for hw in (4, 49, 65) for n in (hw * 3, hw * 4)
            for al in (0, 1) for r in (0, 1)} == {0, 1, 2}


def test_the_issue_s_planes_rows_and_variants_are_listed():
    hw = lambda cs, f: {c.hw for c in cs if c.form == f and not c.mis}
    assert hw(EC.BWD, EC.G16S) >= {1, 15, 17, 49, 63} and hw(EC.BWD, EC.G16V) >= {4, 64, 68, 196, 252, 256}
    assert hw(EC.BWD, EC.R1V) >= {260, 784} and hw(EC.BWD, EC.R1S) >= {65, 81, 225}
    for cs in (EC.BWD, EC.TAIL):
        assert {(c.hw, c.form) for c in cs if c.mis} == {(64, EC.G16S), (256, EC.R1S)}
    rows = {c.rows for c in EC.BWD}
    assert rows >= {1, 3, 5, 15, 17, 1024, 1025, 16500}
    assert {c.N for c in EC.BWD} >= {1, 2, 3, 5, 9} and {c.C for c in EC.BWD} >= {1, 63, 64, 65, 130}
    assert any(c.rows == 16500 and c.hw == 65 for c in EC.TAIL)
    every = EC.BWD + EC.TAIL
    assert {c.bias for c in every} == {c.affine for c in every} == {True, False}
    assert {c.res for c in EC.TAIL} == {None, "tensor", EC.LAZY_BIAS, EC.LAZY_AFFINE}
    assert {c.act for c in EC.BWD} == {0, 1, 2} and {c.q for c in EC.BWD} == {None, EC.Q4Z0, EC.Q4Z3, EC.Q8}
    assert not all(c.need_dy for c in EC.BWD) and not all(c.want_gres for c in every)
    assert {c.p for c in EC.TAIL} == {2.0, 2.4}
    assert {c.hw for c in every if c.view} == {260, 65}
    assert any(c.fwd == 1 and c.N * c.C * c.hw > 4 * 2048 * 256 for c in EC.FWD)
    assert any(c.fwd == 0 and c.N * c.C * c.hw > 2048 * 256 for c in EC.FWD)
