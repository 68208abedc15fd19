"""The K13 glue on the device: what kernels.k13 / LazyK13 / the single launch path add.

A. The plain ABI entries have no Python caller left (every wrapper launches the _rows entries,
   null maps for an operand that is the batch itself).  They stay in the ABI, so here each is
   called directly and compared bit for bit, as int32 views, with its _rows twin given null
   maps and no stage: ssq_bias_act / ssq_bias_act_fq / ssq_epilogue_fwd against
   ssq_epilogue_fwd_rows on the three forward forms (epilogue_cases.ENTRY_FWD: with and
   without residual, activation 0 / 1 / 2, with and without the 4-bit quantizer, the
   pre-quant activation kept and not); ssq_epilogue_bwd against ssq_epilogue_bwd_rows and
   ssq_epilogue_loss_bwd against ssq_epilogue_loss_bwd_rows on the four plane classes
   (ENTRY_BWD, ENTRY_TAIL): outputs, gy, gres, every gamma / phi / delta / zero-point sum and
   the loss.  The _rows side is also the oracle's, bit for bit, where the oracle is exact
   (forward outputs, gy, gres), so the pair cannot be wrong together.
B. The placeholder round trip: a LazyK13's materialize() is bitwise K.epilogue / K.bias_act on
   the same inputs for a tensor residual, a bias-only LazyRes and an affine LazyRes, and
   K.epilogue_loss_bwd takes the record a lazy call left as out._ssq_tail."""
import ctypes as C

import numpy as np
import pytest
import torch

import epilogue_cases as EC
import epilogue_worker as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def ibits(t):
    return None if t is None else W.host(t).reshape(-1).view(np.int32)


def same(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None), (what, k)
        if u is not None:
            np.testing.assert_array_equal(ibits(u), ibits(v), err_msg=f"{what} [{k}]")


class Operands:
    """A case's inputs on the device and their pointers, as the ABI takes them."""

    def __init__(self, K, c):
        x = self.x = EC.inputs(c)
        self.K, self.c = K, c
        self.y, self.res, self.bias = W.dev(x.y), W.dev(x.res), W.dev(x.bias)
        self.gamma, self.phi = W.dev(x.gamma), W.dev(x.phi)
        self.rbias, self.rgamma, self.rphi = W.dev(x.rbias), W.dev(x.rgamma), W.dev(x.rphi)
        self.quant = x.delta is not None
        self.delta = W.dev(np.array([x.delta], np.float32)) if self.quant else None
        self.zp = W.dev(np.array([x.zp], np.float32)) if self.quant else None
        self.lo, self.hi = K.qrange(x.n_bits, False) if self.quant else (0, 1)
        self.stream = K.stream_of(self.y)

    def p(self, name):
        return K_vp(self.K, getattr(self, name))

    def fresh(self, want=True, n=None):
        if not want:
            return None
        return torch.zeros_like(self.y) if n is None else torch.zeros(n, device="cuda")

    def workspace(self, slot):
        n = self.K.query("ssq_epilogue_bwd_workspace_size", self.c.N * self.c.C)
        return self.K.workspace(n, self.y.device, slot)


def K_vp(K, t):
    return K._vp(t)


@pytest.mark.parametrize("shape", sorted({c.shape for c in EC.ENTRY_FWD}))
def test_plain_forward_entries_equal_their_rows_twin(K, shape):
    cases = [c for c in EC.ENTRY_FWD if c.shape == shape]
    assert len(cases) == 24
    for c in cases:
        EC.check_coverage(c)
        assert EC.fwd_form_of(K, c) == c.fwd, EC.case_id(c)
        o, ref = Operands(K, c), EC.reference(c)
        n = o.y.numel()
        dims = (n, c.hw, c.C, c.act)
        qargs = (o.p("delta"), o.p("zp"), o.lo, o.hi)
        for keep in ((True, False) if o.quant else (True,)):
            def outs():
                return o.fresh(keep), o.fresh(o.quant)
            out0, yq0 = outs()
            K.call("ssq_epilogue_fwd_rows", o.p("y"), None, o.p("bias"), o.p("gamma"), o.p("phi"),
                   o.p("res"), None, K._vp(out0), K._vp(yq0), *dims, *qargs, None, None, 0, o.stream)
            out1, yq1 = outs()
            if c.affine:
                K.call("ssq_epilogue_fwd", o.p("y"), o.p("bias"), o.p("gamma"), o.p("phi"),
                       o.p("res"), K._vp(out1), K._vp(yq1), *dims, *qargs, o.stream)
            elif o.quant:
                K.call("ssq_bias_act_fq", o.p("y"), o.p("bias"), o.p("res"), K._vp(out1),
                       K._vp(yq1), *dims, *qargs, o.stream)
            else:
                K.call("ssq_bias_act", o.p("y"), o.p("bias"), o.p("res"), K._vp(out1), *dims,
                       o.stream)
            torch.cuda.synchronize()
            same((out1, yq1), (out0, yq0), EC.case_id(c))
            if keep:
                W.assert_bits(W.host(out0), ref.pre_quant, "pre_quant")
            if o.quant:
                W.assert_bits(W.host(yq0), ref.out, "out")


def _sums(o, c):
    """(ggamma, gphi, gdelta, gzp) destinations of a case."""
    return (o.fresh(c.affine, c.C), o.fresh(c.affine, c.C), o.fresh(o.quant, 1), o.fresh(o.quant, 1))


@pytest.mark.parametrize("c", EC.ENTRY_BWD, ids=EC.case_id)
def test_plain_backward_entry_equals_its_rows_twin(K, c):
    EC.check_coverage(c)
    assert EC.bwd_form_of(K, c) == c.form
    o, ref = Operands(K, c), EC.reference(c)
    g = W.dev(o.x.g)
    got = []
    for k, entry in enumerate(("ssq_epilogue_bwd_rows", "ssq_epilogue_bwd")):
        gy, gres = o.fresh(), o.fresh(o.res is not None)
        sums = _sums(o, c)
        maps = ((None,), (None,)) if entry.endswith("_rows") else ((), ())
        K.call(entry, K._vp(g), o.p("y"), *maps[0], o.p("bias"), o.p("gamma"), o.p("phi"),
               o.p("res"), *maps[1], c.N, c.C, c.hw, c.act, o.p("delta"), o.p("zp"), o.lo, o.hi,
               K._vp(gy), K._vp(gres), *[K._vp(t) for t in sums], *o.workspace("glue%d" % k),
               o.stream)
        torch.cuda.synchronize()
        got.append((gy, gres) + sums)
    same(got[1], got[0], EC.case_id(c))
    W.assert_bits(W.host(got[0][0]), ref.gy, "gy")
    W.assert_bits(W.host(got[0][1]), ref.gres, "gres")


@pytest.mark.parametrize("c", EC.ENTRY_TAIL, ids=EC.case_id)
def test_plain_tail_entry_equals_its_rows_twin(K, c):
    EC.check_coverage(c)
    assert EC.bwd_form_of(K, c) == c.form and c.p == 2.0
    o, ref = Operands(K, c), EC.reference(c)
    tcache, idx = W.dev(o.x.tcache), torch.from_numpy(o.x.idx.copy()).cuda()
    lazy_affine = o.rgamma is not None
    got = []
    for k, entry in enumerate(("ssq_epilogue_loss_bwd_rows", "ssq_epilogue_loss_bwd")):
        loss, gy, gres = o.fresh(n=1), o.fresh(), o.fresh(o.res is not None)
        ggm, gph, gd, gz = _sums(o, c)
        grg, grph = o.fresh(lazy_affine, c.C), o.fresh(lazy_affine, c.C)
        maps = ((None,), (None,)) if entry.endswith("_rows") else ((), ())
        K.call(entry, K._vp(tcache), K._vp(idx), int(o.x.M), float(c.p), K._vp(loss), o.p("y"),
               *maps[0], o.p("bias"), o.p("gamma"), o.p("phi"), o.p("res"), *maps[1], o.p("rbias"),
               o.p("rgamma"), o.p("rphi"), c.N, c.C, c.hw, c.act, o.p("delta"), o.p("zp"), o.lo,
               o.hi, K._vp(gy), K._vp(gres), K._vp(ggm), K._vp(gph), K._vp(grg), K._vp(grph),
               K._vp(gd), K._vp(gz), *o.workspace("glue%d" % k), o.stream)
        torch.cuda.synchronize()
        got.append((loss, gy, gres, ggm, gph, gd, gz, grg, grph))
    same(got[1], got[0], EC.case_id(c))
    W.assert_bits(W.host(got[0][1]), ref.gy, "gy")
    W.assert_bits(W.host(got[0][2]), ref.gres, "gres")
    np.testing.assert_allclose(float(W.host(got[0][0])[0]), ref.loss, rtol=EC.LOSS_RTOL_P2, atol=0)


@pytest.mark.parametrize("kind", ["tensor", EC.LAZY_BIAS, EC.LAZY_AFFINE])
@pytest.mark.parametrize("shape", [(3, 5, 7, 7), (3, 5, 8, 8)])
def test_placeholder_round_trip(K, shape, kind):
    """A LazyK13 materialised is the eager wrapper on the same inputs, bit for bit: the
    residual's own record (the LazyRes kinds), the record the tail's lazy call leaves, and that
    record through K.epilogue_loss_bwd."""
    gen = torch.Generator().manual_seed(shape[2] * 3 + len(kind))
    N, Cc = shape[:2]
    rnd = (lambda *s: torch.randn(*s, generator=gen).cuda())
    y, raw, bias, rbias = rnd(*shape), rnd(*shape), rnd(Cc), rnd(Cc)
    gamma, phi = 1 + 0.1 * rnd(1, Cc, 1, 1), 0.1 * rnd(1, Cc, 1, 1)
    rgamma, rphi = 1 + 0.1 * rnd(1, Cc, 1, 1), 0.1 * rnd(1, Cc, 1, 1)
    if kind == "tensor":
        res, res_eager = raw, raw
    elif kind == EC.LAZY_BIAS:
        res = K.LazyRes(raw, rbias, None, None)
        assert isinstance(res, K.LazyK13) and (res.res, res.relu, res.q) == (None, 0, None)
        res_eager = K.bias_act(raw, rbias, None, 0)
        same([res.materialize()], [res_eager], "bias-only residual")
    else:
        res = K.LazyRes(raw, rbias, rgamma, rphi)
        res_eager = K.epilogue(raw, rbias, rgamma, rphi, None, 0, None)
        same([res.materialize()], [res_eager], "affine residual")
    same([K.materialize(res)], [res_eager], "K.materialize")
    for affine in (True, False):
        gm, ph = (gamma, phi) if affine else (None, None)
        lazy = (K.epilogue(y, bias, gm, ph, res, 1, None, lazy=True) if affine
                else K.bias_act(y, bias, res, 1, lazy=True))
        tail = lazy._ssq_tail
        assert isinstance(tail, K.LazyK13) and tail.y is y and tail.res is res
        assert (tail.bias, tail.gamma, tail.phi, tail.relu, tail.q) == (bias, gm, ph, 1, None)
        eager = K.epilogue(y, bias, gm, ph, res_eager, 1, None) if affine \
            else K.bias_act(y, bias, res_eager, 1)
        same([tail.materialize()], [eager], "tail")
        live = tail.grad_inputs()
        assert any(t is y for t in live) and any(t is raw for t in live)
        assert (kind == EC.LAZY_AFFINE) == any(t is rgamma for t in live)
        cache = torch.randn(N + 2, *shape[1:], generator=gen).relu().cuda()
        idx = torch.arange(N, dtype=torch.int64).cuda()
        M = N * shape[2] * shape[3]
        r = K.epilogue_loss_bwd(tail, K.Rows(cache, idx), M)
        # (the three passes in the epilogue's form, the one the fused tail is bit-identical to)
        yr = y.clone().requires_grad_(True)
        sep = K.epilogue(yr, bias, gm, ph, res_eager, 1, None)
        loss1, g1 = K.lp_loss_and_grad(sep, K.Rows(cache, idx), 2.0)
        sep.backward(g1)
        np.testing.assert_allclose(W.host(r[0]), W.host(loss1), rtol=EC.LOSS_RTOL_P2, atol=0)
        same([r[1]], [yr.grad], "gy")
        assert r[2] is None             # (no residual input asks for a gradient here)
