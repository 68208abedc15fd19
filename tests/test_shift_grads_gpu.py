"""The shift-selection kernels (K5-K9: adaShift, learned_hard_sigmoid, shift init, AdaRound
and their prepared / multi-weight forms) against the fp64 oracle at the shapes where their
tilings change (tests/shift_cases.py).  The reference is always oracle.ssq_ref, never
another kernel; kernel-against-kernel assertions here are bit-identity only.

The alpha-gradient bound.  Per alpha row (conv: input channel; Linear: element)

    |got - ref| <= 16 * 2^-23 * G,   G = ZMG * max_i |g_p[row, i]|,

g_p being the oracle's float64 sum of g_int * F_i (plus the regulariser's d/dp when it is
fused).  Both sides accumulate g_p in double from identical fp32 products, so that term
contributes nothing at this scale.  What differs is the fp32 softmax: a device expf and a
division, about 4 ulp on each s_i.  In s_i * (g_i - sum_j g_j s_j) the factor has
|g_i - dot| <= 2 G, so 4 ulp of s_i move the result by 8 * 2^-24 * G, the same error inside
dot by as much again, and the final rounding to fp32 adds one more ulp of a value <= 2 G:
about 21 * 2^-24 * G, rounded up to 16 * 2^-23 * G.  The oracle's own fp32-vs-fp64 softmax
distance is under 1 * 2^-23 * G (tests/test_shift_grads_host.py).  Rows that a one-ulp
difference can move by a whole element (shift_cases: boundary-fragile) are left out, within
caps the oracle meets on its own.

With the regulariser fused, its d/dp term of g_p is NOT identical on both sides: the kernels
evaluate it in fp32 from their own p (as the reference's tensor ops do), the oracle in
float64.  shift_cases.reg_slack derives what that adds to the bound (the term's second
derivative times the 8 ulp p may be off by, plus 8 ulp of the term); it is negligible where
the data term dominates g_p (conv weights) and decides the bound where it does not (Linear
weights at b = 20, where one element's g_int * F_i is smaller than the regulariser's slope).

Each test reports its worst error / bound and what it left out through $SSQ_PARITY_LOG
(profiles/shift_grads_parity.jsonl)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import ssq_ref as R
import shift_cases as C

pytestmark = pytest.mark.gpu

REG_LAMBDA = 0.1          # shift regulariser
ROUND_LAMBDA = 0.01       # rounding regulariser
REG_B = (20.0, 7.5, 2.0)
CASE_S = [pytest.param(shape, bits, S, id=f"{C.id_of(shape, bits)}-S{S}")
          for shape, bits in C.CASES for S in C.shift_counts(bits)]
PREP_S = [pytest.param(shape, bits, S, id=f"{C.id_of(shape, bits)}-S{S}")
          for shape, bits in C.PREP_CASES for S in C.shift_counts(bits, upto=4)]
FIVE_S = [pytest.param(shape, S, id=f"{C.id_of(shape)}-S{S}")
          for shape in C.FIVE_SHAPES for S in C.LHS_COUNTS]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def dev(a):
    return torch.as_tensor(np.array(a, np.float32)).cuda()


def host(t):
    return t.detach().float().cpu().numpy()


def close(a, b, rtol=1e-5, atol=1e-6):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def parity_report(rec):
    """Print the reached parity and append it to $SSQ_PARITY_LOG (jsonl) when set."""
    print(json.dumps(rec))
    path = os.environ.get("SSQ_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def tol_ratio(got, ref, rtol, atol, out=None, mag=None):
    """Worst |got - ref| / (atol + rtol * mag) over the elements kept; mag = |ref| unless
    given."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ratio = np.abs(got - ref) / (atol + rtol * (np.abs(ref) if mag is None else mag))
    if out is not None:
        ratio = np.where(out, 0.0, ratio)
    return float(ratio.max(initial=0.0))


def on_device(c):
    return dev(c.w), dev(c.delta), dev(c.zp), dev(c.alpha), dev(c.beta), dev(c.gy)


def check_alpha(got, ref, g_p, rows_out, what, slack=None):
    ratio = C.alpha_ratio(host(got), ref, g_p, rows_out, slack)
    print(what, "alpha worst err / bound", ratio)
    assert ratio <= 1.0, (what, ratio)
    return ratio


def check_forward(K_out, ref, ht, hr, what):
    if ht and hr:
        np.testing.assert_array_equal(host(K_out), ref, err_msg=what)
    else:
        close(host(K_out), ref, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------ a. K.adashift
@pytest.mark.parametrize("shape,bits,S", CASE_S)
def test_adashift_vs_oracle(K, shape, bits, S):
    """The recomputing adaShift backward (alpha_col_stage1 / stage2; alpha_grad_fc for
    Linear) and forward, soft and hard rounding: galpha within the alpha bound, gbeta to
    1e-4 (+1e-7), What bit-exact at hard targets + hard rounding and to 1e-7 otherwise."""
    c = C.make_case(shape, S, bits)
    w, d, z, alpha, beta, gy = on_device(c)
    worst, worst_b, n_out, n_str = 0.0, 0.0, 0, 0
    for hr in (0, 1):
        r = C.adashift_ref(shape, S, bits, hr)
        n_str = max(n_str, r.n_structural)
        a = alpha.clone().requires_grad_(True)
        b = beta.clone().requires_grad_(True)
        y = K.adashift(a, b, w, d, z, c.shifts, bits, False, 0, hr)
        check_forward(y, R.adashift_fwd(c.xq, c.alpha, c.beta, c.delta, c.zp, bits, False, c.is_fc,
                                        False, bool(hr)), 0, hr, f"t0r{hr}")
        y.backward(gy)
        worst = max(worst, check_alpha(a.grad, r.galpha, r.g_p, r.rows_out, f"hr{hr}"))
        n_out = max(n_out, int(r.rows_out.sum()))
        if hr:
            assert b.grad is None
        else:
            ratio = tol_ratio(host(b.grad), r.gbeta, 1e-4, 1e-7, r.beta_out)
            assert ratio <= 1.0, ("gbeta", ratio)
            worst_b = max(worst_b, ratio)
        y = K.adashift(alpha, beta, w, d, z, c.shifts, bits, False, 1, hr)
        check_forward(y, R.adashift_fwd(c.xq, c.alpha, c.beta, c.delta, c.zp, bits, False, c.is_fc,
                                        True, bool(hr)), 1, hr, f"t1r{hr}")
    parity_report({"test": "adashift_vs_oracle", "case": C.id_of(shape, bits), "S": S,
                   "worst_over_bound": worst, "gbeta_over_tol": worst_b, "excluded_rows": n_out,
                   "of_them_structural": n_str, "rows": int(np.prod(c.alpha.shape[:-1]))})


# ------------------------------------------------------------------ b. fused regulariser
@pytest.mark.parametrize("shape,bits,S", CASE_S)
def test_adashift_fused_reg_vs_oracle(K, shape, bits, S):
    """The shift regulariser folded into the backward (stage 2's reg_term lanes;
    alpha_chain for Linear), (lambda, b) as host floats and through the device pair:
    galpha against R.adashift_bwd + R.reg_shift's gradient within the alpha bound (g_p
    including the regulariser's d/dp), sum(reg_vals) against its value to 1e-5."""
    c = C.make_case(shape, S, bits)
    w, d, z, alpha, beta, gy = on_device(c)
    n_rows = int(np.prod(c.alpha.shape[:-1]))
    worst, n_out, n_str = 0.0, 0, 0
    for hr in (0, 1):
        r = C.adashift_ref(shape, S, bits, hr)
        n_out, n_str = max(n_out, int(r.rows_out.sum())), max(n_str, r.n_structural)
        for b_ in REG_B:
            loss, g_reg = R.reg_shift(c.alpha, b_, REG_LAMBDA)
            g_p = r.g_p + C.reg_gp(c.alpha, REG_LAMBDA, b_)
            for form in ("host", "dev"):
                vals = torch.zeros(n_rows, device="cuda")
                reg = (REG_LAMBDA, b_, vals, None) if form == "host" else \
                    (0.0, 0.0, vals, dev([REG_LAMBDA, b_]))
                a = alpha.clone().requires_grad_(True)
                K.adashift(a, beta, w, d, z, c.shifts, bits, False, 0, hr, reg=reg).backward(gy)
                worst = max(worst, check_alpha(a.grad, r.galpha + g_reg, g_p, r.rows_out,
                                               f"hr{hr} b{b_} {form}",
                                               C.reg_slack(c.alpha, REG_LAMBDA, b_)))
                close(host(vals).astype(np.float64).sum(), loss, rtol=1e-5, atol=0.0)
    parity_report({"test": "adashift_fused_reg_vs_oracle", "case": C.id_of(shape, bits), "S": S,
                   "worst_over_bound": worst, "excluded_rows": n_out, "of_them_structural": n_str,
                   "rows": n_rows})


# ------------------------------------------------------------------ c. prepared path
def _prepared_once(K, c, tensors, hr, reg_b, want_repeat):
    """Forward (soft / hard targets) and backward of one prepared weight.  Returns
    (What soft, What hard, galpha, reg_vals) as host arrays."""
    w, d, z, alpha, beta, gy = tensors
    prep = K.AdaShiftPrep(w, beta, d, c.shifts, hr)
    assert prep.ok
    hard = K.adashift_prepared(alpha, prep, d, z, c.bits, False, 1)
    grads = []
    for _ in range(3 if want_repeat else 1):
        a = alpha.clone().requires_grad_(True)
        vals = torch.zeros(alpha.shape[0], device="cuda")
        reg = None if reg_b is None else (0.0, 0.0, vals, dev([REG_LAMBDA, reg_b]))
        soft = K.adashift_prepared(a, prep, d, z, c.bits, False, 0, reg=reg)
        soft.backward(gy)
        grads.append(host(a.grad))
    for g in grads[1:]:
        np.testing.assert_array_equal(grads[0], g)
    return host(soft), host(hard), grads[0], host(vals), prep


@pytest.mark.parametrize("shape,bits,S", PREP_S)
def test_adashift_prepared_vs_oracle(K, shape, bits, S):
    """K.adashift_prepared (per-channel form in one and two batches, column form with its
    own stage 2) against the same oracle under the same bound, without and with the fused
    regulariser; repeated launches bit-identical."""
    c = C.make_case(shape, S, bits)
    tensors = on_device(c)
    worst, n_out, n_str = 0.0, 0, 0
    for hr in (0, 1):
        r = C.adashift_ref(shape, S, bits, hr)
        n_out, n_str = max(n_out, int(r.rows_out.sum())), max(n_str, r.n_structural)
        for reg_b in (None, 7.5):
            soft, hard, ga, vals, _ = _prepared_once(K, c, tensors, hr, reg_b, True)
            ref, g_p, slack = r.galpha, r.g_p, None
            if reg_b is not None:
                loss, g_reg = R.reg_shift(c.alpha, reg_b, REG_LAMBDA)
                ref, g_p = ref + g_reg, g_p + C.reg_gp(c.alpha, REG_LAMBDA, reg_b)
                slack = C.reg_slack(c.alpha, REG_LAMBDA, reg_b)
                close(vals.astype(np.float64).sum(), loss, rtol=1e-5, atol=0.0)
            ratio = C.alpha_ratio(ga, ref, g_p, r.rows_out, slack)
            assert ratio <= 1.0, (f"hr{hr} reg{reg_b}", ratio)
            worst = max(worst, ratio)
        for ht, got in ((0, soft), (1, hard)):
            fwd = R.adashift_fwd(c.xq, c.alpha, c.beta, c.delta, c.zp, bits, False, False, bool(ht), bool(hr))
            if ht and hr:
                np.testing.assert_array_equal(got, fwd)
            else:
                close(got, fwd, rtol=1e-5, atol=1e-7)
    parity_report({"test": "adashift_prepared_vs_oracle", "case": C.id_of(shape, bits), "S": S,
                   "worst_over_bound": worst, "excluded_rows": n_out, "of_them_structural": n_str,
                   "rows": int(c.alpha.shape[0])})


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_adashift_prepared_multi_vs_oracle(K, S):
    """Every prepared case of this S in ONE K.adashift_prepared_multi call (more than 8
    segments: a second launch): each weight within the alpha bound of the oracle, its What
    and gradient bit-identical to the single-weight launch, repeated launches bit-identical."""
    cases = [(shape, bits) for shape, bits in C.PREP_CASES if S in C.shift_counts(bits, upto=4)]
    assert len(cases) > 8
    worst, n_out, n_str, n_rows = 0.0, 0, 0, 0
    for hr in (0, 1):
        cs = [C.make_case(shape, S, bits) for shape, bits in cases]
        tensors = [on_device(c) for c in cs]
        singles = [_prepared_once(K, c, t, hr, 7.5, False) for c, t in zip(cs, tensors)]
        entries = [(s[4], t[1], t[2], c.bits, False) for s, t, c in zip(singles, tensors, cs)]
        regp = dev([REG_LAMBDA, 7.5])
        runs = []
        for _ in range(2):
            am = [t[3].clone().requires_grad_(True) for t in tensors]
            vals = [torch.zeros(t[3].shape[0], device="cuda") for t in tensors]
            ys = K.adashift_prepared_multi(am, entries, False, reg=(0.0, 0.0, vals, regp))
            torch.autograd.backward(list(ys), [t[5] for t in tensors])
            runs.append(([host(y) for y in ys], [host(a.grad) for a in am], [host(v) for v in vals]))
        hards = K.adashift_prepared_multi([t[3] for t in tensors], entries, True)
        for k, ((shape, bits), c, single) in enumerate(zip(cases, cs, singles)):
            what = f"{C.id_of(shape, bits)} hr{hr}"
            r = C.adashift_ref(shape, S, bits, hr)
            y, ga, v = runs[0][0][k], runs[0][1][k], runs[0][2][k]
            np.testing.assert_array_equal(y, single[0], err_msg=what)
            np.testing.assert_array_equal(host(hards[k]), single[1], err_msg=what)
            np.testing.assert_array_equal(ga, single[2], err_msg=what)
            np.testing.assert_array_equal(v, single[3], err_msg=what)
            np.testing.assert_array_equal(ga, runs[1][1][k], err_msg=what)
            np.testing.assert_array_equal(y, runs[1][0][k], err_msg=what)
            loss, g_reg = R.reg_shift(c.alpha, 7.5, REG_LAMBDA)
            ratio = C.alpha_ratio(ga, r.galpha + g_reg, r.g_p + C.reg_gp(c.alpha, REG_LAMBDA, 7.5),
                                  r.rows_out, C.reg_slack(c.alpha, REG_LAMBDA, 7.5))
            assert ratio <= 1.0, (what, ratio)
            worst = max(worst, ratio)
            close(v.astype(np.float64).sum(), loss, rtol=1e-5, atol=0.0)
            n_out, n_str = n_out + int(r.rows_out.sum()), n_str + r.n_structural
            n_rows += int(c.alpha.shape[0])
    parity_report({"test": "adashift_prepared_multi_vs_oracle", "S": S, "segments": len(cases),
                   "worst_over_bound": worst, "excluded_rows": n_out, "of_them_structural": n_str,
                   "rows": n_rows})


def test_adashift_prepared_refuses_wide_window(K):
    """A 17x17 kernel window (K = 289 > 256 taps): the preparation reports itself unusable
    and ChannelQuant keeps the recomputing kernels, whose What is the oracle's."""
    from shiftedscalequantization_amd import quant as Q
    shape, S, bits = (10, 3, 17, 17), 3, 2
    c = C.make_case(shape, S, bits)
    w, d, z, alpha, beta, gy = on_device(c)
    for hr in (0, 1):
        assert not K.AdaShiftPrep(w, beta, d, c.shifts, hr).ok
    uaq = Q.UniformAffineQuantizer(n_bits=bits, channel_wise=True, ch=shape).cuda()
    uaq.delta = torch.nn.Parameter(d.clone())
    uaq.zero_point = torch.nn.Parameter(z.clone())
    uaq.inited = True
    cq = Q.ChannelQuant(1.0, uaq=uaq, weight_tensor=w, shiftTarget=c.shifts)
    cq.init_v_beta(w)
    cq.opt_mode = "adaShift"
    cq.beta.requires_grad_(False)
    y = cq(w)
    assert cq._prep is not None and cq._prep[1] is None
    ref = K.adashift(cq.alpha, cq.beta, w, cq.delta, cq.zero_point, c.shifts, bits, False, 0, 0)
    np.testing.assert_array_equal(host(y), host(ref))
    fwd = R.adashift_fwd(c.xq, host(cq.alpha), host(cq.beta), c.delta, c.zp, bits, False, False,
                         False, False)
    close(host(y), fwd, rtol=1e-5, atol=1e-7)
    parity_report({"test": "adashift_prepared_refuses_wide_window", "case": C.id_of(shape, bits), "S": S,
                   "what_over_tol": tol_ratio(host(y), fwd, 1e-5, 1e-7), "excluded_rows": 0})


# ------------------------------------------------------------------ d. K.lhs
@pytest.mark.parametrize("shape,S", FIVE_S)
def test_lhs_vs_oracle(K, shape, S):
    """learned_hard_sigmoid with the candidates of R.init_v: soft forward to 1e-7, hard
    forward bit-exact, galpha against R.lhs_bwd within the alpha bound."""
    r = C.lhs_ref(shape, S, 2)
    c = r.case
    w, d, z, alpha, beta, gy = on_device(c)
    a = alpha.clone().requires_grad_(True)
    y = K.lhs(a, w, d, z, c.shifts, 2, False, False)
    close(host(y), r.soft, atol=1e-7)
    y.backward(gy)
    worst = check_alpha(a.grad, r.galpha, r.g_p, r.rows_out, "lhs")
    np.testing.assert_array_equal(host(K.lhs(alpha, w, d, z, c.shifts, 2, False, True)), r.hard)
    parity_report({"test": "lhs_vs_oracle", "case": C.id_of(shape, 2), "S": S, "worst_over_bound": worst,
                   "excluded_rows": int(r.rows_out.sum()), "rows": int(r.rows_out.size)})


# ------------------------------------------------------------------ e. K.shift_init
@pytest.mark.parametrize("shape,S", FIVE_S)
def test_shift_init_vs_oracle(K, shape, S):
    """Shift init, mode 0 (init_v_beta) and mode 1 (init_v): alpha to 1e-6, the sign of beta
    exactly, the squared-error side output against the oracle's float64 sums to 1e-6."""
    r = C.init_ref(shape, S, 2)
    c = r.case
    w, d, z = dev(c.w), dev(c.delta), dev(c.zp)
    alpha, beta, mse = K.shift_init(w, d, c.shifts)
    close(host(alpha), r.alpha0, atol=1e-6)
    np.testing.assert_array_equal(host(beta) >= 0, r.beta0 >= 0)
    close(host(mse), r.mse0, rtol=1e-6, atol=0.0)
    alpha1, beta1, mse1 = K.shift_init(w, d, c.shifts, zp=z, n_bits=2, mode=1)
    assert beta1 is None
    close(host(alpha1), r.alpha1, atol=1e-6)
    close(host(mse1), r.mse1, rtol=1e-6, atol=0.0)
    parity_report({"test": "shift_init_vs_oracle", "case": C.id_of(shape, 2), "S": S,
                   "alpha_over_tol": max(tol_ratio(host(alpha), r.alpha0, 1e-5, 1e-6),
                                         tol_ratio(host(alpha1), r.alpha1, 1e-5, 1e-6)),
                   "mse_over_tol": max(tol_ratio(host(mse), r.mse0, 1e-6, 0.0),
                                       tol_ratio(host(mse1), r.mse1, 1e-6, 0.0)),
                   "excluded_rows": 0})


# ------------------------------------------------------------------ f. K.adaround
def _round_regs(b_):
    return (None, (ROUND_LAMBDA, b_, None), (0.0, 0.0, dev([ROUND_LAMBDA, b_])))


def _gbeta_ratio(got, r, reg, b_):
    """gbeta against the oracle at rtol 1e-4, atol 1e-7.  With the rounding regulariser
    folded in, the kernel adds two fp32 terms of opposite sign wherever the regulariser
    pulls against the data gradient, and in a few of 2.4 M elements they cancel to 1e-3 of
    their size: each term's own fp32 rounding (6e-8 of it) is then 1e-4 of the sum.  So rtol
    is taken of |data term| + |regulariser term|, what each is held to alone, not of
    their sum."""
    ref = r.gbeta.astype(np.float64)
    if reg is None:
        return tol_ratio(got, ref, 1e-4, 1e-7, r.out)
    g_reg = R.reg_round(r.case.beta, b_, ROUND_LAMBDA)[1]
    return tol_ratio(got, ref + g_reg, 1e-4, 1e-7, r.out, mag=np.abs(ref) + np.abs(g_reg))


@pytest.mark.parametrize("shape", C.ADAROUND_SHAPES, ids=C.id_of)
def test_adaround_vs_oracle(K, shape):
    """AdaRound forward / backward with delta per output row and per (co, ci) (K.get_delta of
    a perturbed alpha, bit-exact against R.get_delta), scale 1 and 33/32, without and with
    the folded rounding regulariser (host floats and the device pair): gbeta to 1e-4 (+1e-7)
    against R.adaround_bwd (+ R.reg_round's gradient)."""
    worst, n_out, n = 0.0, 0, 0
    for per_ci in (False, True):
        for scale in C.ADAROUND_SCALES:
            r = C.adaround_ref(shape, 2, per_ci, scale)
            c = r.case
            w, _, z, alpha, beta, gy = on_device(c)
            if per_ci:
                dd = K.get_delta(dev(c.delta), alpha, c.shifts, shape)
                np.testing.assert_array_equal(host(dd), r.delta)
            else:
                dd = dev(c.delta)
            np.testing.assert_array_equal(host(K.adaround(beta, w, dd, z, 2, False, True, scale)), r.hard)
            close(host(K.adaround(beta, w, dd, z, 2, False, False, scale)), r.soft, atol=1e-7)
            for b_ in REG_B:
                for reg in _round_regs(b_):
                    b = beta.clone().requires_grad_(True)
                    K.adaround(b, w, dd, z, 2, False, False, scale, reg=reg).backward(gy)
                    ratio = _gbeta_ratio(host(b.grad), r, reg, b_)
                    assert ratio <= 1.0, (per_ci, scale, b_, reg is not None, ratio)
                    worst = max(worst, ratio)
            n_out, n = max(n_out, int(r.out.sum())), r.out.size
    parity_report({"test": "adaround_vs_oracle", "case": C.id_of(shape, 2), "worst_over_tol": worst,
                   "excluded_elements": n_out, "elements": n})


# ------------------------------------------------------------------ g. K.adaround_multi
def test_adaround_multi_vs_oracle(K):
    """11 weights in one K.adaround_multi call (more than the 8-segment table: a second
    launch), sizes around the 512-element tile, mixed bits / delta forms / scales and one
    Linear weight: hard forward bit-exact against R.adaround_fwd, soft forward and backward
    as K.adaround's, and every output bit-identical to the single-weight K.adaround."""
    refs = [C.adaround_ref(*spec) for spec in C.ADAROUND_MULTI]
    betas, entries, gys = [], [], []
    for (shape, bits, per_ci, scale), r in zip(C.ADAROUND_MULTI, refs):
        c = r.case
        betas.append(dev(c.beta))
        entries.append((dev(c.w), dev(r.delta), dev(c.zp), bits, False, scale))
        gys.append(dev(c.gy))
    for y, r in zip(K.adaround_multi(betas, entries, True), refs):
        np.testing.assert_array_equal(host(y), r.hard)
    worst, n_out, n = 0.0, 0, 0
    for reg in _round_regs(7.5):
        bm = [b.clone().requires_grad_(True) for b in betas]
        ys = K.adaround_multi(bm, entries, False, reg=reg)
        torch.autograd.backward(list(ys), gys)
        for k, (spec, r) in enumerate(zip(C.ADAROUND_MULTI, refs)):
            w, dd, z, bits, _, scale = entries[k]
            b1 = betas[k].clone().requires_grad_(True)
            y1 = K.adaround(b1, w, dd, z, bits, False, False, scale, reg=reg)
            y1.backward(gys[k])
            np.testing.assert_array_equal(host(ys[k]), host(y1), err_msg=str(spec))
            np.testing.assert_array_equal(host(bm[k].grad), host(b1.grad), err_msg=str(spec))
            close(host(ys[k]), r.soft, atol=1e-7)
            ratio = _gbeta_ratio(host(bm[k].grad), r, reg, 7.5)
            assert ratio <= 1.0, (spec, reg is not None, ratio)
            worst = max(worst, ratio)
    n_out, n = sum(int(r.out.sum()) for r in refs), sum(r.out.size for r in refs)
    parity_report({"test": "adaround_multi_vs_oracle", "segments": len(refs), "worst_over_tol": worst,
                   "excluded_elements": n_out, "elements": n})
