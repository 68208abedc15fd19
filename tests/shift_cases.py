"""Seeded cases for the shift-selection kernels (K5-K9) at their tiling edges, with the fp64
oracle's references, the rows the comparison leaves out and the alpha-gradient bound.
Shared by tests/test_shift_grads_host.py (oracle alone) and tests/test_shift_grads_gpu.py.

A case is a weight shape, a shift count S and a bit width; everything is built from
oracle.ssq_ref and numpy, so the references never depend on a kernel.

Boundary-fragile entries.  Kernel and oracle compute p = soft_targets(alpha) and
sigmoid(beta) with different exp / divide roundings, so they may differ by an ulp.  Where
that ulp can flip a clamp mask the two legitimately disagree by a whole element's
contribution, and such entries are left out of the comparison:
  * element-fragile: u = x_floor + h + zp lies within 2^-18 * max(1, |u|) of qmin or qmax
    without being equal to it (exact hits stay: they test that the mask is inclusive);
  * row-fragile: a softmax(alpha) * ZMG + GAMMA (or sigmoid(beta) * ZMG + GAMMA) value lies
    within 2^-20 of 0 or 1.
A conv input channel is left out of the alpha comparison when its alpha row or any of its
elements is fragile; a Linear weight and gbeta leave out only the fragile elements.  How much
a case may leave out is capped (check_caps); the seeds below are chosen so that the oracle
alone meets the caps (asserted by tests/test_shift_grads_host.py).
"""
import functools
import types

import numpy as np

from oracle import ssq_ref as R

F32 = np.float32
SHIFTS8 = [31 / 32, 33 / 32, 1.0, 17 / 16, 15 / 16, 35 / 32, 29 / 32, 9 / 8]
ELEM_EPS = 2.0 ** -18
ROW_EPS = 2.0 ** -20
ALPHA_BOUND = 16 * 2.0 ** -23      # in units of G = ZMG * max_i |g_p[row, i]|

# Each shape is there for one edge of the backward tilings (col_tiling for the recomputing
# kernels; bwd_tiling_prep / col_tiling_prep for the prepared ones; 256-thread workgroups,
# kRB = 4 rows per load batch, kRBP = 8 in the prepared column form, stage 2 sums 64 chunk
# partials per round).
GOLDEN_SHAPES = [
    (8, 6, 3, 3),        # the goldens' conv size: 1 column block, R = 1; prepared per-channel, 1 batch
    (6, 1, 3, 3),        # depthwise: one input channel, alpha (1, S)
    (10, 12),            # the goldens' Linear size
]
CONV_SHAPES = [
    (143, 9, 3, 3),      # R = 1, 143 chunks: 3 stage-2 rounds | per-channel, Co*K = 1287: 2 batches, 7 elements in the second
    (200, 37, 3, 3),     # 2 column blocks (28 + 9 channels), 200 chunks: 4 rounds | per-channel, 2 batches, 37 channels over 8 XCDs
    (257, 9, 3, 3),      # R = 2, 129 chunks, last chunk 1 row (tail loop only) | Co*K = 2313 > 2304: column form, R = 8, 33 chunks, last 1 row
    (1027, 7, 1, 1),     # R = 5 (batch of 4 + tail 1), 206 chunks: 4 rounds, last chunk 2 rows | 1x1 with Co > 256: column form, 129 chunks, last 3 rows
    (257, 300, 1, 1),    # 2 column blocks of 256 and 44 channels, R = 2, 129 chunks | column form, ragged block, 33 chunks
    (10, 3, 17, 17),     # K = 289 > 256: ncb = 1, 320 threads, 31 idle | the prepared path refuses it
    (33, 5, 5, 5),       # K = 25 does not divide the 256-thread tile (125 of 128 threads) | per-channel, 1 batch
    (512, 512, 3, 3),    # 19 column blocks, R = 5 (4 + 1), 103 chunks: the one large case | column form, R = 8, 64 chunks
]
FC_SHAPES = [
    (64, 300),           # Linear: per-element alpha (alpha_grad_fc)
    (1000, 37),          # Linear: 37000 elements, ragged last workgroup
]
ALL_SHAPES = GOLDEN_SHAPES + CONV_SHAPES + FC_SHAPES
# bits = 2 everywhere, 4 on three shapes (a second batch, a ragged column block, a Linear)
CASES = [(s, 2) for s in ALL_SHAPES] + [((143, 9, 3, 3), 4), ((257, 300, 1, 1), 4), ((64, 300), 4)]
PREP_CASES = [(s, b) for s, b in CASES if len(s) == 4 and s[2] * s[3] <= 256]
FIVE_SHAPES = [(143, 9, 3, 3), (1027, 7, 1, 1), (10, 3, 17, 17), (200, 37, 3, 3), (64, 300)]
LHS_COUNTS = (2, 3, 5)
ADAROUND_SCALES = (1.0, 33 / 32)
# adaround is elementwise: the edges are the per-(co,ci) delta's index, K > 256, a Linear
# weight, and more than 4096 * 256 elements (the grid-stride loop's second pass)
ADAROUND_SHAPES = [(8, 6, 3, 3), (143, 9, 3, 3), (10, 3, 17, 17), (200, 37, 3, 3), (64, 300),
                   (512, 512, 3, 3)]
# ssq_adaround_*_multi: 11 weights (more than the 8-segment table), sizes around the
# 512-element tile and 2^k +- 1; (shape, bits, per-(co,ci) delta, scale)
ADAROUND_MULTI = [
    ((6, 1, 3, 3), 2, False, 1.0),          # 54
    ((64, 8, 1, 1), 4, True, 33 / 32),      # 512
    ((27, 19, 1, 1), 2, True, 1.0),         # 513
    ((73, 7, 1, 1), 4, False, 33 / 32),     # 511
    ((33, 31, 1, 1), 2, True, 33 / 32),     # 1023
    ((25, 41), 4, True, 1.0),               # 1025, Linear
    ((23, 89, 1, 1), 2, False, 1.0),        # 2047
    ((683, 3, 1, 1), 2, True, 33 / 32),     # 2049
    ((65, 7, 3, 3), 4, True, 1.0),          # 4095
    ((241, 17, 1, 1), 2, False, 33 / 32),   # 4097
    ((8, 6, 3, 3), 2, True, 1.0),           # 432
]

SHIFT_COUNTS = (1, 2, 3, 4, 5, 8)       # 5 and 8 take the generic (NS == 0) instantiations


def shift_counts(bits, upto=8):
    """The S values a bit width is crossed with.  Every hard-rounding case must hold exact
    clamp hits (u == qmin or qmax), which at hard rounding needs an integer soft floor:
    sum_i p_i is 1 for S <= 2 but 1.2 - 0.1 * S (0.9 at S = 3) beyond, so x_floor is an
    integer only where every floor is 0, and then u = h + zp reaches qmax = 3 at 2 bits
    (zp = 2) but never 15 at 4 bits (zp <= 8).  So 4 bits is crossed with S <= 2 only."""
    return tuple(S for S in SHIFT_COUNTS if S <= upto and (bits == 2 or S <= 2))


# S = 2 on wide weights.  p_0 + p_1 is 1 in exact arithmetic, so an element whose two floors
# are equal (most are) and whose h is an integer (hard rounding, or a clamped soft h) has
# u = F + h + zp on the integer grid, and wherever that integer is qmin or qmax the element
# sits ON the clamp bound in exact arithmetic.  In fp32, fl(fl(F * p_0) + fl(F * p_1)) is F
# for most alpha rows and F -+ 1 ulp for the others (13 - 16 % of the rows of these cases,
# from the oracle alone): in such a row every element at a bound is element-fragile, and a
# row has hundreds of them, so no seed keeps 99 % of several hundred rows clear.  For the
# shapes below, at S = 2, the fragile rows whose p-sum is inexact ("structural") are left out
# without counting towards the caps; the caps hold for all other fragile rows, and at least
# three quarters of the case's rows must remain compared.  Narrower shapes (and every other
# S) keep the caps as they are, met by the choice of seed.
S2_STRUCTURAL = {(257, 300, 1, 1), (512, 512, 3, 3), (64, 300), (1000, 37)}
S2_MIN_KEPT = 0.75

# seed per (shape, S, bits); 7 unless the oracle's own fragile set missed a cap with it
DEFAULT_SEED = 7
SEEDS = {
    ((8, 6, 3, 3), 2, 2): 8, ((8, 6, 3, 3), 5, 2): 8, ((6, 1, 3, 3), 2, 2): 8, ((10, 12), 2, 2): 43,
    ((143, 9, 3, 3), 2, 2): 24, ((143, 9, 3, 3), 3, 2): 8, ((200, 37, 3, 3), 2, 2): 15,
    ((257, 9, 3, 3), 8, 2): 8, ((1027, 7, 1, 1), 2, 2): 12, ((10, 3, 17, 17), 2, 2): 8,
    ((143, 9, 3, 3), 2, 4): 65,
}


def seed_of(shape, S, bits):
    return SEEDS.get((tuple(shape), S, bits), DEFAULT_SEED)


def id_of(shape, bits=None):
    s = "x".join(str(v) for v in shape)
    return s if bits is None else f"{s}-b{bits}"


@functools.lru_cache(maxsize=None)
def make_case(shape, S, bits, seed=None):
    """The inputs of one case, all float32 and read-only."""
    shape = tuple(shape)
    if seed is None:
        seed = seed_of(shape, S, bits)
    rng = np.random.default_rng(seed)
    w = (0.05 * rng.standard_normal(shape)).astype(F32)
    delta, zp, _ = R.init_scale(w, bits, False, True, "max")
    shifts = SHIFTS8[:S]
    xq, alpha, beta = R.init_v_beta(w, delta, shifts)
    alpha = (alpha + (0.5 * rng.standard_normal(alpha.shape)).astype(F32)).astype(F32)
    beta = (beta + (0.5 * rng.standard_normal(beta.shape)).astype(F32)).astype(F32)
    gy = rng.standard_normal(shape).astype(F32)
    lo, hi = R.qrange(bits, False)
    c = types.SimpleNamespace(shape=shape, S=S, bits=bits, seed=seed, shifts=shifts, w=w, delta=delta,
                              zp=zp, xq=xq, alpha=alpha, beta=beta, gy=gy, is_fc=len(shape) != 4,
                              lo=lo, hi=hi)
    for a in [w, delta, zp, alpha, beta, gy] + list(xq):
        a.setflags(write=False)
    return c


def n_channels(c):
    return c.shape[1]


# ------------------------------------------------------------------ fragile entries
def _near(u, bound, eps):
    u = u.astype(np.float64)
    return (np.abs(u - bound) <= eps * np.maximum(1.0, np.abs(u))) & (u != bound)


def clamp_fragile(u, lo, hi):
    """(element-fragile, exact hit) of the rounding clamp's argument u."""
    return _near(u, lo, ELEM_EPS) | _near(u, hi, ELEM_EPS), (u == lo) | (u == hi)


def alpha_row_fragile(alpha):
    u = (R.softmax(alpha) * R.ZMG + R.GAMMA).astype(np.float64)
    return ((np.abs(u) <= ROW_EPS) | (np.abs(u - 1.0) <= ROW_EPS)).any(axis=-1)


def beta_fragile(beta):
    u = (R.sigmoid(beta) * R.ZMG + R.GAMMA).astype(np.float64)
    return (np.abs(u) <= ROW_EPS) | (np.abs(u - 1.0) <= ROW_EPS)


def _rows_of_elements(c, elem):
    """Alpha rows touched by a set of elements: conv -> input channels, Linear -> itself."""
    return elem if c.is_fc else elem.any(axis=(0, 2, 3))


def s2_inexact_rows(c):
    """S = 2: alpha rows where fl(fl(F * p_0) + fl(F * p_1)) != F for a floor F in range."""
    p = R.sig_soft_targets(c.alpha)
    bad = np.zeros(p.shape[:-1], bool)
    for F in range(1, c.hi - c.lo + 2):
        bad |= (F32(F) * p[..., 0] + F32(F) * p[..., 1]) != F32(F)
    return bad


def check_caps(c, rows_out=None, elems_out=None):
    """The caps on what a comparison may leave out (conditions, not measurements).
    rows_out: excluded alpha rows; elems_out: excluded elements of an elementwise comparison."""
    if rows_out is not None and c.S == 2 and c.shape in S2_STRUCTURAL:
        assert rows_out.sum() <= (1.0 - S2_MIN_KEPT) * rows_out.size, (c.shape, c.bits, int(rows_out.sum()))
        rows_out = rows_out & ~s2_inexact_rows(c)
    if rows_out is not None:
        n_out = int(rows_out.sum())
        if c.is_fc:                                  # per-element alpha: the elementwise cap
            assert n_out <= int(0.001 * rows_out.size), (c.shape, c.S, c.bits, n_out, rows_out.size)
        elif n_channels(c) < 16:
            assert n_out == 0, (c.shape, c.S, c.bits, n_out)
        else:
            assert n_out <= max(1, int(0.01 * n_channels(c))), (c.shape, c.S, c.bits, n_out)
    if elems_out is not None:
        n_out = int(elems_out.sum())
        assert n_out <= int(0.001 * elems_out.size), (c.shape, c.S, c.bits, n_out, elems_out.size)


# ------------------------------------------------------------------ adaShift references
@functools.lru_cache(maxsize=None)
def adashift_ref(shape, S, bits, hard_r):
    """The oracle's backward of one case: galpha (float64), gbeta, g_p (the float64 sums of
    g_int * F_i, the alpha gradient's scale), the excluded alpha rows / gbeta elements and
    the number of exact clamp hits."""
    c = make_case(tuple(shape), S, bits)
    galpha, gbeta = R.adashift_bwd(c.xq, c.alpha, c.beta, c.delta, c.zp, bits, False, c.is_fc,
                                   bool(hard_r), c.gy)
    # g_p as R.adashift_bwd forms it (same fp32 ops, same float64 sums)
    x_floor = R.shifted_x_quant(c.xq, c.alpha, c.is_fc, False)
    h = (c.beta >= 0).astype(F32) if hard_r else R.soft_round(c.beta)
    u = (x_floor + h) + c.zp
    m = (u >= c.lo) & (u <= c.hi)
    g_int = np.where(m, c.gy * (c.delta * F32(1.0)), F32(0)).astype(np.float64)
    if c.is_fc:
        g_p = np.stack([g_int * q for q in c.xq], axis=-1)
    else:
        g_p = np.stack([(g_int * q).sum(axis=(0, 2, 3)) for q in c.xq], axis=-1)
    g_p = g_p.reshape(c.alpha.shape)
    elem, exact = clamp_fragile(u, c.lo, c.hi)
    rows_out = alpha_row_fragile(c.alpha) | _rows_of_elements(c, elem)
    beta_out = None if hard_r else (elem | beta_fragile(c.beta))
    structural = S == 2 and c.shape in S2_STRUCTURAL
    return types.SimpleNamespace(case=c, galpha=galpha, gbeta=gbeta, g_p=g_p, rows_out=rows_out,
                                 beta_out=beta_out, n_exact=int(exact.sum()), elem=elem,
                                 n_structural=int((rows_out & s2_inexact_rows(c)).sum()) if structural else 0)


def reg_gp(alpha, lam, b):
    """d(shift regulariser)/dp, the term the fused backward adds to g_p."""
    return R.round_reg(R.sig_soft_targets(alpha), b, lam)[1]


def alpha_scale(g_p):
    """G = ZMG * max_i |g_p[row, i]| per alpha row."""
    return float(R.ZMG) * np.abs(g_p).max(axis=-1)


def reg_slack(alpha, lam, b):
    """What the fused regulariser adds to the alpha bound, per row.  The bound's derivation
    takes g_p as exact on both sides.  That holds for the float64 sums of g_int * F_i, but the
    kernels evaluate the regulariser's d/dp_i = -lam * b * r^(b-1) * 2 * sign(p_i - 0.5),
    r = 2 |p_i - 0.5|, in fp32 from their own p_i, as the reference's tensor ops do.  Their p_i
    is off by up to dp = 8 * 2^-24 (4 ulp of s_i times ZMG = 4.8, the product's and the sum's
    roundings 2.2, in ulps of 1), which moves the term by |d2/dp2| * dp with
    d2/dp2 = 4 * lam * b * (b-1) * r^(b-2); powf and the four fp32 products add 8 * 2^-24 of
    the term itself; and below fp32's normal range the term is lost (2^-120 covers it).  An
    error e_i on g_p moves galpha_i = s_i * ZMG * (g_i - sum_j s_j g_j) by at most
    ZMG * 2 s_i (1 - s_i) * max|e| <= 0.5 * ZMG * max|e|."""
    p = R.sig_soft_targets(alpha).astype(np.float64)
    r = np.abs(p - 0.5) * 2
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = 4.0 * lam * b * abs(b - 1.0) * np.where((r == 0) & (b < 2), np.inf, r ** (b - 2.0))
    g = np.abs(R.round_reg(p.astype(F32), b, lam)[1])
    e = (d2 * 8 * 2.0 ** -24 + g * 8 * 2.0 ** -24).max(axis=-1)
    return 0.5 * float(R.ZMG) * e + 2.0 ** -120


def alpha_ratio(got, ref, g_p, rows_out, slack=None):
    """Worst |got - ref| / (ALPHA_BOUND * G [+ slack]) over the rows kept (0 / 0 counts as 0,
    anything over a zero bound as inf); slack = reg_slack(...) when the regulariser is fused."""
    err = np.abs(np.asarray(got, np.float64) - ref).max(axis=-1)
    bound = ALPHA_BOUND * alpha_scale(g_p)
    if slack is not None:
        bound = bound + slack
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    ratio = np.where(rows_out, 0.0, ratio)
    return float(ratio.max(initial=0.0))


# ------------------------------------------------------------------ lhs / shift init references
@functools.lru_cache(maxsize=None)
def lhs_ref(shape, S, bits):
    """learned_hard_sigmoid on the case's alpha with the dequantized candidates of R.init_v."""
    c = make_case(tuple(shape), S, bits)
    xq, alpha0 = R.init_v(c.w, c.delta, c.zp, bits, False, c.shifts)
    gy64 = c.gy.astype(np.float64)
    if c.is_fc:
        g_p = np.stack([gy64 * q for q in xq], axis=-1)
    else:
        g_p = np.stack([(gy64 * q).sum(axis=(0, 2, 3)) for q in xq], axis=-1)
    g_p = g_p.reshape(c.alpha.shape)
    return types.SimpleNamespace(case=c, xq=xq, alpha0=alpha0, g_p=g_p,
                                 galpha=R.lhs_bwd(xq, c.alpha, c.is_fc, c.gy),
                                 soft=R.shifted_x_quant(xq, c.alpha, c.is_fc, False),
                                 hard=R.shifted_x_quant(xq, c.alpha, c.is_fc, True),
                                 rows_out=alpha_row_fragile(c.alpha))


def init_mse(w, xq, is_fc):
    """init_alpha's squared errors (fp32 per element, summed in float64), laid out as alpha."""
    if is_fc:
        return np.stack([((w - q) ** 2).astype(np.float64) for q in xq], axis=-1)
    return np.stack([((w - q) ** 2).astype(np.float64).sum(axis=(0, 2, 3)) for q in xq], axis=-1)


# ------------------------------------------------------------------ adaround references
def adaround_inputs(shape, bits, per_ci, seed=None):
    """(case, delta): the S = 3 case's weight / beta / gy, delta per output row or per
    (co, ci) = R.get_delta of the case's perturbed alpha."""
    c = make_case(tuple(shape), 3, bits, seed)
    d = R.get_delta(c.delta, c.alpha, c.shifts, c.is_fc) if per_ci else c.delta
    return c, d


@functools.lru_cache(maxsize=None)
def adaround_ref(shape, bits, per_ci, scale, seed=None):
    c, d = adaround_inputs(shape, bits, per_ci, seed)
    ds = d * F32(scale)
    u = (np.floor(c.w / ds) + R.soft_round(c.beta)) + c.zp
    elem, exact = clamp_fragile(u, c.lo, c.hi)
    return types.SimpleNamespace(
        case=c, delta=d,
        gbeta=R.adaround_bwd(c.w, c.beta, d, c.zp, bits, False, c.gy, scale),
        soft=R.adaround_fwd(c.w, c.beta, d, c.zp, bits, False, False, scale),
        hard=R.adaround_fwd(c.w, c.beta, d, c.zp, bits, False, True, scale),
        out=elem | beta_fragile(c.beta), n_exact=int(exact.sum()))


# ------------------------------------------------------------------ the oracle alone
def check_case(shape, S, bits):
    """Every condition a case must meet before any kernel is compared with it: the caps on
    what each comparison leaves out and exact clamp hits at hard rounding.  Returns the counts."""
    out = {}
    for hard_r in (0, 1):
        r = adashift_ref(shape, S, bits, hard_r)
        check_caps(r.case, rows_out=r.rows_out, elems_out=r.beta_out)
        if hard_r:
            assert r.n_exact >= 1, (shape, S, bits, "no exact clamp hit at hard rounding")
        out[f"hr{hard_r}"] = (int(r.rows_out.sum()), r.n_exact)
    if shape in FIVE_SHAPES and S in LHS_COUNTS and bits == 2:
        r = lhs_ref(shape, S, bits)
        check_caps(r.case, rows_out=r.rows_out)
    if shape in ADAROUND_SHAPES and S == 3 and bits == 2:
        for per_ci in (False, True):
            for scale in ADAROUND_SCALES:
                r = adaround_ref(shape, bits, per_ci, scale)
                check_caps(r.case, elems_out=r.out)
    return out


@functools.lru_cache(maxsize=None)
def init_ref(shape, S, bits):
    """Shift init on the case's weight: mode 0 (init_v_beta: integer floors) and mode 1
    (init_v: dequantized candidates) alphas, mode 0's beta, and both modes' squared errors."""
    c = make_case(tuple(shape), S, bits)
    xq0, alpha0, beta0 = R.init_v_beta(c.w, c.delta, c.shifts)
    xq1, alpha1 = R.init_v(c.w, c.delta, c.zp, bits, False, c.shifts)
    return types.SimpleNamespace(case=c, alpha0=alpha0, beta0=beta0, alpha1=alpha1,
                                 mse0=init_mse(c.w, xq0, c.is_fc), mse1=init_mse(c.w, xq1, c.is_fc))
