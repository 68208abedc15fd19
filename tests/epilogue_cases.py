"""Seeded cases for the K13 epilogue family (forward bias_act_kernel, backward
epilogue_bwd_rows, the fused tail and the fin_epi / fin_loss_rows finalizes of
csrc/recon.hip and csrc/fin_tasks.h) at the edges of their forms, with the fp64 oracle's
references, the coverage conditions of the inputs and the derived bound of the sums.
Shared by tests/test_epilogue_host.py (oracle alone, form queries), tests/test_epilogue_oracle_gpu.py
and tests/epilogue_worker.py.

A case is (N, C, H, W) plus flags; everything is built from numpy and oracle.ssq_ref, so the
references never depend on a kernel.  Rows = N * C, hw = H * W.

Forms (ssq_epilogue_bwd_form -> rows per wave, float4 rows; ssq_epilogue_fwd_form -> 0/1/2):
  backward  16: rows of <= 64 elements / float4s, 4 rows per wave, 16 lanes per row, a lane
                holds elements l16 + 16k (k < 4): nv = 1, 15/16/17, 63/64 matter, rows % 4
                (the clamp of the rows past the end) and rows % 16 (the last workgroup);
            1:  a row per wave in 64-lane strides;
            4:  the A/B register form (SSQ_EPI_G16=0), reached by tests/epilogue_worker.py.
  forward   2: float4s inside one plane (hw % 4 == 0); 1: float4s across planes (n % 4 == 0);
            0: scalar (odd n, a misaligned tensor, a row map with hw % 4 != 0).

Coverage conditions (check_coverage; the seeds below are chosen so that the oracle alone
meets them, asserted by tests/test_epilogue_host.py):
  * ReLU / ReLU6: between 25 % and 75 % of the elements are masked by the activation;
  * act quantizer: at least 50 % in range and at least 5 % clipped at each end the
    activation's output can reach.  A ReLU / ReLU6 output is >= 0 and every case has zp >= 0,
    so round(t / delta) + zp >= qmin = 0 always holds there: the lower end is reachable only
    with activation 0, and only those cases are asked for it;
  * wherever hw >= 8 and the case has a mask at all, every (n, c) row and every channel holds
    both masked and unmasked elements.

The bound of a sum (sum_bound).  The kernels add exact double products of fp32 values in some
order and round once to fp32.  A float64 sum of n terms in any order is within (n - 1) *
2^-53 * A of the exact sum S, A the sum of the absolute terms (gdelta / gzp: of both sums
they subtract), and the rounding to fp32 adds at most half an ulp: so |got - S| <= ulp32(S) +
(n - 1) * 2^-53 * A.  At a tail power p != 2 the loss gradient goes through the hardware log2 /
exp2 and is only within K11's tolerance of the oracle's, so the oracle's sums of its own
gradient are no reference at this bound.  There the device's K11 kernel (lp_loss_rows, the same
lp_elem) is run on the oracle's output, its gradient is checked against the oracle's at K11's
tolerance, and the oracle's backward is restated from that gradient (ssq_ref.epilogue_loss_bwd's
g): gy, gres bit for bit and every sum inside the same bound, with no looser term.
"""
import functools
import types

import numpy as np

from oracle import ssq_ref as R

F32 = np.float32
LAZY_BIAS, LAZY_AFFINE = "lazy_bias", "lazy_affine"
LP_RTOL, LP_ATOL = 1e-5, 1e-9        # K11 (test_lp_loss_golden): gradients / loss at p != 2
LOSS_RTOL_P2 = 1e-6                  # the loss at p = 2 (row partials against block partials)


# seed: 7 unless the oracle's own coverage figures missed a condition with it
def _c(shape, edge, kind="bwd", bias=True, affine=True, res=None, act=1, q=None, need_dy=True,
       want_gres=True, p=2.0, mis=False, view=False, form=None, fwd=None, seed=7, defer=False,
       special=False):
    N, C, H, W = shape
    return types.SimpleNamespace(
        shape=tuple(shape), N=N, C=C, hw=H * W, rows=N * C, edge=edge, kind=kind, bias=bias,
        affine=affine, res=res, act=act, q=q, need_dy=need_dy, want_gres=want_gres, p=p, mis=mis,
        view=view, form=form, fwd=fwd, seed=seed, defer=defer, special=special)


Q4Z0, Q4Z3, Q8 = (4, 0.0), (4, 3.0), (8, 0.0)
G16S, G16V, R1V, R1S = (16, False), (16, True), (1, True), (1, False)

# ---------------------------------------------------------------- the plain backward (+ forward)
BWD = [
    # kG16 scalar rows
    _c((2, 3, 1, 1), "hw 1: nv = 1, one lane of 16 works; rows 6 (% 4 = 2: clamped rows)", form=G16S, fwd=0,
       res="tensor", q=Q4Z0, seed=8),
    _c((1, 1, 3, 5), "hw 15: nv = 15, lane 15 idle; rows = 1, N = 1, C = 1", form=G16S, fwd=0,
       bias=False, act=0, q=Q4Z3),
    _c((1, 3, 1, 17), "hw 17: nv = 17, lane 0 holds a second element; rows = 3", form=G16S, fwd=0,
       affine=False, res="tensor", act=2),
    _c((5, 1, 7, 7), "hw 49; rows = 5, C = 1 (one channel over 5 samples: waves 0..3 then wave 0 again)",
       form=G16S, fwd=0, q=Q8, seed=8),
    _c((3, 5, 7, 9), "hw 63: nv = 63, every lane but one holds 4; rows = 15 (% 16: last workgroup short by one)",
       form=G16S, fwd=0, bias=False, affine=False, res="tensor", act=0, q=Q4Z0),
    # kG16 float4 rows
    _c((1, 17, 2, 2), "hw 4: nv = 1 float4; rows = 17 (a second workgroup of one row)", form=G16V, fwd=2,
       res="tensor", act=2, q=Q4Z3),
    _c((2, 63, 8, 8), "hw 64: nv = 16, each lane one float4; C = 63 (one short of fin_epi's 64); no dy",
       form=G16V, fwd=2, need_dy=False),
    _c((3, 64, 4, 17), "hw 68: nv = 17; C = 64 (exactly one fin_epi workgroup), N = 3 < 4 waves; gres not wanted",
       form=G16V, fwd=2, bias=False, res="tensor", act=0, q=Q8, want_gres=False),
    _c((5, 65, 14, 14), "hw 196: nv = 49; C = 65 (a second fin_epi workgroup of one channel), N = 5",
       form=G16V, fwd=2, res="tensor", q=Q4Z0),
    _c((9, 130, 14, 18), "hw 252: nv = 63; C = 130 (three fin_epi workgroups), N = 9; 1170 rows: 2 delta workgroups",
       form=G16V, fwd=2, affine=False, act=2, q=Q4Z0),
    _c((1, 130, 16, 16), "hw 256: nv = 64, every lane 4 float4s; N = 1 (waves 1..3 of fin_epi sum nothing)",
       form=G16V, fwd=2, res="tensor", q=Q4Z3),
    # a row per wave, float4
    _c((2, 63, 13, 20), "hw 260: nv = 65, one lane in the second 64-lane stride", form=R1V, fwd=2,
       res="tensor", q=Q4Z0),
    _c((1, 5, 28, 28), "hw 784: 196 float4s, 4 strides with lanes 4.. idle in the last", form=R1V, fwd=2,
       bias=False, act=0, q=Q4Z3),
    # a row per wave, scalar
    _c((3, 65, 5, 13), "hw 65: one element in the second stride; C = 65, N = 3", form=R1S, fwd=0,
       res="tensor", q=Q8),
    _c((9, 1, 9, 9), "hw 81; C = 1, N = 9: fin_epi's waves sum 3, 2, 2, 2 samples", form=R1S, fwd=0, act=2),
    _c((5, 64, 15, 15), "hw 225; C = 64, N = 5; no dy; n % 4 == 0: the forward's form 1", form=R1S, fwd=1, bias=False, affine=False,
       res="tensor", q=Q4Z3, need_dy=False),
    # hw % 4 == 0 with y 4 bytes into its buffer: the scalar fallback
    _c((2, 5, 8, 8), "hw 64, y not 16-B aligned: kG16 scalar with nv = 64 (every lane 4 elements)",
       form=G16S, fwd=0, res="tensor", q=Q4Z0, mis=True),
    _c((2, 5, 16, 16), "hw 256, y not 16-B aligned: a row per wave, scalar, 4 strides", form=R1S, fwd=0,
       res="tensor", act=0, q=Q4Z3, mis=True),
    # the delta / zero-point reduction of fin_epi
    _c((8, 128, 7, 7), "rows = 1024: one delta workgroup, its batch loop full", form=G16S, fwd=1, q=Q4Z0),
    _c((5, 205, 7, 7), "rows = 1025: two delta workgroups (513 + 512 rows), the ticket",
       form=G16S, fwd=0, act=0, q=Q4Z3, defer=True, seed=8),
    _c((33, 500, 2, 2), "rows = 16500: the 16-workgroup cap, 1032 rows each: a second batch trip; N = 33",
       form=G16V, fwd=2, q=Q4Z0, defer=True),
    # y and the residual read through row views: mapped() of the row-per-wave form
    _c((3, 5, 13, 20), "hw 260 through row views (duplicate rows): mapped() with float4 rows",
       form=R1V, fwd=2, res="tensor", q=Q4Z0, view=True),
    _c((3, 5, 5, 13), "hw 65 through row views: mapped() with scalar rows; the forward's row map forces form 0",
       form=R1S, fwd=0, res="tensor", q=Q4Z3, view=True),
]

# ---------------------------------------------------------------- the fused tail (LOSS forms)
TAIL = [
    _c((2, 3, 1, 1), "tail, hw 1, residual epilogue with a bias only", "tail", form=G16S, res=LAZY_BIAS, seed=8),
    _c((1, 5, 3, 5), "tail, hw 15, p = 2.4, N = 1", "tail", form=G16S, res="tensor", act=0, q=Q4Z3, p=2.4),
    _c((3, 5, 7, 7), "tail, hw 49, residual epilogue with gamma / phi (RES 2), rows = 15", "tail", form=G16S,
       res=LAZY_AFFINE, q=Q4Z0),
    _c((2, 17, 2, 2), "tail, hw 4, RES 2, p = 2.4, rows = 34", "tail", form=G16V, res=LAZY_AFFINE, p=2.4),
    _c((2, 63, 8, 8), "tail, hw 64, gres not wanted, 8-bit quantizer", "tail", form=G16V, res="tensor", q=Q8,
       want_gres=False),
    _c((3, 5, 4, 17), "tail, hw 68, no residual, no bias, identity", "tail", form=G16V, bias=False, act=0),
    _c((5, 13, 14, 14), "tail, hw 196, bias-only residual epilogue, p = 2.4", "tail", form=G16V,
       res=LAZY_BIAS, q=Q4Z0, p=2.4),
    _c((1, 65, 16, 16), "tail, hw 256 (nv = 64), RES 2, identity, zp 3", "tail", form=G16V,
       res=LAZY_AFFINE, act=0, q=Q4Z3),
    _c((2, 9, 13, 20), "tail, hw 260: a row per wave, float4, RES 2; the loss partial per 4 rows (18 rows: 5 partials)",
       "tail", form=R1V, res=LAZY_AFFINE, q=Q4Z0),
    _c((1, 3, 28, 28), "tail, hw 784, p = 2.4, rows = 3 (one workgroup, a wave past the end)", "tail", form=R1V,
       res="tensor", p=2.4),
    _c((3, 7, 5, 13), "tail, hw 65: a row per wave, scalar, bias-only residual epilogue", "tail", form=R1S,
       res=LAZY_BIAS, q=Q4Z3),
    _c((2, 3, 15, 15), "tail, hw 225, RES 2, identity, p = 2.4, 8-bit", "tail", form=R1S, res=LAZY_AFFINE,
       act=0, q=Q8, p=2.4, affine=False),
    _c((9, 130, 9, 9), "tail, hw 81, 1170 rows: 293 loss partials, 2 delta workgroups", "tail", form=R1S,
       res="tensor", q=Q4Z0),
    _c((2, 5, 8, 8), "tail, hw 64 with y not 16-B aligned: kG16 scalar", "tail", form=G16S, res="tensor",
       q=Q4Z0, mis=True),
    _c((2, 5, 16, 16), "tail, hw 256 with y not 16-B aligned: a row per wave, scalar, RES 2", "tail", form=R1S,
       res=LAZY_AFFINE, mis=True),
    _c((33, 500, 5, 13), "tail, 16500 rows at hw 65: 4125 loss partials, the second trip of fin_loss_rows",
       "tail", form=R1S, q=Q4Z0, defer=True),
    _c((3, 5, 13, 20), "tail, hw 260, the residual through a row view (duplicates)", "tail", form=R1V,
       res="tensor", q=Q4Z0, view=True),
    _c((3, 5, 5, 13), "tail, hw 65, y and the residual through row views, p = 2.4", "tail", form=R1S,
       res="tensor", p=2.4, view=True),
]

# ---------------------------------------------------------------- forward only
FWD = [
    _c((4, 3, 7, 7), "forward, hw 49 with n % 4 == 0: float4s straddle planes (form 1)", "fwd", fwd=1,
       res="tensor", q=Q4Z0),
    _c((3, 5, 7, 7), "forward, odd n = 735: the scalar form", "fwd", fwd=0, res="tensor", act=2, q=Q4Z3),
    _c((44, 1000, 7, 7), "forward, form 1 with n = 2156000 > 4 * 2048 * 256: a second grid-stride trip", "fwd",
       fwd=1, affine=False, q=Q4Z0),
    _c((3, 3567, 7, 7), "forward, scalar with n = 524349 > 2048 * 256: a second grid-stride trip", "fwd", fwd=0,
       res="tensor", act=0),
]

# -0.0, NaN, +-inf, 6.0 and its two neighbours, a denormal: forward, gy, gres bit for bit
# (a NaN wherever the oracle has one), each sum NaN exactly where the oracle's is
SPECIAL = _c((2, 4, 4, 4), "planted special values on ReLU6 + 4-bit quantizer, no bias, no affine", "bwd",
             form=G16V, fwd=2, bias=False, affine=False, res="tensor", act=2, q=Q4Z0, special=True)
SPECIAL_VALUES = [-0.0, np.nan, np.inf, -np.inf, 6.0, np.nextafter(F32(6), F32(0)),
                  np.nextafter(F32(6), F32(7)), 1e-41, 0.0, -1e-41]

CASES = BWD + TAIL + FWD + [SPECIAL]

# one case per plane class with affine + residual + quantizer on, and its twin without the
# quantizer (only that one can take the 4-rows register form): tests/epilogue_worker.py
WORKER = [
    _c((3, 5, 7, 7), "worker: small scalar plane", form=G16S, fwd=0, res="tensor", q=Q4Z0),
    _c((3, 5, 7, 7), "worker: small scalar plane, no quantizer", form=G16S, fwd=0, res="tensor"),
    _c((3, 5, 8, 8), "worker: small float4 plane", form=G16V, fwd=2, res="tensor", q=Q4Z0),
    _c((3, 5, 8, 8), "worker: small float4 plane, no quantizer", form=G16V, fwd=2, res="tensor"),
    _c((3, 5, 13, 20), "worker: long float4 plane", form=R1V, fwd=2, res="tensor", q=Q4Z0),
    _c((3, 5, 5, 13), "worker: long scalar plane", form=R1S, fwd=0, res="tensor", q=Q4Z0),
    _c((3, 5, 7, 7), "worker: tail, small scalar plane", "tail", form=G16S, res="tensor", q=Q4Z0),
    _c((3, 5, 8, 8), "worker: tail, small float4 plane, no quantizer", "tail", form=G16V, res="tensor"),
    _c((3, 5, 8, 8), "worker: tail, small float4 plane, RES 2", "tail", form=G16V, res=LAZY_AFFINE, q=Q4Z0),
    _c((4, 3, 7, 7), "worker: forward, n % 4 == 0 on hw 49", "fwd", fwd=1, res="tensor", q=Q4Z0),
]
# the A/B environments and the form each turns a small plane's plain backward / tail into:
# (quantizer off, quantizer on) for the backward, then for the tail (RES 2 is always 1)
WORKER_ENVS = {
    "g16_0": ({"SSQ_EPI_G16": "0"}, {"bwd": (4, 1), "tail": (1, 1)}),
    "g16_0_multi_2": ({"SSQ_EPI_G16": "0", "SSQ_EPI_MULTI_ROW": "2"}, {"bwd": (4, 1), "tail": (4, 1)}),
    "g16_0_multi_0": ({"SSQ_EPI_G16": "0", "SSQ_EPI_MULTI_ROW": "0"}, {"bwd": (1, 1), "tail": (1, 1)}),
    "plane4_0": ({"SSQ_K13_PLANE4": "0"}, None),
}


# The plain ABI entries (ssq_bias_act, ssq_bias_act_fq, ssq_epilogue_fwd, ssq_epilogue_bwd,
# ssq_epilogue_loss_bwd) against their _rows twins with null maps (tests/test_k13_glue_gpu.py;
# no Python wrapper calls the plain ones): every forward form with and without residual,
# activation 0 / 1 / 2, with and without a 4-bit quantizer, with gamma / phi (ssq_epilogue_fwd)
# and without; the backward on WORKER's four plane classes; the tail on the same four.
ENTRY_SEEDS = {"fwd-2x4x4x4-b1a0r1t0-q4z0": 2}     # (see _c's seed)
ENTRY_FWD = [
    _c(shape, "entry: forward form %d" % f, "fwd", fwd=f, affine=a, res=r, act=t, q=q)
    for shape, f in (((2, 3, 5, 5), 0), ((4, 3, 7, 7), 1), ((2, 4, 4, 4), 2))
    for a in (False, True) for r in (None, "tensor") for t in (0, 1, 2) for q in (None, Q4Z0)]
ENTRY_BWD = [c for c in WORKER if c.kind == "bwd"]
ENTRY_TAIL = [c for c in WORKER if c.kind == "tail"] + [
    _c((3, 5, 13, 20), "entry: tail, long float4 plane", "tail", form=R1V, res="tensor", q=Q4Z0),
    _c((3, 5, 5, 13), "entry: tail, long scalar plane", "tail", form=R1S, res=LAZY_BIAS, q=Q4Z0),
]


def case_id(c):
    s = f"{c.kind}-" + "x".join(str(v) for v in c.shape)
    s += f"-b{int(c.bias)}a{int(c.affine)}r{ {None: 0, 'tensor': 1, LAZY_BIAS: 2, LAZY_AFFINE: 3}[c.res] }t{c.act}"
    s += "-q" + ("0" if c.q is None else f"{c.q[0]}z{int(c.q[1])}")
    if c.kind == "tail":
        s += f"-p{c.p}"
    return s + ("-mis" if c.mis else "") + ("-view" if c.view else "") + ("-nody" if not c.need_dy else "")


def bwd_form_of(K, c):
    """What ssq_epilogue_bwd_form answers for the case's launch (K: the kernels module)."""
    return K.epilogue_bwd_form(c.hw, aligned=not c.mis, quant=c.q is not None,
                               res2=c.res in (LAZY_BIAS, LAZY_AFFINE), loss=c.kind == "tail")


def fwd_form_of(K, c):
    return K.epilogue_fwd_form(c.N * c.C * c.hw, c.hw, aligned=not c.mis, rows=c.view)


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def _choose_quantizer(t, act, n_bits, zp):
    """delta (and, with activation 0, a common offset of y) from the pre-quant activation t of
    the un-offset inputs: about 10 % of what can clip does so at each reachable end."""
    lo, hi = R.qrange(n_bits, False)
    if act == 0:
        a, b = np.quantile(t, 0.10), np.quantile(t, 0.90)
        d = (b - a) / (hi - lo + 1)
        # a -> (lo - zp - 0.5) * d
        return F32(d), F32((lo - zp - 0.5) * d - a)
    inner = t[(t > 0) & (t < 6)] if act == 2 else t[t > 0]
    if inner.size == 0:
        return F32(0.25), F32(0)
    return F32(np.quantile(inner, 0.75) / (hi - zp + 0.5)), F32(0)


@functools.lru_cache(maxsize=None)
def _inputs(key):
    c = BY_ID[key]
    N, C, H, W = c.shape
    rng = np.random.default_rng(c.seed)
    sc = F32(4.0 if c.act == 2 else 1.0)
    nrm = lambda *s: rng.standard_normal(s).astype(F32)
    x = types.SimpleNamespace(case=c)
    ncache = N + 3
    # idx: this batch's rows of the caches, with a duplicate wherever N >= 2
    idx = rng.permutation(ncache)[:N].astype(np.int64)
    if N >= 2:
        idx[-1] = idx[0]
    x.idx = idx
    x.ycache = x.rcache = None
    if c.view:
        x.ycache = sc * nrm(ncache, C, H, W)
        x.y = np.ascontiguousarray(x.ycache[idx])
    else:
        x.y = sc * nrm(N, C, H, W)
    x.bias = (F32(0.3) * nrm(C)) if c.bias else None
    x.gamma = (F32(1) + F32(0.1) * nrm(C)).astype(F32) if c.affine else None
    x.phi = (F32(0.1) * nrm(C)) if c.affine else None
    x.res = x.rbias = x.rgamma = x.rphi = None
    if c.res is not None:
        if c.view:
            x.rcache = sc * nrm(ncache, C, H, W)
            x.res = np.ascontiguousarray(x.rcache[idx])
        else:
            x.res = sc * nrm(N, C, H, W)
        if c.res in (LAZY_BIAS, LAZY_AFFINE):
            x.rbias = F32(0.3) * nrm(C)
        if c.res == LAZY_AFFINE:
            x.rgamma = (F32(1) + F32(0.1) * nrm(C)).astype(F32)
            x.rphi = F32(0.1) * nrm(C)
    x.g = nrm(N, C, H, W)
    x.tcache = np.maximum(sc * nrm(ncache, C, H, W), 0).astype(F32) if c.kind == "tail" else None
    x.res_epi = None if x.rbias is None else (x.rbias, x.rgamma, x.rphi)
    x.delta = x.zp = None
    x.n_bits = 8
    if c.special:
        flat = x.y.reshape(-1)
        pos = rng.permutation(flat.size)[:3 * len(SPECIAL_VALUES)]
        flat[pos] = np.tile(np.array(SPECIAL_VALUES, F32), 3)
        x.res.reshape(-1)[pos] = F32(0)       # the planted values reach the activation as they are
        x.res.reshape(-1)[pos[:2]] = F32(-0.0)
        x.n_bits, x.delta, x.zp = 4, F32(0.5), F32(0)
    elif c.q is not None:
        x.n_bits, zp = c.q[0], c.q[1]
        t = R.epilogue_fwd(x.y, x.bias, x.gamma, x.phi, x.res, c.act, res_epi=x.res_epi)[0]
        x.delta, off = _choose_quantizer(t.astype(np.float64), c.act, x.n_bits, zp)
        x.zp = F32(zp)
        if off != 0:
            x.y = (x.y + off).astype(F32)
            if x.ycache is not None:
                x.ycache = (x.ycache + off).astype(F32)
                x.y = np.ascontiguousarray(x.ycache[idx])
    x.M = N * H * W
    _ro(x.y, x.bias, x.gamma, x.phi, x.res, x.rbias, x.rgamma, x.rphi, x.g, x.tcache, x.ycache,
        x.rcache, x.idx)
    return x


def inputs(c):
    """The inputs of a case, all float32 and read-only."""
    return _inputs(case_id(c))


@functools.lru_cache(maxsize=None)
def _reference(key):
    c, x = BY_ID[key], _inputs(key)
    pre_q, out = R.epilogue_fwd(x.y, x.bias, x.gamma, x.phi, x.res, c.act, x.delta, x.zp, x.n_bits,
                                False, x.res_epi)
    if c.kind == "fwd":
        r = {}
    elif c.kind == "tail":
        r = R.epilogue_loss_bwd(x.tcache[x.idx], c.p, x.M, x.y, x.bias, x.gamma, x.phi, x.res, c.act,
                                x.delta, x.zp, x.n_bits, False, x.res_epi)
    else:
        r = R.epilogue_bwd(x.g, x.y, x.bias, x.gamma, x.phi, x.res, c.act, x.delta, x.zp, x.n_bits,
                           False)
    r = dict(r)
    r.update(pre_quant=pre_q, out=out)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return types.SimpleNamespace(**r)


def reference(c):
    """The oracle's outputs of a case (computed once, read-only)."""
    return _reference(case_id(c))


def coverage(c):
    """The figures check_coverage asserts, from the oracle alone."""
    ref = reference(c)
    t = ref.pre_quant
    s = {}
    blocked = np.zeros(t.shape, bool)
    if c.act:
        am = R._act_blocks(t, c.act)
        s["act_masked"] = float(am.mean())
        blocked |= am
    if c.q is not None:
        x = inputs(c)
        lo, hi = R.qrange(x.n_bits, False)
        with np.errstate(all="ignore"):
            xi = R.round_ste_fwd(t / x.delta) + x.zp
        s["clip_lo"], s["clip_hi"] = float((xi < lo).mean()), float((xi > hi).mean())
        s["in_range"] = float(((xi >= lo) & (xi <= hi)).mean())
        blocked |= ~((xi >= lo) & (xi <= hi))
    if (c.act or c.q is not None) and c.hw >= 8:
        rows = blocked.reshape(c.rows, c.hw)
        s["rows_mixed"] = bool(np.all(rows.any(axis=1) & ~rows.all(axis=1)))
        ch = blocked.transpose(1, 0, 2, 3).reshape(c.C, -1)
        s["chan_mixed"] = bool(np.all(ch.any(axis=1) & ~ch.all(axis=1)))
    return s


def check_coverage(c):
    s = coverage(c)
    if "act_masked" in s:
        assert 0.25 <= s["act_masked"] <= 0.75, (case_id(c), s)
    if "in_range" in s:
        assert s["in_range"] >= 0.5 and s["clip_hi"] >= 0.05, (case_id(c), s)
        if c.act == 0:
            assert s["clip_lo"] >= 0.05, (case_id(c), s)
    assert s.get("rows_mixed", True) and s.get("chan_mixed", True), (case_id(c), s)
    return s


def ulp32(v):
    v = np.abs(np.asarray(v, np.float64)).astype(F32)
    return np.spacing(np.maximum(v, np.finfo(F32).tiny)).astype(np.float64)


def sum_bound(S, A, n):
    """|got - S| allowed for a sum of n terms with oracle value S and absolute-term sum A
    (module docstring)."""
    return ulp32(S) + (n - 1) * 2.0 ** -53 * np.asarray(A, np.float64)


def reference_from_gradient(c, g):
    """The tail's oracle with the loss gradient g taken as given (p != 2: the device's K11
    gradient of the oracle's output)."""
    x = inputs(c)
    r = R.epilogue_loss_bwd(x.tcache[x.idx], c.p, x.M, x.y, x.bias, x.gamma, x.phi, x.res, c.act,
                            x.delta, x.zp, x.n_bits, False, x.res_epi, g=g)
    return types.SimpleNamespace(**r)


def sums_of(c):
    """(name, number of terms) of every sum the case's kernel returns."""
    if c.kind == "fwd":
        return []
    out = []
    if c.affine:
        out += [("ggamma", "n_chan"), ("gphi", "n_chan")]
    if c.q is not None:
        out += [("gdelta", "n_all"), ("gzp", "n_all")]
    if c.kind == "tail" and c.res == LAZY_AFFINE:
        out += [("gres_gamma", "n_chan"), ("gres_phi", "n_chan")]
    return out


BY_ID = {case_id(c): c for c in CASES + WORKER}
for _cases in (ENTRY_FWD, ENTRY_TAIL):
    for _k, _case in enumerate(_cases):
        _case.seed = ENTRY_SEEDS.get(case_id(_case), _case.seed)
        _cases[_k] = BY_ID.setdefault(case_id(_case), _case)     # (a case above: that one)
