"""The prepared weight blobs (ssq_qweight_prepare, ..._colscale, ..._grouped, ..._grouped_colscale)
byte for byte against a numpy statement of the layouts, written from the layout comments of
csrc/qinfer.hip, csrc/qinfer_layout.h and csrc/qinfer_grouped.hip and not from the kernels:

  dense      int8 [Cop = 64*ceil(Co/64)][Kp = 64*ceil(R*S*Cp/64)], k = (r*S + s)*Cp + ci with
             Cp = 16*ceil(Ci/16); the 0/1 row [Kp]; cwz[Cop]; T[Cop] (int32)
  grouped    int8 [G*Cogp][Kp], Cogp = 16*ceil(Cog/16), Kp = 64*ceil(R*S*Wc/64),
             k = tap*Wc + (c - w0_g) in group g's window [w0_g, w0_g + Wc),
             w0_g = 16*floor(g*Cig/16), Wc = max_g(16*ceil((g+1)*Cig/16) - w0_g); the 0/1 rows
             [G][Kp]; cwz[Co]; T[Co] (int32)
  depthwise  int32 [R*S][Cp], wc = q - z_w[c]

Plain: a real element is q - (qmin + 128), cwz = qmin + 128 - z_w[co], T = sum + K*cwz.
Column-scaled: a real element is (q - z_w[co]) * k[j] saturated to +-127, cwz = 0, T = sum.
Everything else (padded channels and rows, the k tail, window channels outside the group) is 0.
A zero point that is no integer in [qmin - 256, qmin + 511] is taken as qmin and counted once
per channel; a saturated element and a k[j] outside [1, 127] (the element then 0) once each.

The whole blob is compared: every byte of every layout is written by the kernels (the blob is
filled with 0x5a before the call to show it).

Shapes: the smallest with channel padding, a k tail, a second channel tile and window offsets."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (Co, Ci, R, S), a Linear as (Co, Ci)
DENSE = [(1, 1, 1, 1), (65, 17, 3, 3), (5, 3, 1, 7), (10, 40)]
# (Co, Cig, R, S, groups)
GROUPED = [(9, 5, 3, 3, 3), (130, 20, 1, 1, 2), (8, 24, 3, 1, 2)]
DEPTHWISE = [(17, 1, 3, 3, 17), (16, 1, 1, 1, 16), (33, 1, 5, 5, 33)]
CONFIGS = [(b, s) for b in (2, 4, 8) for s in (False, True)]   # (n_bits, symmetric)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def rup(v, m):
    return (v + m - 1) // m * m


def pack(u, bits):
    """Codes u = q - qmin, element i at bit i * bits of the byte stream (low bits first); the
    stream holds whole groups of four elements (ssq_pack_bytes)."""
    per = 8 // bits
    flat = np.zeros(rup(u.size, 4), np.uint8)
    flat[:u.size] = u.reshape(-1)
    flat = flat.reshape(-1, per)
    return sum(flat[:, i] << (bits * i) for i in range(per)).astype(np.uint8)


def zero_points(zp, qmin):
    """(the integer each channel's zero point is taken as, the channels counted)."""
    ok = (zp == np.rint(zp)) & (zp >= qmin - 256) & (zp <= qmin + 511)
    return np.where(ok, zp, qmin).astype(np.int64), int((~ok).sum())


def operand(u, z, qmin, k):
    """The stored integer of every real element (Co, J...), and the elements counted.
    u: (Co, ...) codes q - qmin; z: (Co,) ints; k: None or ints broadcastable to u[0]."""
    zb = z.reshape((-1,) + (1,) * (u.ndim - 1))
    if k is None:
        return u - 128, 0
    kb = np.broadcast_to(k, u.shape[1:])[None]
    badk = (kb < 1) | (kb > 127)
    m = (u + qmin - zb) * np.where(badk, 0, kb)
    sat = np.abs(m) > 127
    return np.clip(m, -127, 127), int(np.broadcast_to(badk, u.shape).sum() + sat.sum())


def ref_dense(u, zp, qmin, k=None):
    Co, Ci, R, S = u.shape
    RS, Cp, Cop = R * S, rup(Ci, 16), rup(Co, 64)
    Kp = rup(RS * Cp, 64)
    z, bad = zero_points(zp, qmin)
    m, nb = operand(u, z, qmin, None if k is None else k.reshape(Ci, R, S))
    rows = np.zeros((Cop, Kp), np.int8)
    mask = np.zeros(Kp, np.int8)
    tile = np.zeros((Co, RS, Cp), np.int8)
    tile[:, :, :Ci] = m.transpose(0, 2, 3, 1).reshape(Co, RS, Ci)
    rows[:Co, :RS * Cp] = tile.reshape(Co, -1)
    one = np.zeros((RS, Cp), np.int8)
    one[:, :Ci] = 1
    mask[:RS * Cp] = one.reshape(-1)
    cwz = np.zeros(Cop, np.int32)
    tt = np.zeros(Cop, np.int32)
    if k is None:
        cwz[:Co] = qmin + 128 - z
    tt[:Co] = m.reshape(Co, -1).sum(1) + Ci * RS * cwz[:Co].astype(np.int64)
    return b"".join(a.tobytes() for a in (rows, mask, cwz, tt)), bad + nb


def ref_grouped(u, zp, qmin, groups, k=None):
    Co, Cig, R, S = u.shape
    RS, Cog = R * S, Co // groups
    Cogp = rup(Cog, 16)
    w0 = [g * Cig // 16 * 16 for g in range(groups)]
    Wc = max(rup((g + 1) * Cig, 16) - w0[g] for g in range(groups))
    Kp = rup(RS * Wc, 64)
    z, bad = zero_points(zp, qmin)
    m, nb = operand(u, z, qmin, None if k is None else k.reshape(Cig, R, S))
    rows = np.zeros((groups * Cogp, Kp), np.int8)
    masks = np.zeros((groups, Kp), np.int8)
    for g in range(groups):
        lo = g * Cig - w0[g]
        tile = np.zeros((Cog, RS, Wc), np.int8)
        tile[:, :, lo:lo + Cig] = m[g * Cog:(g + 1) * Cog].transpose(0, 2, 3, 1).reshape(Cog, RS, Cig)
        rows[g * Cogp:g * Cogp + Cog, :RS * Wc] = tile.reshape(Cog, -1)
        one = np.zeros((RS, Wc), np.int8)
        one[:, lo:lo + Cig] = 1
        masks[g, :RS * Wc] = one.reshape(-1)
    cwz = np.zeros(Co, np.int32) if k is not None else (qmin + 128 - z).astype(np.int32)
    tt = (m.reshape(Co, -1).sum(1) + Cig * RS * cwz.astype(np.int64)).astype(np.int32)
    return b"".join(a.tobytes() for a in (rows, masks, cwz, tt)), bad + nb


def ref_depthwise(u, zp, qmin, k=None):
    C, _, R, S = u.shape
    z, bad = zero_points(zp, qmin)
    if k is None:
        m, nb = u + qmin - z.reshape(-1, 1, 1, 1), 0
    else:
        m, nb = operand(u, z, qmin, k.reshape(1, R, S))
    wc = np.zeros((R * S, rup(C, 16)), np.int32)
    wc[:, :C] = m.reshape(C, R * S).T
    return wc.tobytes(), bad + nb


def reference(shape, groups, u, zp, qmin, k):
    if groups == 1:
        return ref_dense(u, zp, qmin, k)
    if shape[1] == 1 and shape[0] == groups:
        return ref_depthwise(u, zp, qmin, k)
    return ref_grouped(u, zp, qmin, groups, k)


def bad_zero_points(Co, qmin, sym):
    """{channel: value} sets: one non-integer and one outside the band (Co = 1: one each)."""
    frac, out = qmin + 1.5, float(qmin - 257 if sym else qmin + 512)
    return [{0: frac, Co - 1: out}] if Co > 1 else [{0: frac}, {0: out}]


def case_inputs(rng, shape4, n_bits, sym, colscale, zbad):
    """Codes, zero points and (colscale) factors k with 1, 127 and values in between, every real
    product inside +-127 but one, which exceeds it."""
    Co, Cj, R, S = shape4
    J = Cj * R * S
    qmin = -(1 << (n_bits - 1)) if sym else 0
    nq = 1 << n_bits
    if not colscale:
        u = rng.integers(0, nq, size=shape4)
        zp = rng.integers(qmin - 3, qmin + nq + 3, size=Co).astype(np.float32)
        if Co > 3:
            zp[1], zp[2] = qmin - 256, qmin + 511      # the band's own edges are accepted
        for c, v in zbad.items():
            zp[c] = v
        return u, zp, qmin, None
    k = rng.integers(2, 127, size=J)
    k[0] = 127
    if J > 1:
        k[J - 1] = 1
    zi = rng.integers(qmin, qmin + nq, size=Co)
    zp = zi.astype(np.float32)
    for c, v in zbad.items():
        zp[c], zi[c] = v, qmin
    cmax = 127 // k.reshape(1, J)
    lo = np.maximum(-cmax, (qmin - zi).reshape(Co, 1))
    hi = np.minimum(cmax, (qmin + nq - 1 - zi).reshape(Co, 1))
    c = rng.integers(lo, hi + 1)
    co = Co // 2
    c[co, 0] = 2 if qmin + nq - 1 - zi[co] >= 2 else -2       # times k[0] = 127: saturates
    u = (c + zi.reshape(Co, 1) - qmin).reshape(shape4)
    assert u.min() >= 0 and u.max() < nq
    return u, zp, qmin, k


def run_wrapper(K, shape, groups, u, zp, qmin, n_bits, k):
    packed = torch.from_numpy(pack(u, n_bits)).cuda()
    prep = K.qweight_prepare(packed, shape, torch.from_numpy(zp).cuda(), n_bits, qmin, groups=groups,
                             kcol=None if k is None else torch.from_numpy(k.astype(np.int32)))
    assert prep.centred == (k is not None)
    return prep.blob.cpu().numpy().tobytes(), int(prep.bad.item())


def run_raw(K, shape4, groups, u, zp, qmin, n_bits, k):
    """The entry point itself on a blob filled with 0x5a: a byte no kernel writes shows."""
    Co, Cj, R, S = shape4
    packed = torch.from_numpy(pack(u, n_bits)).cuda()
    zt = torch.from_numpy(zp).cuda()
    kt = None if k is None else torch.from_numpy(k.astype(np.int32)).cuda()
    nbytes = (K.query("ssq_qweight_prepared_bytes_grouped", Co, Cj, R, S, groups) if groups > 1
              else K.query("ssq_qweight_prepared_bytes", Co, Cj, R, S))
    blob = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    name = "ssq_qweight_prepare" + ("_grouped" if groups > 1 else "") + ("" if k is None else "_colscale")
    args = [K._vp(packed), K._vp(zt)] + ([] if k is None else [K._vp(kt)]) + [Co, Cj, R, S]
    args += ([groups] if groups > 1 else []) + [n_bits, qmin, K._vp(blob), K._vp(bad), K.stream_of(blob)]
    K.call(name, *args)
    return blob.cpu().numpy().tobytes(), int(bad.item())


def check(got, want, what):
    (gb, gbad), (wb, wbad) = got, want
    assert len(gb) == len(wb), f"{what}: blob of {len(gb)} bytes, layout says {len(wb)}"
    if gb != wb:
        g, w = np.frombuffer(gb, np.uint8), np.frombuffer(wb, np.uint8)
        i = int(np.flatnonzero(g != w)[0])
        raise AssertionError(f"{what}: {int((g != w).sum())} bytes differ, first at {i}: "
                             f"{g[i]} != {w[i]}")
    assert gbad == wbad, f"{what}: bad = {gbad}, expected {wbad}"


ALL = [(s, 1) for s in DENSE] + [(s[:4], s[4]) for s in GROUPED + DEPTHWISE]


@pytest.mark.parametrize("colscale", [False, True], ids=["plain", "colscale"])
@pytest.mark.parametrize("shape,groups", ALL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"g{v}")
def test_prepared_blob_bytes(K, shape, groups, colscale):
    shape4 = tuple(shape) + (1, 1) * (len(shape) == 2)
    rng = np.random.default_rng(1000 * len(ALL) + 7 * shape4[0] + groups + colscale)
    for n_bits, sym in CONFIGS:
        qmin = -(1 << (n_bits - 1)) if sym else 0
        for zbad in [{}] + bad_zero_points(shape4[0], qmin, sym):
            u, zp, qmin, k = case_inputs(rng, shape4, n_bits, sym, colscale, zbad)
            want = reference(shape4, groups, u, zp, qmin, k)
            assert want[1] == len(zbad) + (1 if colscale else 0)     # what the case was built to count
            what = f"{shape} g{groups} W{n_bits}{'s' if sym else 'u'} zbad={zbad}"
            check(run_wrapper(K, shape, groups, u, zp, qmin, n_bits, k), want, what)
            check(run_raw(K, shape4, groups, u, zp, qmin, n_bits, k), want, what + " (raw)")


@pytest.mark.parametrize("shape,groups", [((5, 3, 1, 7), 1), ((9, 5, 3, 3), 3), ((17, 1, 3, 3), 17)],
                         ids=["dense", "grouped", "depthwise"])
def test_column_factor_out_of_range(K, shape, groups):
    """k[j] of 0 and of 128, which qweight_prepare refuses before the call: every real element
    of those columns is stored as 0 and counted once."""
    rng = np.random.default_rng(77 + groups)
    u, zp, qmin, k = case_inputs(rng, shape, 4, False, True, {})
    k[1], k[2] = 0, 128
    want = reference(shape, groups, u, zp, qmin, k)
    per_column = shape[0]                      # a column has one real element per output channel
    assert want[1] == 1 + 2 * per_column
    check(run_raw(K, shape, groups, u, zp, qmin, 4, k), want, f"{shape} g{groups}")
    with pytest.raises(Exception, match="kcol must lie"):
        run_wrapper(K, shape, groups, u, zp, qmin, 4, k)
