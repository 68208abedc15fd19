"""kernels.conv_route against the routes recorded from the commit before it existed
(tests/conv_routes.json: what that commit's conv2d, Conv2dFn.forward and Conv2dFn.backward ran
for each case, with every executor replaced by a label), on stub tensors that carry only what
the rules read.  Nothing here needs a device; libssq.so's host-side planners are queried."""
import json
import os

import pytest
import torch

FWD = {"lib", "k18", "im2col_gemm", "grouped_gemm", "gemm_1x1", "epi_gemm"}
DX = {"lib", "k18", "gemm_1x1", None}
DW = {"lib", "k17", "im2col_gemm", "bmm_1x1", "bmm_s2", "grouped_gemm", None}


@pytest.fixture(scope="module")
def K():
    from shiftedscalequantization_amd import _capi, kernels
    try:
        _capi.load()
    except _capi.SSQError as e:
        pytest.skip(f"libssq.so is not built: {e}")
    return kernels


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(os.path.dirname(__file__), "conv_routes.json")) as fh:
        t = json.load(fh)
    tup = (lambda v: tuple(v) if isinstance(v, list) else v)
    t["shapes"] = [(tuple(xs), tuple(ws), tup(st), tup(pad), tup(dil), g)
                   for xs, ws, st, pad, dil, g in t["shapes"]]
    t["rows"] = [(si, fi, tuple(None if v == "-" else v for v in r.split("/")))
                 for si, fi, r in t["rows"]]
    return t


class Stub:
    """A tensor as far as the routing reads one."""
    is_cuda, dtype = True, torch.float32

    def __init__(self, shape, requires_grad=False, contiguous=True, lazy=False):
        self.shape, self.requires_grad, self._contiguous = torch.Size(shape), requires_grad, contiguous
        if lazy:
            self._ssq_epi = object()

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._contiguous


class flags:
    """A row's policy switches and cudnn.deterministic set for a block, restored after it."""
    NAMES = ("WGRAD_POLICY", "WGRAD_GEMM", "FWD_1X1_GEMM", "EPI_INTO_GEMM")

    def __init__(self, K, row_flags):
        self.K, self.f = K, row_flags

    def __enter__(self):
        self.old = [getattr(self.K, n) for n in self.NAMES] + [torch.backends.cudnn.deterministic]
        pol, wg, f1, det, _, _, _, _, _, epi = self.f
        self.K.WGRAD_POLICY, self.K.WGRAD_GEMM = pol, wg
        self.K.FWD_1X1_GEMM, self.K.EPI_INTO_GEMM = bool(f1), bool(epi)
        torch.backends.cudnn.deterministic = bool(det)

    def __exit__(self, *exc):
        for n, v in zip(self.NAMES, self.old):
            setattr(self.K, n, v)
        torch.backends.cudnn.deterministic = self.old[-1]


def stubs(shape, f):
    """(x, w, need_dx, need_dw) of a row: conv2d's own reading of the two requires_grad flags
    (a LazyEpi placeholder stands inside the graph being trained)."""
    xs, ws = shape[:2]
    _, _, _, _, xg, wg, ge, cont, lazy, _ = f
    return (Stub(xs, bool(xg), bool(cont), bool(lazy)), Stub(ws, bool(wg)),
            bool(ge and (xg or lazy)), bool(ge and wg))


def test_conv_route_returns_every_recorded_route(K, table):
    assert len(table["rows"]) > 3000
    bad = []
    for si, fi, want in table["rows"]:
        shape, f = table["shapes"][si], table["flags"][fi]
        x, w, need_dx, need_dw = stubs(shape, f)
        with flags(K, f):
            r = K.conv_route(x, w, *shape[2:], need_dx, need_dw)
        if (r.fwd, r.dx, r.dw) != want:
            bad.append((shape, f, want, (r.fwd, r.dx, r.dw)))
    assert not bad, (len(bad), bad[:10])


def test_table_names_every_route_value(table):
    """The table cannot hide a rule: every value of every field occurs, bmm_s2 only with the
    forward that made its operand, and every model / test / edge family is there."""
    routes = {r for _, _, r in table["rows"]}
    assert {r[0] for r in routes} == FWD
    assert {r[1] for r in routes} == DX
    assert {r[2] for r in routes} == DW
    assert all(r[0] == "gemm_1x1" for r in routes if r[2] == "bmm_s2")
    assert all(r[1:] in (("lib", "im2col_gemm"), (None, "im2col_gemm")) for r in routes if r[0] == "epi_gemm")
    cols = list(zip(*table["flags"]))
    assert set(cols[0]) == {"auto", "always", "never"} and set(cols[1]) == {"auto", "never"}
    for c in cols[2:]:
        assert set(c) == {0, 1}
    assert {tuple(f[4:7]) for f in table["flags"]} == {(1, 1, 1), (0, 1, 1), (1, 0, 1), (0, 0, 1), (1, 1, 0)}
    shapes = table["shapes"]
    assert any(isinstance(s[3], str) for s in shapes) and any(s[4] in (2, (2, 2)) for s in shapes)
    assert any(isinstance(s[2], tuple) and len(set(s[2])) == 2 for s in shapes)
    assert {s[0][0] for s in shapes} >= {32, 128}
    assert ((32, 3, 224, 224), (64, 3, 7, 7), (2, 2), (3, 3), (1, 1), 1) in shapes          # ResNet stem


def _plane(s):
    (_, _, H, W), (_, _, R, S), st, pad = s[0], s[1], s[2], s[3]
    return ((H + 2 * pad - R) // st + 1) * ((W + 2 * pad - S) // st + 1)


def _np(s):
    return s[0][0] * _plane(s)


# threshold pair -> (the quantity the rules compare, its value on the two sides)
PAIRS = {
    "plane_49_50": (_plane, 49, 50), "plane_99_100": (_plane, 99, 100),
    "plane_99_100_1x1": (_plane, 99, 100), "plane_100_101": (_plane, 100, 101),
    "plane_196_197": (_plane, 196, 197), "plane_196_197_grouped": (_plane, 196, 197),
    "plane_196_197_1x1": (_plane, 196, 197), "plane_195_196_dgrad": (_plane, 195, 196),
    "plane_399_400": (_plane, 399, 400), "plane_399_400_batch128": (_plane, 399, 400),
    "plane_783_784": (_plane, 783, 784), "plane_784_785": (_plane, 784, 785),
    "plane_12543_12544": (_plane, 12543, 12544),
    "co_127_128": (lambda s: s[1][0], 127, 128), "co_255_256": (lambda s: s[1][0], 255, 256),
    "crs_1151_1152": (lambda s: s[1][1] * s[1][2] * s[1][3], 1151, 1152),
    "co_below_c": (lambda s: s[1][0] - s[1][1], -1, 0),
    "co_below_2c": (lambda s: s[1][0] - 2 * s[1][1], -1, 0),
    "co_above_4c": (lambda s: s[1][0] - 4 * s[1][1], 0, 1),
    "c_multiple_of_64": (lambda s: s[1][1] % 64, 0, 32),
    "co_multiple_of_64": (lambda s: s[1][0] % 64, 0, 32),
    "batch_127_128": (lambda s: s[0][0], 127, 128),
    # the im2col operand (N*P x C*R*S) and the permuted gradient (Co x N*P) against 2^31
    "col_below_2_31": (lambda s: _np(s) * s[0][1] * 9 >= 1 << 31, False, True),
    "dy2_below_2_31": (lambda s: _np(s) * s[1][0] >= 1 << 31, False, True),
    "grouped_col_below_2_31": (lambda s: _np(s) * s[0][1] * 9 >= 1 << 31, False, True),
}


def test_threshold_pairs_sit_on_different_routes(table):
    """Each threshold the rules name has a shape on either side of it in the table, alike in
    everything else the rule reads, and under some flag setting the two take different routes."""
    assert set(table["threshold_pairs"]) == set(PAIRS)
    by_shape = {}
    for si, fi, r in table["rows"]:
        by_shape.setdefault(si, {})[fi] = r
    for name, (ia, ib) in table["threshold_pairs"].items():
        quantity, va, vb = PAIRS[name]
        a, b = table["shapes"][ia], table["shapes"][ib]
        assert (quantity(a), quantity(b)) == (va, vb), (name, a, b)
        assert a[2:] == b[2:] and a[1][2:] == b[1][2:] or name == "crs_1151_1152", (name, a, b)
        common = set(by_shape[ia]) & set(by_shape[ib])
        assert any(by_shape[ia][f] != by_shape[ib][f] for f in common), (name, a, b)


RULES = ("_use_fwd_1x1", "_use_fwd_gemm", "_use_dgrad_1x1", "_use_wgrad_bmm", "_use_wgrad_bmm_s2",
         "_use_wgrad_gemm", "_use_wgrad_grouped_gemm", "conv_wgrad_supported", "dwconv_supported",
         "wgrad_kind")
EXECUTORS = ("conv_fwd_gemm", "conv_fwd_grouped_gemm", "conv1x1_fwd_gemm", "dwconv_fwd",
             "epi_conv_gemm", "materialize_epi")


def test_one_conv2d_call_evaluates_each_rule_once(K, table, monkeypatch):
    """conv2d on one shape per recorded route (executors replaced, so nothing launches): no rule
    function and no planner query runs twice, and the decision is the table's."""
    counts = {}

    def counted(name, fn):
        def wrapper(*a, **k):
            counts[name] = counts.get(name, 0) + 1
            return fn(*a, **k)
        return wrapper

    for name in RULES:
        monkeypatch.setattr(K, name, counted(name, getattr(K, name)))
    query = K.query
    monkeypatch.setattr(K, "query", lambda fn, *a: counted(fn, query)(fn, *a))
    ran = []
    for name in EXECUTORS:
        monkeypatch.setattr(K, name, lambda x, *a, _n=name, **k: ran.append(_n) or x)
    monkeypatch.setattr(torch.nn.functional, "conv2d", lambda x, *a, **k: ran.append("lib") or x)
    monkeypatch.setattr(K.Conv2dFn, "apply", lambda x, w, st, pad, dil, g, route: ran.append(route))
    monkeypatch.setattr(K.DwConv2dFn, "apply", lambda x, *a: ran.append("DwConv2dFn"))
    seen = {}
    for si, fi, want in table["rows"]:
        seen.setdefault(want, (si, fi))
    assert len(seen) >= 29
    for want, (si, fi) in seen.items():
        shape, f = table["shapes"][si], table["flags"][fi]
        x, w, _, _ = stubs(shape, f)
        counts.clear()
        del ran[:]
        with flags(K, f), torch.set_grad_enabled(bool(f[6])):
            K.conv2d(x, w, *shape[2:])
        assert counts and max(counts.values()) == 1, (shape, f, counts)
        assert "_use_fwd_gemm" not in counts            # conv_route asks _use_wgrad_gemm itself
        trained = want[1] is not None or want[2] is not None
        if want[0] == "epi_gemm":
            assert ran == ["epi_conv_gemm"]
        elif want[0] == "k18":
            assert ran[-1] == ("DwConv2dFn" if trained else "dwconv_fwd")
        elif want[2] not in (None, "lib") or want[1] == "gemm_1x1":
            assert (ran[-1].fwd, ran[-1].dx, ran[-1].dw) == want        # Conv2dFn carries the route
        else:
            assert ran[-1] == {"lib": "lib", "gemm_1x1": "conv1x1_fwd_gemm"}[want[0]]
        assert (ran[0] == "materialize_epi") == (bool(f[8]) and want[0] != "epi_gemm")
