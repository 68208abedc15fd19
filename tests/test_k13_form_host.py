"""Which K13 wrapper runs for which inputs, against the table recorded from the commit before
kernels.k13 existed (tests/k13_forms.json).

How the table was recorded: this file's own enumeration (`python tests/test_k13_form_host.py
--record tests/k13_forms.json`) was run on that commit, where the choice was still written out in
QuantModule.forward, BaseQuantBlock._tail and the two placeholder classes.  K.epilogue,
K.bias_act_quant, K.bias_act, K.materialize and K.lazy_epilogue are replaced by spies that note
their name, lazy or not, which of bias / gamma / residual / act quantizer they were handed and the
activation code; forward_raw returns a stub tensor; the act quantizers, the block activation, the
eager last(inp) and the eager residual add are spies too, so a row is the whole sequence of ops
the site ran.  The third site calls the real K.bias_act / K.epilogue with lazy=True on host
tensors (the autograd Functions replaced, so nothing launches) and notes whether the placeholder
came back and what it carries.  Every site is enumerated as the full product of its dimensions,
and the recorder refuses a table in which a wrapper or a dimension's value is missing -- the same
conditions test_table_names_every_form asserts.  Nothing here needs a device or libssq.so."""
import contextlib
import itertools
import json
import os
import re
import sys
import types

import torch
import torch.nn as nn

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "k13_forms.json")

DIMS = {
    "module": [("bias", (0, 1)), ("affine", (0, 1)), ("act", (0, 1, 2)),
               ("act_quant", ("off", "fusable", "per_channel", "disabled")),
               ("nonaffine_q", (0, 1)), ("consumer", (0, 1)), ("hooks", (0, 1))],
    "tail": [("gamma", (0, 1)), ("last_act", (0, 1)), ("last_act_quant", (0, 1)),
             ("block_act", (0, 1, 2)), ("block_act_quant", ("off", "fusable", "per_channel")),
             ("residual", ("none", "tensor", "lazy")), ("tail_lazy", (0, 1)), ("hooks", (0, 1))],
    "lazy": [("fn", ("bias_act", "epilogue")), ("act", (0, 1, 2)),
             ("strided", ("none", "y", "res")), ("hw_mod_4", (0, 1)),
             ("misaligned", ("none", "y", "res")), ("tail_scalar", (0, 1)),
             ("residual", ("none", "tensor", "lazy"))],
}
WRAPPERS = ("epilogue", "bias_act_quant", "bias_act", "materialize", "lazy_epilogue")
CALL = re.compile(r"(\w+)\(b(.),g(.),r(.),q(.),a(.),L(.)\)")


class Stub:
    """A device tensor as far as the form rules read one."""
    is_cuda, dtype, requires_grad, shape = True, torch.float32, False, torch.Size((2, 4, 8, 8))

    def __init__(self, log=None):
        self.log = log

    def dim(self):
        return 4

    def numel(self):
        return 512

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return 0

    def __add__(self, other):
        self.log.append("add")
        return Stub(self.log)


class Scalars:
    """An act quantizer's delta / zero point on the device: n values."""
    is_cuda = True

    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


@contextlib.contextmanager
def patched(pairs):
    old = [(o, n, getattr(o, n)) for o, n, _ in pairs]
    try:
        for o, n, v in pairs:
            setattr(o, n, v)
        yield
    finally:
        for o, n, v in old:
            setattr(o, n, v)


def _mods():
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd.quant import quant_block as QB
    from shiftedscalequantization_amd.quant import quant_layer as QL
    return K, QL, QB


def spies(K, log):
    """The five wrappers as labelled spies."""
    def kind(res):
        return "-" if res is None else ("z" if isinstance(res, K.LazyRes) else "t")

    def note(name, bias, gamma, res, q, relu, lazy):
        log.append("%s(b%d,g%d,r%s,q%d,a%d,L%d)" % (name, bias is not None, gamma is not None,
                                                  kind(res), q is not None, int(relu), bool(lazy)))
        return Stub(log)

    def epilogue(y, bias, gamma, phi, res, relu, q=None, lazy=False):
        assert (gamma is None) == (phi is None)
        return note("epilogue", bias, gamma, res, q, relu, lazy)

    def bias_act_quant(y, bias, res, relu, delta, zp, n_bits, sym=False):
        assert delta is not None and zp is not None
        return note("bias_act_quant", bias, None, res, delta, relu, False)

    def bias_act(y, bias=None, res=None, relu=True, lazy=False):
        return note("bias_act", bias, None, res, None, relu, lazy)

    def materialize(res):
        log.append("materialize(r%s)" % kind(res))
        return Stub(log) if isinstance(res, K.LazyRes) else res

    def lazy_epilogue(y, bias, gamma, phi, relu, q):
        return note("lazy_epilogue", bias, gamma, None, q, relu, False)

    return [(K, f.__name__, f) for f in (epilogue, bias_act_quant, bias_act, materialize,
                                         lazy_epilogue)]


def _spy_forward(mod, log, label):
    mod.forward = lambda *a: log.append(label) or Stub(log)


def _act(code):
    from shiftedscalequantization_amd.quant.quant_layer import StraightThrough
    return (StraightThrough, nn.ReLU, nn.ReLU6)[code]()


def _set_quantizer(q, mode, log, label):
    """off / disabled: left as built; fusable: initialised, one delta; per_channel: four."""
    _spy_forward(q, log, label)
    if mode in ("fusable", "per_channel"):
        for name in ("delta", "zero_point"):
            if name in q._parameters:
                delattr(q, name)
            setattr(q, name, Scalars(1 if mode == "fusable" else 4))
        q.inited = True


def _qmodule(QL, log, bias, affine, act, disable):
    m = QL.QuantModule(nn.Conv2d(4, 4, 1, bias=bool(bias)), {}, {}, disable_act_quant=disable)
    m.use_weight_quant = True
    if affine:
        with torch.no_grad():
            m.alpha_out.fill_(1.5)
    m.activation_function = _act(act)
    m.forward_raw = lambda inp: (Stub(log), m.bias)
    return m


def module_site(bias, affine, act, act_quant, nonaffine_q, consumer, hooks):
    K, QL, _ = _mods()
    log = []
    m = _qmodule(QL, log, bias, affine, act, act_quant == "disabled")
    m.use_act_quant = act_quant != "off"
    _set_quantizer(m.act_quantizer, act_quant, log, "act_quantizer")
    if hooks:
        m.register_forward_hook(lambda mod, i, o: None)
    with patched(spies(K, log) + [(QL, "EPI_NONAFFINE_Q", bool(nonaffine_q))]):
        prev = K.EPI_CONSUMER[0]
        K.EPI_CONSUMER[0] = object() if consumer else None
        try:
            m(Stub(log))
        finally:
            K.EPI_CONSUMER[0] = prev
    return " ".join(log)


def tail_site(gamma, last_act, last_act_quant, block_act, block_act_quant, residual, tail_lazy,
              hooks):
    K, QL, QB = _mods()
    log = []
    last = _qmodule(QL, log, 1, gamma, last_act, False)
    last.use_act_quant, last.disable_act_quant = True, not last_act_quant
    last.forward = lambda inp: log.append("last()") or Stub(log)
    blk = QB.BaseQuantBlock({})
    blk.activation_function = _act(block_act)
    _spy_forward(blk.activation_function, log, "act")
    blk.use_act_quant = block_act_quant != "off"
    _set_quantizer(blk.act_quantizer, block_act_quant, log, "act_quantizer")
    if hooks:
        blk.register_forward_hook(lambda mod, i, o: None)
    res = {"none": None, "tensor": Stub(log),
           "lazy": K.LazyRes(Stub(log), Scalars(4), None, None)}[residual]
    with patched(spies(K, log)):
        prev = K.TAIL_LAZY[0]
        K.TAIL_LAZY[0] = blk if tail_lazy else None
        try:
            blk._tail(last, Stub(log), res)
        finally:
            K.TAIL_LAZY[0] = prev
    return " ".join(log)


def _host_tensor(hw_mod_4, strided, misaligned):
    s = 3 if hw_mod_4 else 4
    buf = torch.zeros(2 * 3 * s * s + 8)
    off = (-(buf.data_ptr() // 4)) % 4 + (1 if misaligned else 0)
    t = buf[off:off + 2 * 3 * s * s].view(2, 3, s, s)
    assert (t.data_ptr() % 16 != 0) == bool(misaligned)
    return t.transpose(2, 3) if strided else t


def lazy_site(fn, act, strided, hw_mod_4, misaligned, tail_scalar, residual):
    K, _, _ = _mods()
    y = _host_tensor(hw_mod_4, strided == "y", misaligned == "y")
    r = _host_tensor(hw_mod_4, strided == "res", misaligned == "res")
    res = {"none": None, "tensor": r, "lazy": K.LazyRes(r, None, None, None)}[residual]
    bias, gamma, phi = torch.zeros(3), torch.ones(3), torch.zeros(3)
    q = types.SimpleNamespace(delta=torch.ones(1), zero_point=torch.zeros(1), n_bits=4, sym=False)
    eager = staticmethod(lambda *a: torch.zeros(1))
    with patched([(K, "TAIL_SCALAR", bool(tail_scalar)), (K.BiasActFn, "apply", eager),
                  (K.EpilogueFn, "apply", eager)]):
        if fn == "bias_act":
            out = K.bias_act(y, bias, res, act, lazy=True)
            want = (y, bias, None, None, res, act, None)
        else:
            out = K.epilogue(y, bias, gamma, phi, res, act, q, lazy=True)
            want = (y, bias, gamma, phi, res, act, q)
    tail = getattr(out, "_ssq_tail", None)
    if tail is None:
        return "eager"
    assert out.shape == y.shape and all(a is b or a == b for a, b in zip(tuple(tail), want))
    return "placeholder"


SITES = {"module": module_site, "tail": tail_site, "lazy": lazy_site}


def cases(site):
    return itertools.product(*(values for _, values in DIMS[site]))


def check_table(t):
    """The table cannot hide a rule: every site is the full product of its dimensions, every
    dimension takes every value, and every wrapper -- lazy and not, every residual kind, every
    activation code, the placeholder made and refused -- occurs."""
    labels = t["labels"]
    for site, dims in DIMS.items():
        assert [[n, list(v)] for n, v in dims] == t[site]["dims"], site
        n = 1
        for _, v in dims:
            n *= len(v)
        assert len(t[site]["rows"]) == n, site
        assert all(0 <= r < len(labels) for r in t[site]["rows"])
    ops = {op for s in ("module", "tail") for r in t[s]["rows"] for op in labels[r].split(" ")}
    calls = [m.groups() for m in map(CALL.fullmatch, ops) if m]
    assert {c[0] for c in calls} == set(WRAPPERS) - {"materialize"}
    assert {"materialize(r-)", "materialize(rt)", "materialize(rz)"} <= ops
    assert {"act_quantizer", "act", "last()", "add"} <= ops
    for w in ("epilogue", "bias_act"):
        mine = [c for c in calls if c[0] == w]
        assert {c[6] for c in mine} == {"0", "1"}, w                    # lazy and not
        assert {c[3] for c in mine} == {"-", "t", "z"}, w               # every residual kind
        assert {c[5] for c in mine} == {"0", "1", "2"}, w               # every activation code
        assert {c[1] for c in mine} == {"0", "1"}, w                    # bias or none
    assert {(c[2], c[4]) for c in calls if c[0] == "epilogue"} == {("1", "0"), ("1", "1"), ("0", "1")}
    assert {c[5] for c in calls if c[0] == "bias_act_quant"} == {"0", "1", "2"}
    assert {(c[2], c[4]) for c in calls if c[0] == "lazy_epilogue"} == \
        {("0", "0"), ("1", "0"), ("1", "1")}
    assert {labels[r] for r in t["lazy"]["rows"]} == {"eager", "placeholder"}


def record(path):
    labels, t = [], {}
    for site, fn in SITES.items():
        rows = []
        for c in cases(site):
            label = fn(*c)
            if label not in labels:
                labels.append(label)
            rows.append(labels.index(label))
        t[site] = {"dims": [[n, list(v)] for n, v in DIMS[site]], "rows": rows}
    t["labels"] = labels
    check_table(t)
    with open(path, "w") as fh:
        json.dump(t, fh, separators=(",", ":"))
        fh.write("\n")
    print(len(labels), "labels;", {s: len(t[s]["rows"]) for s in SITES})


def _table():
    with open(TABLE) as fh:
        return json.load(fh)


def test_every_site_runs_the_recorded_form():
    t = _table()
    bad = []
    for site, fn in SITES.items():
        for c, r in zip(cases(site), t[site]["rows"]):
            got = fn(*c)
            if got != t["labels"][r]:
                bad.append((site, c, t["labels"][r], got))
    assert not bad, (len(bad), bad[:10])


def test_table_names_every_form():
    check_table(_table())



def test_byte_ledger_counts_a_rows_launch_as_its_plain_twin():
    """tools/ssq_bytes.py prices a call from its ABI arguments: the wrappers now launch the
    _rows entries where they launched ssq_bias_act / ssq_bias_act_fq / the plain epilogue
    entries, and an iteration's ledger must not move -- same bytes for the same operands."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "ssq_bytes", os.path.join(os.path.dirname(TABLE), os.pardir, "tools", "ssq_bytes.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    P, n, N, C_, hw = object(), 2 * 3 * 16, 2, 3, 16
    for res, out, yq in itertools.product((None, P), repeat=3):
        rows = B.bytes_of("ssq_epilogue_fwd_rows", (P, None, P, None, None, res, None, out, yq, n,
                                                    hw, C_, 1, None, None, 0, 1, None, None, 0, P))
        assert rows == B.bytes_of("ssq_epilogue_fwd", (P, P, None, None, res, out, yq, n, hw, C_, 1,
                                                       None, None, 0, 1, P))
        assert rows == B.bytes_of("ssq_bias_act_fq", (P, P, res, out, yq, n, hw, C_, 1, P, P, 0, 15, P))
        if out is not None and yq is None:
            assert rows == B.bytes_of("ssq_bias_act", (P, P, res, out, n, hw, C_, 1, P))
    for res, gy, gres in itertools.product((None, P), repeat=3):
        tail = (N, C_, hw, 1, None, None, 0, 1, gy, gres, None, None, None, None, P, 0, P)
        assert B.bytes_of("ssq_epilogue_bwd_rows", (P, P, None, P, None, None, res, None) + tail) == \
            B.bytes_of("ssq_epilogue_bwd", (P, P, P, None, None, res) + tail)
        tail = (None, None, None, N, C_, hw, 1, None, None, 0, 1, gy, gres) + (None,) * 6 + (P, 0, P)
        head = (P, P, 96, 2.0, P, P)
        assert B.bytes_of("ssq_epilogue_loss_bwd_rows", head + (None, P, None, None, res, None) + tail) == \
            B.bytes_of("ssq_epilogue_loss_bwd", head + (P, None, None, res) + tail)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert sys.argv[1] == "--record"
    record(sys.argv[2])
