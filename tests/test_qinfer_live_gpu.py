"""The single live rule of the carried routes (quant/integer.py, Edge.live, with
carry_head=True, so every kind of edge is installed): a condition that no longer holds at run
time costs time, never correctness.  One condition at a time is applied AFTER planning -- a
forward under torch.enable_grad(), act quantization switched off on one interior consumer and on
one block-edge reader, quant_layer._CONV_CACHE set, a no-op forward hook on an interior consumer,
on the stem's max-pool and on the head's average pool -- and the forward must give the logits of
the same model in the same state planned with no carry flag, bit for bit, with nothing off the
grid, the counter of every edge the condition touches standing still and every other counter
advancing.

An edge is touched by a module when the module is in the edge's own watched(): the modules its
live() inspects.  A head's pool and fc see codes only when its emitter edge emitted, so they are
touched by the emitter's watched() too.  Grad mode and a set _CONV_CACHE are looked at by every
emitter, and with no emitter no pool sees codes, so they touch everything."""
import numpy as np
import pytest
import torch

from test_qinfer_carry_model_gpu import host, restored

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


@pytest.fixture(scope="module")
def r18(Q):
    return restored(Q, "resnet18", 11, (8, 3, 64, 64))


def counters(Q, qnn):
    """Every edge counter of the installed plan, keyed (kind, module name)."""
    c = {("pair", n): v for n, v in Q.carry_report(qnn)["calls"].items()}
    c.update({("tail", n): v for n, v in Q.block_carry_report(qnn)["calls"].items()})
    s, h = Q.stem_carry_report(qnn), Q.head_carry_report(qnn)
    c.update({("stem", n): v for n, v in s["calls"].items()})
    c.update({("stem_pool", n): v for n, v in s["pooled"].items()})
    c.update({("head_emit", n): v for n, v in h["calls"].items()})
    c.update({("head_pool", n): v for n, v in h["pooled"].items()})
    c.update({("head_fc", n): v for n, v in h["fc"].items()})
    return c


def touched_by(Q, qnn, mod):
    """The counters of the edges whose watched() holds `mod`."""
    from shiftedscalequantization_amd.quant import integer as I
    names = {m: n for n, m in qnn.named_modules()}
    keys = set()
    for e in qnn._int_edges:
        mine = mod in e.watched()
        if isinstance(e, I.PairEdge) and mine:
            keys.add(("pair", names[e.at]))
        elif isinstance(e, I.TailEdge) and mine:
            keys.add(("tail", names[e.at]))
        elif isinstance(e, I.StemEdge) and mine:
            keys.add(("stem", names[e.at]))
            keys.update(("stem_pool", names[p]) for p in e.pools)
        elif isinstance(e, I.HeadEdge):
            emits = mod in e.emitter.watched()
            if emits:
                keys.add(("head_emit", names[e.producer]))
            if emits or mine:
                keys.update({("head_pool", names[e.at]), ("head_fc", names[e.fc])})
    return keys


def interior_consumer(Q, qnn):
    """The consumer of a carried pair in the middle of the model."""
    mods = dict(qnn.named_modules())
    pairs = Q.carry_report(qnn)["pairs"]
    return mods[pairs[len(pairs) // 2][1]]


def block_edge_reader(Q, qnn):
    """A reader of a block edge with no act quantizer of its own (a downsample conv), so that
    switching its act quantization off takes nothing off the grid."""
    mods = dict(qnn.named_modules())
    for blk, _ in Q.block_carry_report(qnn)["edges"]:
        for r in mods[blk]._int_tail.readers:       # the block's TailEdge
            if r.disable_act_quant:
                return r
    raise AssertionError("no block-edge reader without an act quantizer of its own")


class Condition:
    """pick(Q, qnn) -> the module the condition is applied to (None: the whole forward)."""

    def __init__(self, pick=None, grad=False, conv_cache=False, hook=False):
        self.pick, self.grad, self.conv_cache, self.hook = pick, grad, conv_cache, hook

    def forward(self, Q, qnn, x, monkeypatch):
        """(logits, the module) of one forward of the planned model under the condition."""
        from shiftedscalequantization_amd.quant import quant_layer
        mod = self.pick(Q, qnn) if self.pick else None
        with monkeypatch.context() as mp:
            if self.conv_cache:
                mp.setattr(quant_layer, "_CONV_CACHE", {})
            handle = None
            if self.hook:
                handle = mod.register_forward_hook(lambda m, args, out: None)
            elif mod is not None:
                mod.set_quant_state(True, False)
            try:
                with torch.enable_grad() if self.grad else torch.no_grad():
                    return qnn(x).detach().clone(), mod
            finally:
                if handle is not None:
                    handle.remove()
                elif mod is not None:
                    mod.set_quant_state(True, True)


CONDITIONS = {"enable_grad": Condition(grad=True),
              "interior_consumer_act_off": Condition(pick=interior_consumer),
              "block_edge_reader_act_off": Condition(pick=block_edge_reader),
              "conv_cache_set": Condition(conv_cache=True),
              "interior_consumer_hooked": Condition(pick=interior_consumer, hook=True),
              "stem_maxpool_hooked": Condition(pick=lambda Q, qnn: qnn.model.maxpool, hook=True),
              "head_avgpool_hooked": Condition(pick=lambda Q, qnn: qnn.model.avgpool, hook=True)}


@pytest.mark.parametrize("name", list(CONDITIONS))
def test_condition_costs_time_not_correctness(Q, r18, monkeypatch, name):
    qnn, x = r18
    cond = CONDITIONS[name]
    try:
        # the module is picked from the carried plan, the reference run on the uncarried one
        Q.enable_integer_inference(qnn, x, carry_head=True)
        picked = cond.pick(Q, qnn) if cond.pick else None
        Q.enable_integer_inference(qnn, x)
        assert counters(Q, qnn) == {}
        want, _ = Condition(pick=(lambda Q, q: picked) if picked is not None else None,
                            grad=cond.grad, conv_cache=cond.conv_cache,
                            hook=cond.hook).forward(Q, qnn, x, monkeypatch)
        assert Q.integer_report(qnn)["off_grid"] == 0

        Q.enable_integer_inference(qnn, x, carry_head=True)
        before = counters(Q, qnn)
        assert {k[0] for k in before} == {"pair", "tail", "stem", "stem_pool", "head_emit",
                                          "head_pool", "head_fc"}          # every kind of edge
        got, mod = cond.forward(Q, qnn, x, monkeypatch)
        assert mod is picked
        after = counters(Q, qnn)
        touched = set(before) if mod is None else touched_by(Q, qnn, mod)
        print(name, "touched:", sorted(touched))
        assert touched and touched <= set(before)
        assert Q.integer_report(qnn)["off_grid"] == 0
        assert np.array_equal(host(got).view(np.int32), host(want).view(np.int32))
        advanced = {k for k in before if after[k] > before[k]}
        assert advanced == set(before) - touched, (sorted(advanced), sorted(touched))
        # the condition gone, every edge carries again
        with torch.no_grad():
            qnn(x)
        again = counters(Q, qnn)
        assert all(again[k] > after[k] for k in before)
    finally:
        Q.disable_integer_inference(qnn)


def test_disable_leaves_no_edge_and_no_mark(Q, r18):
    """enable(carry_head=True) then disable: the registry is empty, the four carry reports are
    their empty forms and no module holds a mark."""
    qnn, x = r18
    Q.enable_integer_inference(qnn, x, carry_head=True)
    assert {type(e).__name__ for e in qnn._int_edges} == {"PairEdge", "TailEdge", "StemEdge", "HeadEdge"}
    Q.disable_integer_inference(qnn)
    assert qnn._int_edges == [] and qnn._int_counter is None
    assert Q.carry_report(qnn) == {"pairs": [], "calls": {}}
    assert Q.block_carry_report(qnn) == {"edges": [], "calls": {}, "residual": {}}
    assert Q.stem_carry_report(qnn) == {"edges": [], "calls": {}, "pooled": {}}
    assert Q.head_carry_report(qnn) == {"edges": [], "calls": {}, "pooled": {}, "fc": {}}
    marks = ("_int_plan", "_int_tail", "_int_stem", "_int_head")
    assert not [(n, a) for n, m in qnn.named_modules() for a in marks
                if getattr(m, a, None) is not None]
