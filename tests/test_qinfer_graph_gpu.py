"""The integer forward as one replayed HIP graph (quant.IntegerGraph) and the planner's split-K
flag, on whole models.  A replay runs the kernels the eager forward runs on the same inputs, so
its logits are the eager ones bit for bit; the split-K form is bit-identical by the exactness of
the integer sum.  Also: the counters mean under replay what they mean eagerly, a second shape is
captured beside the first and a fifth evicts the oldest, the graph owns what it reads, a replay
under another plan and a construction without one or with a hook are refused, and
validate_model(graph=True) returns validate_model's accuracy."""
import numpy as np
import pytest
import torch

from test_qinfer_carry_model_gpu import host, restored

pytestmark = pytest.mark.gpu

ALL = dict(carry_head=True)                       # implies every carry flag below it


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import quant
    return quant


@pytest.fixture(scope="module")
def r18(Q):
    return restored(Q, "resnet18", 11, (8, 3, 64, 64))


def images(seed, n=8):
    return torch.randn(n, 3, 64, 64, generator=torch.Generator().manual_seed(seed)).cuda()


def eager(qnn, x):
    with torch.no_grad():
        return host(qnn(x)).view(np.int32).copy()


def bits(t):
    return host(t).view(np.int32).copy()


def check_replay(Q, qnn, x1, x2, **flags):
    """Replayed logits equal eager logits for x1, another x2 of the same shape, and x1 again."""
    try:
        Q.enable_integer_inference(qnn, x1, **flags)
        e1, e2 = eager(qnn, x1), eager(qnn, x2)
        assert not np.array_equal(e1, e2)
        g = Q.IntegerGraph(qnn)
        for x, want in ((x1, e1), (x2, e2), (x1, e1)):
            assert np.array_equal(bits(g(x)), want)
        assert g.shapes() == [tuple(x1.shape)]
        assert Q.integer_report(qnn)["off_grid"] == 0
    finally:
        Q.disable_integer_inference(qnn)


# ---------------------------------------------------------------- bit equality
def test_resnet18_replay_equals_eager(Q, r18):
    qnn, x = r18
    check_replay(Q, qnn, x, images(112), **ALL)


def test_mobilenetv2_grouped_replay_equals_eager(Q):
    qnn, _ = restored(Q, "mobilenetv2", 31, (2, 3, 64, 64))
    check_replay(Q, qnn, images(32, 2), images(33, 2), grouped=True, **ALL)


def test_regnetx600m_grouped_carry_blocks_replay_equals_eager(Q):
    qnn, x = restored(Q, "regnetx_600m", 41, (2, 3, 64, 64))
    check_replay(Q, qnn, x, images(142, 2), grouped=True, carry_blocks=True)


# ---------------------------------------------------------------- split-K in the planner
def test_resnet18_splitk_logits_equal_unsplit(Q, r18):
    qnn, x = r18
    try:
        Q.enable_integer_inference(qnn, x, **ALL)
        want = eager(qnn, x)
        assert Q.split_report(qnn) == {}
        Q.enable_integer_inference(qnn, x, splitk=True, **ALL)
        assert np.array_equal(eager(qnn, x), want)
        rep = Q.split_report(qnn)
        layer4 = [n for n in rep if "layer4" in n and "downsample" not in n]
        # the four 3x3 convs of layer4: at 64 x 64 their grid is 8 workgroups
        assert len(layer4) == 4 and all(rep[n] > 1 for n in layer4), rep
        assert all(z in (1, 2, 4, 8) for z in rep.values())
        g = Q.IntegerGraph(qnn)
        assert np.array_equal(bits(g(x)), want) and np.array_equal(bits(g(x)), want)
        assert Q.split_report(qnn) == rep
        assert Q.integer_report(qnn)["off_grid"] == 0
    finally:
        Q.disable_integer_inference(qnn)


# ---------------------------------------------------------------- counters
def reports(Q, qnn):
    return {"integer": Q.integer_report(qnn), "carry": Q.carry_report(qnn),
            "blocks": Q.block_carry_report(qnn), "stem": Q.stem_carry_report(qnn),
            "head": Q.head_carry_report(qnn)}


def counts(rep):
    """Every forward counter of the five reports, flat."""
    out = {}
    for r, d in rep.items():
        for key in ("calls", "pooled", "fc"):
            for name, v in d.get(key, {}).items():
                out[(r, key, name)] = v
    return out


def test_counters_mean_under_replay_what_they_mean_eagerly(Q, r18):
    from shiftedscalequantization_amd.quant.integer import _reset_calls
    qnn, x = r18
    x = x.clone()
    x[1, 2, 5, 7] = float("nan")
    try:
        Q.enable_integer_inference(qnn, r18[1], **ALL)
        _reset_calls(qnn)
        eager(qnn, x)
        one = reports(Q, qnn)
        c = one["integer"]["off_grid"]
        assert c > 0 and len(counts(one)) > 20 and max(counts(one).values()) == 1
        g = Q.IntegerGraph(qnn)
        _reset_calls(qnn)
        g(x)                                        # warm-up, capture and the first replay
        first = reports(Q, qnn)
        assert first["integer"]["off_grid"] == c and counts(first) == counts(one)
        _reset_calls(qnn)
        for _ in range(3):
            g(x)
        three = reports(Q, qnn)
        assert three["integer"]["off_grid"] == 3 * c
        assert counts(three) == {k: 3 * v for k, v in counts(one).items()}
        assert three["blocks"]["residual"] == one["blocks"]["residual"]
        for r in one:
            assert {k: v for k, v in three[r].items() if k in ("pairs", "edges")} == \
                {k: v for k, v in one[r].items() if k in ("pairs", "edges")}
    finally:
        Q.disable_integer_inference(qnn)


# ---------------------------------------------------------------- shapes
def test_a_second_shape_is_captured_and_a_fifth_evicts_the_oldest(Q, r18):
    qnn, x = r18
    try:
        Q.enable_integer_inference(qnn, x, **ALL)
        g = Q.IntegerGraph(qnn)
        want8 = eager(qnn, x)
        assert np.array_equal(bits(g(x)), want8)
        for n in (3, 2, 1):
            xn = images(50 + n, n)
            assert np.array_equal(bits(g(xn)), eager(qnn, xn)), n
        assert g.shapes() == [(n, 3, 64, 64) for n in (8, 3, 2, 1)]
        assert np.array_equal(bits(g(x)), want8)            # the oldest is now the 3-batch
        x4 = images(54, 4)
        assert np.array_equal(bits(g(x4)), eager(qnn, x4))
        assert g.shapes() == [(n, 3, 64, 64) for n in (2, 1, 8, 4)]
        x3 = images(53, 3)
        assert np.array_equal(bits(g(x3)), eager(qnn, x3))  # captured again
        assert g.shapes() == [(n, 3, 64, 64) for n in (1, 8, 4, 3)]
    finally:
        Q.disable_integer_inference(qnn)


# ---------------------------------------------------------------- ownership
def test_the_graph_owns_what_its_kernels_read(Q, r18):
    """After the capture every context is left, the allocator's cache is returned and junk is
    written over at least as much memory as that freed: the replay's bits do not move."""
    qnn, x = r18
    try:
        Q.enable_integer_inference(qnn, x, splitk=True, **ALL)
        want = eager(qnn, x)
        g = Q.IntegerGraph(qnn)
        assert np.array_equal(bits(g(x)), want)
        torch.cuda.synchronize()
        before = torch.cuda.memory_reserved()
        torch.cuda.empty_cache()
        freed = before - torch.cuda.memory_reserved()
        junk = [torch.full((max(freed, 1 << 26) // 4 + (1 << 20),), 0x5A, dtype=torch.uint8,
                           device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        assert sum(j.numel() for j in junk) >= freed
        x2 = images(61)
        assert np.array_equal(bits(g(x2)), eager(qnn, x2))
        assert np.array_equal(bits(g(x)), want)
        del junk
    finally:
        Q.disable_integer_inference(qnn)


# ---------------------------------------------------------------- staleness and refusal
def test_stale_and_refused_graphs(Q, r18):
    from shiftedscalequantization_amd._capi import SSQError
    qnn, x = r18
    Q.disable_integer_inference(qnn)
    with pytest.raises(ValueError, match="no integer plan"):
        Q.IntegerGraph(qnn)
    try:
        Q.enable_integer_inference(qnn, x, **ALL)
        g = Q.IntegerGraph(qnn)
        want = bits(g(x))
        Q.disable_integer_inference(qnn)
        with pytest.raises(SSQError, match="re-installed or removed"):
            g(x)
        Q.enable_integer_inference(qnn, x, **ALL)
        with pytest.raises(SSQError, match="re-installed or removed"):
            g(x)
        assert np.array_equal(bits(Q.IntegerGraph(qnn)(x)), want)
        name = "model.layer2.0.conv1"
        h = dict(qnn.named_modules())[name].register_forward_hook(lambda m, a, out: None)
        try:
            with pytest.raises(ValueError, match=name):
                Q.IntegerGraph(qnn)
        finally:
            h.remove()
        h = qnn.register_forward_pre_hook(lambda m, a: None)
        try:
            with pytest.raises(ValueError, match="hook"):
                Q.IntegerGraph(qnn)
        finally:
            h.remove()
    finally:
        Q.disable_integer_inference(qnn)


# ---------------------------------------------------------------- validate_model
def test_validate_model_graph_returns_the_same_accuracy(Q, r18):
    from shiftedscalequantization_amd.cli import validate_model
    qnn, x = r18
    try:
        Q.enable_integer_inference(qnn, x, **ALL)
        with torch.no_grad():
            target = qnn(x).argmax(1).cpu()
        target[::2] = (target[::2] + 1) % 1000              # half right, half wrong
        loader = [(x[:3].cpu(), target[:3]), (x[3:6].cpu(), target[3:6]), (x[6:].cpu(), target[6:])]
        plain = validate_model(loader, qnn)
        assert plain == 50.0
        assert validate_model(loader, qnn, graph=True) == plain
    finally:
        Q.disable_integer_inference(qnn)
