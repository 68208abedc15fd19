"""The integer weight operand as host arithmetic (quant/integer.py, weight_operand): which column
factors kcol[j], per-(co, ci) factors kfac, common denominator L and row scale d1 a layer's plan
prepares its int8 operand with, and the reason it is refused otherwise.  CPU tensors only; the
expected integers are numpy int64 arithmetic here, the expected reasons written out."""
import numpy as np
import pytest
import torch

from shiftedscalequantization_amd import kernels as K
from shiftedscalequantization_amd.quant import integer as I

OFF = I.PlanFlags()
PLAIN_ACT = K.ActQuant(0.05, 3.0, 4, False)
KIND = "channelquantmse"


def fields(Co, scale=None, per_ci=False, col_scale=None, kind="uniform"):
    scale = torch.linspace(0.01, 0.02, Co) if scale is None else scale
    return dict(zero_point=torch.full((Co,), 2.0), scale=scale, per_ci=per_ci, col_scale=col_scale,
                n_bits=2, qmin=0, qmax=3, kind=kind)


def shifted_act(La, ka, base=0.05):
    """The input grid of a hard shifted act quantizer: d[c] = fp32(base * fp32(k[c] / La))."""
    ka = torch.tensor(ka, dtype=torch.int32)
    d = torch.tensor(np.float32(base) * (ka.numpy().astype(np.float32) / np.float32(La)))
    return K.ActQuant(K.ChannelScale(d, base, (La, ka)), 3.0, 4, False)


def col(values, RS=1):
    """A column scale over j = (ci, r, s) from one value per ci."""
    return torch.tensor(values, dtype=torch.float32).repeat_interleave(RS)


def perci(base, k, L):
    """scale[co, ci] = fp32(base[co] * fp32(k[co, ci] / L))."""
    base, k = np.asarray(base, np.float32), np.asarray(k, np.float32)
    return torch.from_numpy(base[:, None] * (k / np.float32(L)))


def ints(t):
    return None if t is None else np.asarray(torch.as_tensor(t), dtype=np.int64).reshape(-1)


@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (3, 3, 3, 3), (2, 3)])
def test_a_plain_weight_and_an_all_ones_column_scale(shape):
    f = fields(shape[0])
    assert I.weight_operand(f, shape, 1, PLAIN_ACT, False, OFF) == (None, None, 1, f["scale"])
    J = int(np.prod(shape[1:]))
    f = fields(shape[0], col_scale=torch.ones(J), kind=KIND)
    kcol, kfac, L, d1 = I.weight_operand(f, shape, 1, PLAIN_ACT, False, OFF._replace(colscale=True))
    assert (kcol, kfac, L) == (None, None, 1) and d1 is f["scale"]


@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (3, 3, 3, 3), (2, 3)])
def test_a_column_scale_on_a_grid(shape):
    RS = int(np.prod(shape[2:]))
    f = fields(shape[0], col_scale=col([0.5, 1.0, 0.5], RS), kind=KIND)
    kcol, kfac, L, d1 = I.weight_operand(f, shape, 1, PLAIN_ACT, False, OFF._replace(colscale=True))
    assert kfac is None and L == 2 and d1 is f["scale"]
    assert np.array_equal(ints(kcol), np.repeat(np.array([1, 2, 1], np.int64), RS))
    assert I.weight_operand(f, shape, 1, PLAIN_ACT, False, OFF) == "weight has a column scale (channelquantmse)"


def test_an_off_grid_column_scale_names_the_limit_it_was_held_to():
    f = fields(2, col_scale=col([0.3337, 1.0, 0.5]), kind=KIND)
    on = OFF._replace(colscale=True)
    assert I.weight_operand(f, (2, 3, 1, 1), 1, PLAIN_ACT, False, on) == (
        "weight has a column scale (channelquantmse) that is not on an integer grid k / L, L <= 127")
    assert I.weight_operand(f, (2, 3, 1, 1), 1, PLAIN_ACT, False, on._replace(wide=True)) == (
        "weight has a column scale (channelquantmse) that is not on an integer grid k / L, L <= 1024")


def test_per_co_ci_scales():
    base = [0.01, 0.02]
    f = fields(2, scale=perci(base, [[31, 32, 33], [33, 33, 31]], 32), per_ci=True, kind="channelquant")
    assert I.weight_operand(f, (2, 3, 1, 1), 1, PLAIN_ACT, False, OFF) == (
        "weight scale is per (co, ci) (channelquant)")
    kcol, kfac, L, d1 = I.weight_operand(f, (2, 3, 1, 1), 1, PLAIN_ACT, False, OFF._replace(per_ci=True))
    # the grid's own contract: fp32(base[co] * fp32(k / L)) is the stored scale, bit for bit
    k = ints(kfac).reshape(2, 3).astype(np.float32)
    again = d1.numpy().astype(np.float32)[:, None] * (k / np.float32(L))
    assert kcol is None and np.array_equal(again.view(np.int32), f["scale"].numpy().view(np.int32))
    # every k = L: a plain weight with scale = base
    f = fields(2, scale=perci(base, [[32, 32, 32], [32, 32, 32]], 32), per_ci=True, kind="channelquant")
    kcol, kfac, L, d1 = I.weight_operand(f, (2, 3, 1, 1), 1, PLAIN_ACT, False, OFF._replace(per_ci=True))
    assert (kcol, kfac, L) == (None, None, 1)
    assert np.array_equal(d1.numpy().view(np.int32), np.asarray(base, np.float32).view(np.int32))
    # both scales
    f["col_scale"] = col([0.5, 1.0, 0.5])
    assert I.weight_operand(f, (2, 3, 1, 1), 1, PLAIN_ACT, False, OFF._replace(per_ci=True, colscale=True)) == (
        "weight has both a column scale and a per-(co, ci) scale (channelquant)")


def test_a_shifted_act_grid_is_folded_into_the_operand():
    ka, La = [3, 4, 5], 4
    act = shifted_act(La, ka)
    on = OFF._replace(colscale=True, per_ci=True, act_shift=True)
    # onto a plain 3 x 3 conv: kcol = k_a repeated per tap
    f = fields(3)
    kcol, kfac, L, d1 = I.weight_operand(f, (3, 3, 3, 3), 1, act, False, on)
    assert kfac is None and L == 4 and d1 is f["scale"]
    assert np.array_equal(ints(kcol), np.repeat(np.array(ka, np.int64), 9))
    # onto a column-scaled weight: the elementwise product, L_w * L_a
    f = fields(3, col_scale=col([0.5, 1.0, 0.5], 9), kind=KIND)
    kcol, kfac, L, _ = I.weight_operand(f, (3, 3, 3, 3), 1, act, False, on)
    want = np.repeat(np.array([1, 2, 1], np.int64), 9) * np.repeat(np.array(ka, np.int64), 9)
    assert kfac is None and L == 8 and np.array_equal(ints(kcol), want)
    # onto a per-(co, ci) weight: the product along ci, for every co
    f = fields(2, scale=perci([0.01, 0.02], [[31, 32, 33], [33, 33, 31]], 32), per_ci=True,
               kind="channelquant")
    _, k0, L0, _ = I.weight_operand(f, (2, 3, 1, 1), 1, PLAIN_ACT, False, on)
    kcol, kfac, L, _ = I.weight_operand(f, (2, 3, 1, 1), 1, act, False, on)
    want = ints(k0).reshape(2, 3) * np.array(ka, np.int64)[None, :]
    assert kcol is None and L == L0 * La and np.array_equal(ints(kfac).reshape(2, 3), want)
    # onto a 2-D fc weight: one factor per input feature
    kcol, _, L, _ = I.weight_operand(fields(2), (2, 3), 1, act, False, on)
    assert L == 4 and np.array_equal(ints(kcol), np.array(ka, np.int64))
    # L_a = 1 and every k_a = 1: stays plain
    f = fields(3)
    assert I.weight_operand(f, (3, 3, 3, 3), 1, shifted_act(1, [1, 1, 1]), False, on) == (
        None, None, 1, f["scale"])


def test_a_folded_grid_beyond_the_operands_limit():
    c = [126.0 / 127.0, 1.0, 125.0 / 127.0]
    f = fields(2, col_scale=col(c), kind=KIND)
    on = OFF._replace(colscale=True, act_shift=True)
    assert I.weight_operand(f, (2, 3, 1, 1), 1, PLAIN_ACT, False, on)[2] == 127
    assert I.weight_operand(f, (2, 3, 1, 1), 1, shifted_act(2, [1, 2, 3]), False, on) == (
        "shifted act grid folded into the weight's leaves the operand's grid (L = 254 > 127, or a "
        "factor above 16319)")
    assert I.weight_operand(f, (2, 3, 1, 1), 1, shifted_act(2, [1, 2, 3]), False,
                            on._replace(wide=True))[2] == 254


def test_a_shifted_grid_where_the_kernels_read_a_scalar_one():
    act, on = shifted_act(4, [3, 4, 5]), OFF._replace(act_shift=True, grouped=True)
    assert I.weight_operand(fields(3), (3, 1, 3, 3), 3, act, False, on) == (
        "input is a per-channel shifted act quantizer: the grouped and depthwise kernels "
        "(K25 / K26) read a scalar act grid")
    assert I.weight_operand(fields(2), (2, 3), 1, act, True, on) == (
        "input is a per-channel shifted act quantizer: the pooling head (K29 / K30) sums codes of "
        "one scalar grid")


def test_the_pooled_fc_takes_a_scaled_weight_only_with_wide_all():
    f = fields(2, col_scale=col([0.5, 1.0, 0.5]), kind=KIND)
    on = OFF._replace(colscale=True, wide=True)
    assert I.weight_operand(f, (2, 3), 1, PLAIN_ACT, True, on) == (
        "weight has a column scale (channelquantmse): the pooled-operand fc takes plain weights only")
    kcol, kfac, L, _ = I.weight_operand(f, (2, 3), 1, PLAIN_ACT, True, on._replace(wide_all=True))
    assert kfac is None and L == 2 and np.array_equal(ints(kcol), np.array([1, 2, 1], np.int64))
    # a plain weight is the pooled fc's own operand
    assert I.weight_operand(fields(2), (2, 3), 1, PLAIN_ACT, True, OFF)[:3] == (None, None, 1)
