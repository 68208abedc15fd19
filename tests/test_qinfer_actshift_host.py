"""K.actshift_grid's predicate and the act_shift flag's default.  No device."""
import inspect

import numpy as np
import pytest

F32 = np.float32


@pytest.mark.parametrize("targets,want", [([1.0, 0.5], (2, [2, 1])),
                                          ([1.0, 0.5, 0.75], (4, [4, 2, 3])),
                                          ([1.0], (1, [1])),
                                          ([1.0, 2 ** -0.5], None), ([1.0, 0.0], None)])
def test_actshift_grid(targets, want):
    from shiftedscalequantization_amd import kernels as K
    delta = F32(0.0371)
    got = K.actshift_grid(float(delta), targets)
    assert got == want
    if got is not None:
        L, k = got
        for s, ki in zip(targets, k):
            a, b = delta * (F32(ki) / F32(L)), delta * F32(s)
            assert 1 <= ki <= 127 and F32(a).view(np.int32) == F32(b).view(np.int32)


def test_flag_defaults_to_off():
    from shiftedscalequantization_amd import cli, quant as Q
    assert inspect.signature(Q.enable_integer_inference).parameters["act_shift"].default is False
    assert cli.build_parser().parse_args([]).int_infer_act_shift is False
