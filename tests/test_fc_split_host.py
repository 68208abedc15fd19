"""Host-side checks of the split fc iteration (ssq_fc_recon_grad / ssq_fc_recon_apply): the
symbols and their ctypes signatures, the SSQ_FC_SPLIT knob, and the argument validation,
which returns before any launch."""
import ctypes as C

import pytest


def test_split_symbols_load_with_declared_signatures():
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    p, i, i64, f, sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
    want = {
        "ssq_fc_recon_grad": [p, p, p, i64, p, p, p, p, p, i, i, p, i64, i64, p, p, p, p, sz, p],
        "ssq_fc_recon_apply": [p, p, p, p, p, i, i, i64, i64, p, i64, p, f, f, f, f, p, p, p],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
        assert _capi.SIGNATURES[name] == (C.c_int, args)


@pytest.mark.parametrize("value,mode", [("auto", "auto"), ("", "auto"), ("1", "on"), ("0", "off"),
                                        ("on", "on"), ("OFF", "off")])
def test_fc_split_knob_parses(value, mode):
    import importlib
    BR = importlib.import_module("shiftedscalequantization_amd.quant.block_recon")
    assert BR._fc_split_mode(value) == mode
    assert BR.FC_SPLIT in ("auto", "on", "off")


def test_fc_split_knob_refuses_other_values():
    import importlib
    BR = importlib.import_module("shiftedscalequantization_amd.quant.block_recon")
    with pytest.raises(ValueError):
        BR._fc_split_mode("2")


def test_fc_recon_apply_argument_errors_without_gpu():
    """C_in = 63 and a null gradient are refused on the host: a non-zero code and a message,
    no launch (the buffers here are host memory the library must not touch)."""
    from shiftedscalequantization_amd import _capi
    lib = _capi.load()
    bufs = [(C.c_float * 64)() for _ in range(8)]
    W, V, What, d, z, grad, m, v = (C.cast(b, C.c_void_p) for b in bufs)
    slot = C.cast((C.c_int64 * 8)(), C.c_void_p)

    def apply(Ci, grad_):
        return lib.ssq_fc_recon_apply(W, V, What, d, z, 0, 255, 1, Ci, slot, 4, grad_, 0.1, 0.999,
                                      0.001, 1e-8, m, v, None)

    assert apply(63, grad) == -1 and b"C_in" in lib.ssq_last_error()
    assert apply(64, None) == -1 and b"null" in lib.ssq_last_error()
    # ssq_fc_recon_grad: gv_out is required
    rc = lib.ssq_fc_recon_grad(W, V, slot, 4, W, V, What, d, z, 0, 255, None, 1, 64, grad, None,
                               m, v, 64, None)
    assert rc == -1 and b"gv_out" in lib.ssq_last_error()
