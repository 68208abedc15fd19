"""The K13 epilogue cases of tests/epilogue_cases.py on the device, against the fp64 oracle.

check_case(K, c) runs one case through the public wrappers (K.bias_act, K.bias_act_quant,
K.epilogue, K.epilogue(..., lazy=True) + K.epilogue_loss_bwd, K.LazyRes), asserts it and
returns its parity record; tests/test_epilogue_oracle_gpu.py calls it for every case.

As a program it is one child of that test's non-default-forms function: the A/B knobs
(SSQ_EPI_G16, SSQ_EPI_MULTI_ROW, SSQ_K13_PLANE4) are read once per process, so each
environment gets a fresh process, which checks through the form queries that the knob took
effect and then applies the same assertions to the reduced list EC.WORKER.

    python tests/epilogue_worker.py {g16_0|g16_0_multi_2|g16_0_multi_0|plane4_0}
"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import epilogue_cases as EC  # noqa: E402

F32 = np.float32


def dev(a, mis=False):
    """The array on the device; mis: 4 bytes into its (16-B aligned) buffer."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    if not mis:
        return t.cuda()
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def host(t):
    return None if t is None else t.detach().float().cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(a, F32).reshape(-1).view(np.int32)


def assert_bits(got, ref, what, nan_in=None):
    """Bit for bit, a NaN that propagates from a NaN input (nan_in: where the input is NaN)
    included: its sign and payload are the input's on both sides.  A NaN made by an invalid
    operation (inf - inf, 0 * inf) has no defined sign -- the host's default NaN is negative,
    the device's positive -- so there only the position is compared."""
    got, ref = np.asarray(got, F32).reshape(-1), np.asarray(ref, F32).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions differ")
    cmp = ~nan if nan_in is None else ~(nan & ~np.asarray(nan_in).reshape(-1))
    bad = np.flatnonzero(bits(got)[cmp] != bits(ref)[cmp])
    assert bad.size == 0, (what, f"{bad.size} of {got.size} differ", got[cmp][bad[:4]], ref[cmp][bad[:4]])


def chan(a):
    return None if a is None else dev(a.reshape(1, -1, 1, 1))


def quantizer(x, grad=True):
    if x.delta is None:
        return None
    return types.SimpleNamespace(delta=dev(np.array(x.delta, F32)).requires_grad_(grad),
                                 zero_point=dev(np.array(x.zp, F32)).requires_grad_(grad),
                                 n_bits=x.n_bits, sym=False)


def operands(K, c, x, grad=True):
    """y, bias, gamma, phi, res (a tensor or a K.LazyRes), q of the case on the device (inside
    a K.row_views() context: view cases register y and res as views of their caches)."""
    o = types.SimpleNamespace()
    idx = dev(x.idx)
    if c.view:
        o.y = K.rows_view(torch.empty(c.shape, device="cuda"), dev(x.ycache), idx)
    else:
        o.y = dev(x.y, c.mis)
    o.y.requires_grad_(grad and c.need_dy)
    o.rraw = None
    if x.res is not None:
        if c.view:
            o.rraw = K.rows_view(torch.empty(c.shape, device="cuda"), dev(x.rcache), idx)
        else:
            o.rraw = dev(x.res)
        o.rraw.requires_grad_(grad and c.want_gres)
    o.bias = dev(x.bias)
    o.gamma, o.phi = chan(x.gamma), chan(x.phi)
    o.rgamma, o.rphi = chan(x.rgamma), chan(x.rphi)
    for t in (o.gamma, o.phi, o.rgamma, o.rphi):
        if t is not None:
            t.requires_grad_(grad)
    o.res = o.rraw
    if x.res_epi is not None:
        o.res = K.LazyRes(o.rraw, dev(x.rbias), o.rgamma, o.rphi)
    o.q = quantizer(x, grad)
    return o


def run_fwd_only(K, c, x):
    """Forward outputs through every public wrapper that takes the case."""
    got = {}
    with torch.no_grad(), K.row_views():
        o = operands(K, c, x, grad=False)
        got["out"] = host(K.epilogue(o.y, o.bias, o.gamma, o.phi, o.res, c.act, o.q))
        if o.q is not None:
            # the same pass without its quantizer: the pre-quant activation, whose last bits a
            # coarse quantizer would hide
            got["pre_quant"] = host(K.epilogue(o.y, o.bias, o.gamma, o.phi, o.res, c.act, None))
    if not c.affine and not c.view:
        with K.row_views():
            o = operands(K, c, x, grad=False)
            if o.q is None:
                with torch.no_grad():
                    got["out_bias_act"] = host(K.bias_act(o.y, o.bias, o.res, c.act))
            else:
                # with a gradient wanted the pass keeps the pre-quant activation for its backward
                o.y.requires_grad_(True)
                yq = K.bias_act_quant(o.y, o.bias, o.res, c.act, o.q.delta, o.q.zero_point, x.n_bits)
                got["out_bias_act"] = host(yq)
                got["pre_quant_kept"] = host(yq.grad_fn.saved_tensors[0])
                with torch.no_grad():
                    got["out_nokeep"] = host(K.bias_act_quant(o.y.detach(), o.bias, o.res, c.act,
                                                              o.q.delta.detach(), o.q.zero_point.detach(),
                                                              x.n_bits))
    return got


def run_bwd(K, c, x, defer=False):
    with K.row_views():
        o = operands(K, c, x)
        with K.deferred_finalize(defer):
            out = K.epilogue(o.y, o.bias, o.gamma, o.phi, o.res, c.act, o.q)
            out.backward(dev(x.g))
        torch.cuda.synchronize()
        g = lambda t: None if t is None else host(t.grad)
        return {"out": host(out), "gy": g(o.y), "gres": g(o.rraw), "ggamma": g(o.gamma),
                "gphi": g(o.phi), "gdelta": None if o.q is None else g(o.q.delta),
                "gzp": None if o.q is None else g(o.q.zero_point)}


def run_tail(K, c, x, defer=False):
    with K.row_views():
        o = operands(K, c, x)
        lazy = K.epilogue(o.y, o.bias, o.gamma, o.phi, o.res, c.act, o.q, lazy=True)
        assert hasattr(lazy, "_ssq_tail"), "the fused tail refused the case"
        with K.deferred_finalize(defer):
            r = K.epilogue_loss_bwd(lazy._ssq_tail, K.Rows(dev(x.tcache), dev(x.idx)), x.M, c.p)
        torch.cuda.synchronize()
        names = ("loss", "gy", "gres", "ggamma", "gphi", "gdelta", "gzp", "gres_gamma", "gres_phi")
        return {k: host(v) for k, v in zip(names, r)}


def check_sums(c, ref, got, rec):
    for name, nk in EC.sums_of(c):
        S, A = np.asarray(getattr(ref, name), np.float64).reshape(-1), getattr(ref, name + "_abs")
        v = np.asarray(got[name], np.float64).reshape(-1)
        assert v.shape == S.shape, (name, v.shape, S.shape)
        if c.special:
            assert np.array_equal(np.isnan(v), np.isnan(S)), (name, v, S)
            continue
        bound = np.broadcast_to(EC.sum_bound(S, A, getattr(ref, nk)), S.shape)
        ratio = np.abs(v - S) / bound
        rec["sums"][name] = float(ratio.max())
        print(f"  {name}: worst error / bound {ratio.max():.3g} (n = {getattr(ref, nk)})")
    for name, r in rec["sums"].items():
        assert r <= 1.0, (EC.case_id(c), name, r)


def check_case(K, c, form=None):
    """Run and assert one case; returns its parity record.  form: the backward form the
    environment is expected to give the case (default: the case's own)."""
    x, ref = EC.inputs(c), EC.reference(c)
    rec = {"case": EC.case_id(c), "edge": c.edge, "sums": {}}
    nan_in = np.isnan(x.y)
    if c.kind != "tail":
        rec["fwd_form"] = EC.fwd_form_of(K, c)
        assert rec["fwd_form"] == c.fwd, (rec, c.fwd)
        f = run_fwd_only(K, c, x)
        for k, v in f.items():
            assert_bits(v, ref.pre_quant if k.startswith("pre_quant") else ref.out, k, nan_in)
        again = run_fwd_only(K, c, x)
        assert all(np.array_equal(bits(f[k]), bits(again[k])) for k in f), "forward not repeatable"
        if c.kind == "fwd":
            return rec
    rec["bwd_form"] = list(EC.bwd_form_of(K, c))
    assert tuple(rec["bwd_form"]) == (c.form if form is None else form), (rec, c.form, form)
    run = run_tail if c.kind == "tail" else run_bwd
    got = run(K, c, x)
    exact = c.kind != "tail" or c.p == 2.0
    ref_g = ref
    if not exact:
        # K11's gradient of the oracle's output: within K11's tolerance of the oracle's own,
        # and the gradient from which everything downstream is exact again
        g = host(K.lp_loss_and_grad(dev(ref.out), K.Rows(dev(x.tcache), dev(x.idx)), c.p)[1])
        np.testing.assert_allclose(g, ref.g, rtol=EC.LP_RTOL, atol=EC.LP_ATOL, err_msg="K11 gradient")
        ref_g = EC.reference_from_gradient(c, g)
    if c.kind != "tail":
        assert_bits(got["out"], ref.out, "out", nan_in)
    for k, wanted in (("gy", c.need_dy or c.kind == "tail"), ("gres", x.res is not None and c.want_gres)):
        assert (got[k] is not None) == wanted, k
        if not wanted:
            continue
        assert_bits(got[k], getattr(ref_g, k), k, nan_in)
        if not exact:
            np.testing.assert_allclose(got[k], getattr(ref, k), rtol=EC.LP_RTOL, atol=EC.LP_ATOL, err_msg=k)
    if c.kind == "tail":
        rtol, atol = (EC.LOSS_RTOL_P2, 0.0) if exact else (EC.LP_RTOL, EC.LP_ATOL)
        loss = float(got["loss"].reshape(-1)[0])
        np.testing.assert_allclose(loss, ref.loss, rtol=rtol, atol=atol)
        rec["loss_rel"] = abs(loss - ref.loss) / abs(ref.loss)
        print(f"  loss: relative error {rec['loss_rel']:.3g} (rtol {rtol:g})")
    check_sums(c, ref_g, got, rec)
    # repeated once: bit-identical (the delta ticket resets); deferred finalize the same bits
    for defer in (False, True) if c.defer else (False,):
        again = run(K, c, x, defer)
        for k, v in got.items():
            assert (v is None) == (again[k] is None), k
            if v is not None:
                nan = np.isnan(v)
                assert np.array_equal(nan, np.isnan(again[k])) and \
                    np.array_equal(bits(v[~nan]), bits(again[k][~nan])), (k, "defer" if defer else "repeat")
    return rec


def main(env_name):
    from shiftedscalequantization_amd import kernels as K
    env, forms = EC.WORKER_ENVS[env_name]
    for k, v in env.items():
        assert os.environ.get(k) == v, f"{k} is not {v} in this process"
    assert torch.cuda.is_available(), "no HIP device"
    hit = set()
    for c in EC.WORKER:
        form = None
        if c.kind != "fwd" and forms is not None:
            small, lazy = c.form[0] == 16, c.res in (EC.LAZY_BIAS, EC.LAZY_AFFINE)
            rpw = forms[c.kind][int(c.q is not None)] if small and not lazy else 1
            form = (rpw, c.form[1])
        if forms is None and c.kind != "tail":
            # SSQ_K13_PLANE4=0: the per-element plane form wherever the float4 form ran
            c = types.SimpleNamespace(**{**vars(c), "fwd": 1 if c.fwd == 2 else c.fwd})
        rec = check_case(K, c, form)
        hit.add(tuple(rec.get("bwd_form", ())) or ("fwd", rec["fwd_form"]))
        print("PARITY", json.dumps(dict(rec, env=env_name)))
    if forms is not None:
        want4 = any(4 in v for v in forms.values())
        assert any(h[0] == 4 for h in hit) == want4 and not any(h[0] == 16 for h in hit), hit
    print("worker OK", env_name, sorted(map(str, hit)))


if __name__ == "__main__":
    main(sys.argv[1])
