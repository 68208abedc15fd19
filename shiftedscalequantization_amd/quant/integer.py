"""Integer inference of a calibrated model (K21-K23, csrc/qinfer.hip; grouped and depthwise
convs on K24-K26, csrc/qinfer_grouped.hip, with `grouped=True`).

A QuantModule whose input is the direct output of an act quantizer (scalar delta, integer
zero point) and whose hard weight is (q - zero_point[co]) * scale[co] runs its conv / linear
on the integer codes: the input is re-encoded to int8 (ssq_act_encode), multiplied with the
layer's prepared int8 weight on the int8 MFMA (ssq_qconv_i8_fwd) and leaves as
fp32(I) * fp32(delta_a * scale[co]).  The raw output then takes the module's unchanged bias /
gamma^z, phi^z / activation / act-quant epilogue.  Every other layer keeps the decoded fp32
path.  The switch is off until `enable_integer_inference` installs a plan; the plan holds the
act quantizers' (delta, zero_point) as of that call, so re-enable after changing them.

With `carry=True` the tensor between two integer layers of one block stays int8: the producer
runs the code-emitting kernels (ssq_qconv_i8_codes_fwd / ssq_qconv_i8_grouped_codes_fwd:
conv, bias, gamma^z / phi^z, activation and its act quantizer in one launch) and the consumer
takes the codes as its operand, so the K13 epilogue pass and the K21 re-encode between them
drop out.  Only the pairs a block declares (`BaseQuantBlock.interior_chain`) are carried: the
planning trace sees module inputs, not residual adds or pooling, so the block's structure is
what guarantees the producer's output has one reader.
"""
import torch
import torch.nn.functional as F

from .. import kernels as K
from .export import PackedWeight, dequant_form
from .quant_layer import QuantModule, UniformAffineQuantizer, fusable_act_quantizer

INT8 = "int8"


class IntPlan:
    """One layer's installed integer route."""

    def __init__(self, prepared, scale, delta, zp, n_bits, sym, stride, padding, counter):
        self.prepared, self.scale = prepared, scale
        self.groups = prepared.groups
        self.kind = K.qconv_kind(prepared)      # "dense" | "depthwise" | "grouped"
        self.delta, self.zp, self.n_bits, self.sym = delta, zp, n_bits, sym
        self.stride, self.padding = stride, padding
        self.counter = counter
        self.calls = 0
        self.carry = None                       # a Carry when this layer emits codes

    def accepts(self, cc):
        """A carried tensor (K.CarriedCodes) holds this layer's planned operand."""
        return cc.quantizer() == (self.delta, self.zp, self.n_bits, self.sym)

    def run_codes(self, x, bias, gamma, phi, relu):
        """The layer's whole forward as the consumer's int8 operand."""
        c = self.carry
        self.calls += 1
        c.calls += 1
        codes = K.qconv_codes(x, self.prepared, self.scale, self.stride, self.padding,
                              groups=self.groups, act_zp=self.zp, act_bits=self.n_bits,
                              act_sym=self.sym, act_delta=self.delta, bias=bias, gamma=gamma,
                              phi=phi, relu=relu, out_delta=c.delta, out_zp=c.zp,
                              out_bits=c.n_bits, out_sym=c.sym, bad=self.counter)
        N, H, W, _ = codes.shape
        return K.carried(codes, (N, self.prepared.shape[0], H, W), c.delta, c.zp, c.n_bits, c.sym)

    def run(self, x):
        self.calls += 1
        return K.qconv(x, self.prepared, self.scale, self.stride, self.padding,
                       groups=self.groups, act_zp=self.zp,
                       act_bits=self.n_bits, act_sym=self.sym, act_delta=self.delta,
                       bad=self.counter)


class Carry:
    """A producer's carried output: the consumer and the producer's act quantizer as the
    consumer's plan holds it."""

    def __init__(self, consumer):
        p = consumer._int_plan
        self.consumer = consumer
        self.delta, self.zp, self.n_bits, self.sym = p.delta, p.zp, p.n_bits, p.sym
        self.calls = 0


def _layers(qnn):
    return [(n, m) for n, m in qnn.named_modules() if isinstance(m, QuantModule)]


def _act_quantizers(qnn):
    seen, out = set(), []
    for m in qnn.modules():
        aq = getattr(m, "act_quantizer", None)
        if isinstance(aq, torch.nn.Module) and id(aq) not in seen:
            seen.add(id(aq))
            out.append(aq)
    return out


@torch.no_grad()
def _trace_inputs(qnn, sample):
    """{QuantModule: the act quantizer whose output tensor is that module's input} from one
    forward of `sample`.  A hooked act quantizer runs unfused (fusable_act_quantizer), so its
    output is the very tensor object the next layer receives."""
    produced, keep, source, hooks = {}, [], {}, []

    def post(q, args, out):
        if isinstance(out, torch.Tensor):
            produced[id(out)] = q
            keep.append(out)          # ids stay unique while the trace runs

    def pre(m, args):
        x = args[0] if args else None
        source[m] = produced.get(id(x)) if isinstance(x, torch.Tensor) else None

    def raw_of(m):
        def forward_raw(x):     # a block's fused tail calls forward_raw, not forward
            pre(m, (x,))
            return type(m).forward_raw(m, x)
        return forward_raw

    layers = [m for _, m in _layers(qnn)]
    for q in _act_quantizers(qnn):
        hooks.append(q.register_forward_hook(post))
    for m in layers:
        hooks.append(m.register_forward_pre_hook(pre))
        m.forward_raw = raw_of(m)
    try:
        qnn(sample)
    finally:
        for h in hooks:
            h.remove()
        for m in layers:
            del m.forward_raw
    return source


def _input_reason(q):
    if q is None:
        return None, "input is not the direct output of an act quantizer"
    if type(q) is not UniformAffineQuantizer or not q.inited or q.delta is None:
        return None, "input act quantizer is not an initialised UniformAffineQuantizer"
    if q.delta.numel() != 1 or q.zero_point.numel() != 1:
        return None, "input act quantizer is not per-tensor"
    delta, zp = float(q.delta.detach().float()), float(q.zero_point.detach().float())
    lo, hi = K.qrange(q.n_bits, q.sym)
    if not (delta > 0.0 and delta == delta and delta != float("inf")):
        return None, "input act quantizer's delta is not positive and finite"
    if zp != round(zp) or not lo <= zp <= lo + 255:
        return None, f"input act quantizer's zero point {zp} is not an integer in [{lo}, {lo + 255}]"
    if q.n_bits < 2:
        return None, "activation bits below 2"
    return (delta, zp, q.n_bits, q.sym), None


def _weight_codes(m):
    """(packed codes, fields) of the module's hard weight: a restored model's PackedWeight as
    stored, a live quantizer through dequant_form + pack_encode (soft state is refused there)."""
    q = m.weight_quantizer
    if isinstance(q, PackedWeight):
        return q.packed, q.fields()
    what, f = dequant_form(m)
    if f["per_ci"] or f["col_scale"] is not None:
        return None, f
    packed, bad = K.pack_encode(what, f["zero_point"], f["scale"], f["per_ci"], f["col_scale"],
                                f["n_bits"], f["qmin"], f["qmax"])
    if bad:
        raise ValueError(f"{m.pathName or 'layer'}: {bad} weights are not integer codes of the "
                         f"{f['kind']} quantizer (soft state?)")
    return packed, f


@torch.no_grad()
def enable_integer_inference(qnn, sample, grouped=False, carry=False):
    """Plan and install the integer route; returns {QuantModule name: "int8" | reason}.
    `sample` is one input batch (any batch size) for the planning forward, run in the model's
    current quantization state with weight and act quantization expected on.  `grouped`: also
    plan grouped and depthwise convs (K24-K26); off, they are reported as refused.  `carry`:
    also carry int8 codes between the integer layers of a block (`carry_report`)."""
    disable_integer_inference(qnn)
    layers = _layers(qnn)
    if not layers:
        return {}
    source = _trace_inputs(qnn, sample)
    dev = layers[0][1].weight.device
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    qnn._int_counter = counter
    report = {}
    for name, m in layers:
        if m not in source:
            report[name] = "not reached by the planning forward"
            continue
        if m.fwd_func is F.conv2d:
            kw = m.fwd_kwargs
            groups = int(kw["groups"])
            if groups != 1 and not grouped:
                report[name] = f"grouped conv (groups = {kw['groups']})"
                continue
            st, pd, dl = kw["stride"], kw["padding"], kw["dilation"]
            if isinstance(pd, str) or st[0] != st[1] or pd[0] != pd[1] or tuple(dl) != (1, 1):
                report[name] = "stride / padding not square or dilation != 1"
                continue
            if max(m.weight.shape[2:]) > 7:
                report[name] = "kernel larger than 7x7"
                continue
            stride, padding = int(st[0]), int(pd[0])
        elif m.fwd_func is F.linear:
            stride, padding, groups = 1, 0, 1
        else:
            report[name] = "neither a conv nor a linear"
            continue
        if m.weight[0].numel() > 65536:
            report[name] = "K = Ci*R*S exceeds 65536"
            continue
        if not (m.use_weight_quant and m.use_act_quant):
            report[name] = "weight and act quantization are not both on"
            continue
        act, why = _input_reason(source[m])
        if act is None:
            report[name] = why
            continue
        if not m.weight.is_cuda:
            report[name] = "weight is not on the HIP device"
            continue
        try:
            packed, f = _weight_codes(m)
        except TypeError as e:
            report[name] = str(e)
            continue
        if f["per_ci"]:
            report[name] = f"weight scale is per (co, ci) ({f['kind']})"
            continue
        if f["col_scale"] is not None:
            report[name] = f"weight has a column scale ({f['kind']})"
            continue
        prep = K.qweight_prepare(packed, tuple(m.weight.shape), f["zero_point"], f["n_bits"],
                                 f["qmin"], groups=groups)
        if int(prep.bad.item()):
            report[name] = "weight zero point is not an integer code"
            continue
        delta, zp, n_bits, sym = act
        # s[co] = fp32(delta_a * d1[co]): one fp32 product of the two stored fp32 values
        scale = (torch.full((1,), delta, dtype=torch.float32, device=dev)
                 * f["scale"].detach().reshape(-1).float()).contiguous()
        m._int_plan = IntPlan(prep, scale, delta, zp, n_bits, sym, stride, padding, counter)
        report[name] = INT8
    if carry:
        _plan_carry(qnn, source)
    return report


def _plan_carry(qnn, source):
    """Install a Carry on every producer of a block's interior chain whose pair can stay int8:
    both planned, the consumer's traced input quantizer the producer's own act quantizer, the
    producer's epilogue one the kernel applies (fusable quantizer and epilogue, no SE module),
    and no hook that would see the tensor."""
    from .quant_block import BaseQuantBlock
    for blk in qnn.modules():
        if not isinstance(blk, BaseQuantBlock):
            continue
        for prod, cons in blk.interior_chain():
            if prod._int_plan is None or cons._int_plan is None:
                continue
            q = prod.act_quantizer
            if source.get(cons) is not q or prod.disable_act_quant:
                continue
            if fusable_act_quantizer(q, True) is None or prod.se_module is not None:
                continue
            # (the weight stands in for the input: epilogue_fusable asks for its device only)
            if not prod.epilogue_fusable(prod.weight) or prod.act_code() not in (0, 1, 2):
                continue
            if any(m._forward_hooks or m._forward_pre_hooks for m in (prod, cons)):
                continue
            prod._int_plan.carry = Carry(cons)


def disable_integer_inference(qnn):
    """Every layer back on the decoded fp32 path."""
    for _, m in _layers(qnn):
        m._int_plan = None
    qnn._int_counter = None


def integer_report(qnn):
    """{"off_grid": elements seen by the integer layers that were not on their act quantizer's
    grid (0 = every integer layer computed what the decoded path computes up to fp32
    rounding), "calls": {layer name: forwards taken on the integer route}}.  Reads one device
    word (the only sync of the integer path)."""
    counter = getattr(qnn, "_int_counter", None)
    calls = {n: m._int_plan.calls for n, m in _layers(qnn) if getattr(m, "_int_plan", None) is not None}
    return {"off_grid": int(counter.item()) if counter is not None else 0, "calls": calls}


def carry_report(qnn):
    """{"pairs": [(producer name, consumer name), ...] the installed plan carries int8 codes
    between, "calls": {producer name: forwards that emitted codes}}; empty without a plan."""
    names = {m: n for n, m in _layers(qnn)}
    pairs, calls = [], {}
    for n, m in _layers(qnn):
        c = getattr(getattr(m, "_int_plan", None), "carry", None)
        if c is not None:
            pairs.append((n, names[c.consumer]))
            calls[n] = c.calls
    return {"pairs": pairs, "calls": calls}
