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

With `carry_blocks=True` the codes also cross a block's tail and its boundary: the block's last
conv runs ssq_qconv_i8_codes_res_fwd (the residual add, the block's activation and the block's
act quantizer in the conv kernel; the residual an fp32 tensor or the carried block input) and
the next block's readers, its identity residual among them, take the codes.  Which boundaries
qualify is structural again (`block_edges`: neighbours in an nn.Sequential, and the stages a
model declares with `stage_chain`); the trace confirms the readers' input quantizer.  A tagged
tensor that arrives where it is not the planned operand is decoded (K.materialize_epi), so a
condition that fails at run time costs time, never correctness.

With `carry_stem=True` the codes start at the model's front: the stem conv stays on the fp32
route (its input is an unquantized image), but its K13 epilogue leaves as codes
(ssq_epilogue_codes_fwd), a max-pool behind it pools the codes (ssq_maxpool_i8_fwd: a max-pool
commutes with the decode, which is non-decreasing in the code) and the first block's readers
take them.  The chain is structural once more (`stem_edges`, from the `stem_chain` a model
declares); the planning trace follows an act quantizer's output through such a pool, so the
layers behind it become eligible.

With `carry_head=True` the codes run to the logits: the global average pool in front of the
fc sums the carried codes of its input (ssq_avgpool_i8_digits_fwd: exact integers, stored as two
int8 digits) and the fc multiplies the sums with its prepared int8 weight
(ssq_qlinear_pooled_fwd), one int -> fp32 conversion and one multiply per logit.  The head has a
numerics contract of its own: its logits are a function of the codes alone, not bit
for bit those of an fp32 mean and an fp32 GEMM.  The chain is structural (`head_edges`, from
the `head_chain` a model declares); the fc is planned for the pooled operand only, so whenever
the pool does not pool codes the head is the fp32 one of the other routes.

With `colscale=True` a column-scaled weight ((q - zero_point[co]) * scale[co]) * c[j]
(ChannelQuantMSE, the form channelShift_wMSE puts on every conv) is planned too when its column
scale lies on an integer grid c[j] = k[j] / L, L <= 127 (K.colscale_grid, host arithmetic on the
J stored floats): the prepared int8 operand is the centred integer (q - zero_point[co]) * k[j]
(ssq_qweight_prepare_colscale; every element must fit int8, counted on the device otherwise),
the output scale fp32(fp32(delta * scale[co]) / fp32(L)), and the dense convs run the kernel
instantiation without the window-sum MFMA.  Such a layer carries and consumes codes
like any other; an all-ones column scale is a plain weight on the plain route.
"""
import torch
import torch.nn as nn
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
        self.head = None                        # a HeadCarry: the fc, on pooled digits only

    def accepts(self, cc):
        """A carried tensor (K.CarriedCodes) holds this layer's planned operand."""
        return cc.quantizer() == (self.delta, self.zp, self.n_bits, self.sym)

    def run_codes(self, x, bias, gamma, phi, relu, c=None, residual=None):
        """The layer's whole forward as the consumer's int8 operand.  `c`: the output quantizer
        and call counter (the layer's own Carry, or a block's TailCarry with the block's
        activation as `relu` and the tail's `residual`)."""
        c = self.carry if c is None else c
        self.calls += 1
        c.calls += 1
        codes = K.qconv_codes(x, self.prepared, self.scale, self.stride, self.padding,
                              groups=self.groups, act_zp=self.zp, act_bits=self.n_bits,
                              act_sym=self.sym, act_delta=self.delta, bias=bias, gamma=gamma,
                              phi=phi, relu=relu, out_delta=c.delta, out_zp=c.zp,
                              out_bits=c.n_bits, out_sym=c.sym, bad=self.counter,
                              residual=residual)
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


class TailCarry:
    """A block's carried output (carry_blocks): the block's last conv, the successor and its
    module readers, and the block's act quantizer as the readers' plans hold it."""

    def __init__(self, last, successor, entry, readers):
        p = readers[0]._int_plan
        self.last, self.successor, self.entry, self.readers = last, successor, entry, readers
        self.delta, self.zp, self.n_bits, self.sym = p.delta, p.zp, p.n_bits, p.sym
        self.calls = 0
        self.residual = None        # the kind the last emitting forward added


class StemCarry:
    """The stem's carried output (carry_stem): the producing conv, the pools its codes pass, the
    successor with its entry and module readers, and the producer's act quantizer as the
    readers' plans hold it."""

    def __init__(self, producer, pools, successor, entry, readers):
        p = readers[0]._int_plan
        self.producer, self.pools, self.successor = producer, list(pools), successor
        self.entry, self.readers = entry, readers
        self.delta, self.zp, self.n_bits, self.sym = p.delta, p.zp, p.n_bits, p.sym
        self.counter = p.counter
        self.calls = 0
        self.pooled = {m: 0 for m in self.pools}    # forwards in which a pool pooled codes

    def live(self):
        """The run-time state behind the producer is still the planned one."""
        mods = [self.entry] + self.readers
        if _hooked(self.successor, *self.pools, *mods):
            return False
        if any(m._int_stem is not self or m._plan() is None for m in self.pools):
            return False
        if any(m.cache_features != 'none' for m in mods):
            return False
        return all(m._int_plan is not None and m.use_weight_quant and m.use_act_quant
                   for m in self.readers)


class HeadCarry:
    """The carried head (carry_head): the producer (the last quant block, or a trailing
    QuantModule) whose codes the marked pool sums and the fc that reads the sums; the fc's plan
    holds the producer's act quantizer."""

    def __init__(self, producer, pool, fc):
        self.producer, self.pool, self.fc = producer, pool, fc
        self.calls = 0          # fc forwards on ssq_qlinear_pooled_fwd
        self.pooled = 0         # forwards in which the pool summed codes
        self._scale_h = {}      # HW -> K.head_scale(plan.scale, HW)
        self.emitter = None     # the producer's TailCarry / Carry: counts its emitting forwards

    def live(self):
        """The run-time state behind the pool is still the planned one."""
        fc, p = self.fc, self.fc._int_plan
        if torch.is_grad_enabled() or _hooked(self.pool, fc):
            return False
        if self.pool._int_head is not self or p is None or p.head is not self:
            return False
        return fc.cache_features == 'none' and fc.use_weight_quant and fc.use_act_quant

    def accepts(self, pc):
        """A pooled digit tensor (K.PooledCodes) holds the fc's planned operand."""
        p = self.fc._int_plan
        return (pc.quantizer() == (p.delta, p.zp, p.n_bits, p.sym)
                and pc.shape[1] == p.prepared.shape[1] and 1 <= pc.HW <= K.HEAD_MAX_HW)

    def run(self, hi, pc):
        p = self.fc._int_plan
        sh = self._scale_h.get(pc.HW)
        if sh is None:
            sh = self._scale_h[pc.HW] = K.head_scale(p.scale, pc.HW)
        self.calls += 1
        p.calls += 1
        return K.qlinear_pooled(hi, pc.lo, pc.sp, p.prepared, sh, pc.HW, p.zp, p.n_bits, p.sym)


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
def _trace_inputs(qnn, sample, pools=False, heads=()):
    """{QuantModule: the act quantizer whose output tensor is that module's input} from one
    forward of `sample`.  A hooked act quantizer runs unfused (fusable_act_quantizer), so its
    output is the very tensor object the next layer receives.  `pools` (carry_stem): the output
    of a max-pool the code kernel can run (SsqMaxPool2d with a plan) whose input is an act
    quantizer's output counts as that quantizer's: the same grid, delta and zero point.
    `heads` (carry_head): `head_edges`' (producer, pool, fc); a pool whose input is an act
    quantizer's output makes that quantizer the fc's source -- the structure guarantees that
    only a flatten lies between them, which makes a new tensor object -- and the pooled plane's
    H * W is left in `source[pool]`."""
    produced, keep, source, hooks = {}, [], {}, []
    via_pool = {}

    def post(q, args, out):
        if isinstance(out, torch.Tensor):
            produced[id(out)] = q
            keep.append(out)          # ids stay unique while the trace runs

    def post_pool(m, args, out):
        x = args[0] if args else None
        q = produced.get(id(x)) if isinstance(x, torch.Tensor) else None
        if q is not None:
            post(q, args, out)

    def post_head(fc):
        def hook(m, args, out):
            x = args[0] if args else None
            if isinstance(x, torch.Tensor) and x.dim() == 4:
                via_pool[fc] = produced.get(id(x))
                source[m] = int(x.shape[2] * x.shape[3])
        return hook

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
    for m in qnn.modules() if pools else ():
        if isinstance(m, K.SsqMaxPool2d) and m._plan() is not None:
            hooks.append(m.register_forward_hook(post_pool))
    for _, pool, fc in heads:
        hooks.append(pool.register_forward_hook(post_head(fc)))
    for m in layers:
        hooks.append(m.register_forward_pre_hook(pre))
        m.forward_raw = raw_of(m)
    try:
        qnn(sample)
        for fc, q in via_pool.items():
            if fc in source and source[fc] is None:
                source[fc] = q
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


def _weight_codes(m, colscale=False):
    """(packed codes, fields) of the module's hard weight: a restored model's PackedWeight as
    stored, a live quantizer through dequant_form + pack_encode (soft state is refused there).
    A column-scaled weight is encoded only with `colscale` (its caller refuses it otherwise)."""
    q = m.weight_quantizer
    if isinstance(q, PackedWeight):
        return q.packed, q.fields()
    what, f = dequant_form(m)
    if f["per_ci"] or (f["col_scale"] is not None and not colscale):
        return None, f
    packed, bad = K.pack_encode(what, f["zero_point"], f["scale"], f["per_ci"], f["col_scale"],
                                f["n_bits"], f["qmin"], f["qmax"])
    if bad:
        raise ValueError(f"{m.pathName or 'layer'}: {bad} weights are not integer codes of the "
                         f"{f['kind']} quantizer (soft state?)")
    return packed, f


@torch.no_grad()
def enable_integer_inference(qnn, sample, grouped=False, carry=False, carry_blocks=False,
                             carry_stem=False, carry_head=False, colscale=False):
    """Plan and install the integer route; returns {QuantModule name: "int8" | reason}.
    `sample` is one input batch (any batch size) for the planning forward, run in the model's
    current quantization state with weight and act quantization expected on.  `grouped`: also
    plan grouped and depthwise convs (K24-K26); off, they are reported as refused.  `carry`:
    also carry int8 codes between the integer layers of a block (`carry_report`).
    `carry_blocks`: `carry`, and the codes also cross block tails and block boundaries
    (`block_carry_report`).  `carry_stem`: `carry_blocks`, and the stem's epilogue emits codes
    that a max-pool behind it pools as codes (`stem_carry_report`); the layers behind such a
    pool are planned too.  `carry_head`: `carry_stem`, and the global average pool in front of
    the fc sums the codes and the fc runs on the sums (`head_carry_report`); the fc is planned
    for that operand only, and reported with the reason when the head edge is not installed.
    `colscale`: also plan column-scaled weights (ChannelQuantMSE) whose column scale lies on an
    integer grid k[j] / L, L <= 127 (K.colscale_grid), with the centred integer (q - z) * k[j] as
    the int8 operand; off, they are reported as refused.  An all-ones column scale is
    a plain weight and takes the plain route."""
    carry_stem = carry_stem or carry_head
    carry_blocks = carry_blocks or carry_stem
    carry = carry or carry_blocks
    disable_integer_inference(qnn)
    layers = _layers(qnn)
    if not layers:
        return {}
    heads = head_edges(qnn) if carry_head else []
    source = _trace_inputs(qnn, sample, pools=carry_stem, heads=heads)
    head_fc = {fc: pool for _, pool, fc in heads}
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
        if m in head_fc and not 1 <= source.get(head_fc[m], 0) <= K.HEAD_MAX_HW:
            report[name] = f"pooled plane H*W exceeds {K.HEAD_MAX_HW} (int8 digit range)"
            continue
        if not m.weight.is_cuda:
            report[name] = "weight is not on the HIP device"
            continue
        try:
            packed, f = _weight_codes(m, colscale)
        except TypeError as e:
            report[name] = str(e)
            continue
        if f["per_ci"]:
            report[name] = f"weight scale is per (co, ci) ({f['kind']})"
            continue
        kcol, L = None, 1
        if f["col_scale"] is not None:
            grid = K.colscale_grid(f["col_scale"]) if colscale else None
            if grid is None:
                report[name] = f"weight has a column scale ({f['kind']})" + (
                    f" that is not on an integer grid k / L, L <= {K.COLSCALE_MAX_L}" if colscale else "")
                continue
            L, kcol = grid
            if L == 1 and int(kcol.max()) == 1:
                kcol = None                     # all ones: a plain weight, the plain K22 blob
            elif m in head_fc:
                report[name] = (f"weight has a column scale ({f['kind']}): the pooled-operand fc "
                                "takes plain weights only")
                continue
        prep = K.qweight_prepare(packed, tuple(m.weight.shape), f["zero_point"], f["n_bits"],
                                 f["qmin"], groups=groups, kcol=kcol)
        if int(prep.bad.item()):
            report[name] = ("weight zero point is not an integer code" if kcol is None else
                            "scaled weight (q - z) * k leaves int8 (|m| > 127), or a zero point "
                            "is not an integer code")
            continue
        delta, zp, n_bits, sym = act
        # s[co] = fp32(delta_a * d1[co]): one fp32 product of the two stored fp32 values
        scale = (torch.full((1,), delta, dtype=torch.float32, device=dev)
                 * f["scale"].detach().reshape(-1).float()).contiguous()
        if kcol is not None:
            # ... / fp32(L): the column grid's common denominator, one more rounding
            scale = (scale / torch.full((1,), float(L), dtype=torch.float32, device=dev)).contiguous()
        m._int_plan = IntPlan(prep, scale, delta, zp, n_bits, sym, stride, padding, counter)
        report[name] = INT8
    if carry:
        _plan_carry(qnn, source)
    if carry_blocks:
        _plan_block_carry(qnn, source)
    if carry_stem:
        _plan_stem_carry(qnn, source)
    if carry_head:
        _plan_head_carry(qnn, source, heads, report, sample)
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


def _edge_entry(m):
    """The module a successor hands its input to and to nothing else: a quant block or a
    QuantModule itself, the first child (recursively) of an nn.Sequential; None otherwise."""
    from .quant_block import BaseQuantBlock
    while not isinstance(m, (BaseQuantBlock, QuantModule)):
        if not isinstance(m, nn.Sequential) or len(m) == 0:
            return None
        m = m[0]
    return m


def block_edges(qnn):
    """The (producer block, successor) module pairs where the producer's output goes to the
    successor and nowhere else, from the structure alone (no device, no forward): consecutive
    children of an nn.Sequential, the first a quant block, the second a quant block, a
    QuantModule or an nn.Sequential that starts with one; and, where the model declares the
    containers its forward applies back to back (`stage_chain()` on `qnn.model`), the last
    child of one stage and the first child of the next."""
    from .quant_block import BaseQuantBlock
    edges = []
    for seq in qnn.modules():
        if isinstance(seq, nn.Sequential):
            kids = list(seq)
            for a, b in zip(kids[:-1], kids[1:]):
                if isinstance(a, BaseQuantBlock) and _edge_entry(b) is not None:
                    edges.append((a, b))
    chain = getattr(getattr(qnn, "model", qnn), "stage_chain", None)
    stages = list(chain()) if callable(chain) else []
    for s0, s1 in zip(stages[:-1], stages[1:]):
        if not (isinstance(s0, nn.Sequential) and isinstance(s1, nn.Sequential) and len(s0) and len(s1)):
            continue
        if isinstance(s0[-1], BaseQuantBlock) and _edge_entry(s1[0]) is not None:
            edges.append((s0[-1], s1[0]))
    return edges


def _hooked(*mods):
    return any(m._forward_hooks or m._forward_pre_hooks for m in mods)


def block_act_code(blk):
    """The block activation as the kernels' code (0 identity, 1 ReLU, 2 ReLU6), None for any
    other."""
    from .quant_layer import StraightThrough
    f = blk.activation_function
    if isinstance(f, nn.ReLU6):
        return 2
    if isinstance(f, nn.ReLU):
        return 1
    return 0 if isinstance(f, StraightThrough) else None


def edge_readers(successor):
    """(entry module, the QuantModules that read the successor's input, whether the input is
    also an identity residual); readers None when the input has a reader that is not known."""
    from .quant_block import BaseQuantBlock
    entry = _edge_entry(successor)
    if isinstance(entry, QuantModule):
        return entry, [entry], False
    if isinstance(entry, BaseQuantBlock):
        readers = entry.input_readers()
        if readers is not None:
            return entry, list(readers), False
        readers = entry.identity_input_convs()
        if readers is not None:
            return entry, list(readers), True
    return entry, None, False


def _decoded_grouped(mod):
    """`mod` holds a grouped or depthwise conv that is not planned."""
    return any(isinstance(m, QuantModule) and m.fwd_kwargs.get("groups", 1) != 1
               and m._int_plan is None for m in mod.modules())


def _emitting_tail(blk):
    """The block's last conv when its tail can emit codes (see _plan_block_carry), else None."""
    from .quant_layer import StraightThrough
    last = blk.last_conv()
    plan = None if last is None else last._int_plan
    if plan is None or plan.kind != "dense":
        return None
    if not isinstance(last.activation_function, StraightThrough) or last.se_module is not None:
        return None
    if not last.disable_act_quant or not last.epilogue_fusable(last.weight):
        return None
    q = blk.act_quantizer
    if block_act_code(blk) is None or fusable_act_quantizer(q, True) is None:
        return None
    if _input_reason(q)[0] is None:
        return None
    return last


def _plan_block_carry(qnn, source):
    """Install a TailCarry on every block of `block_edges` whose tail can emit codes: the last
    conv a planned dense conv whose epilogue the kernel applies (no activation or act
    quantizer of its own, no SE module), the block's activation and act quantizer ones the
    kernel applies, every reader of the successor planned with the block's act quantizer as
    its traced input, no grouped or depthwise conv of either side left on the decoded path
    (without `grouped=True` a MobileNetV2 / RegNetX block has one in its middle: such a block
    keeps its fp32 edges), and no hook that would see the tensor."""
    for blk, succ in block_edges(qnn):
        last = _emitting_tail(blk)
        if last is None:
            continue
        q = blk.act_quantizer
        entry, readers, _ = edge_readers(succ)
        if not readers or any(m._int_plan is None or source.get(m) is not q for m in readers):
            continue
        if any(_decoded_grouped(m) for m in (blk, entry)):
            continue
        if _hooked(blk, last, succ, entry, *readers):
            continue
        blk._int_tail = TailCarry(last, succ, entry, readers)


def stem_edges(qnn):
    """The (producer QuantModule, [max-pools], successor) chains from the stem conv to the first
    stage, from the structure alone (no device, no forward): the `stem_chain()` the model
    declares on `qnn.model`, whose first entry is a QuantModule -- itself, or an nn.Sequential
    of one followed by StraightThrough only --, whose entries in between are StraightThrough or
    a max-pool the code kernel can run (SsqMaxPool2d with a plan), and whose last entry has an
    `_edge_entry`.  Empty for any other chain and for a model that declares none."""
    from .fold_bn import StraightThrough as FoldedBN
    from .quant_layer import StraightThrough as MovedAct
    StraightThrough = (FoldedBN, MovedAct)      # a folded BN's and a moved activation's identity
    chain = getattr(getattr(qnn, "model", qnn), "stem_chain", None)
    mods = list(chain()) if callable(chain) else []
    if len(mods) < 2:
        return []
    prod = mods[0]
    if isinstance(prod, nn.Sequential):
        kids = list(prod)
        if not kids or not all(isinstance(k, StraightThrough) for k in kids[1:]):
            return []
        prod = kids[0]
    if not isinstance(prod, QuantModule):
        return []
    pools = []
    for m in mods[1:-1]:
        if isinstance(m, K.SsqMaxPool2d) and m._plan() is not None:
            pools.append(m)
        elif not isinstance(m, StraightThrough):
            return []
    if _edge_entry(mods[-1]) is None:
        return []
    return [(prod, pools, mods[-1])]


def _plan_stem_carry(qnn, source):
    """Install a StemCarry on the producer of every `stem_edges` chain that can emit codes: a
    conv on the fp32 route whose epilogue and act quantizer K27 applies (no SE module), every
    reader of the successor planned with that act quantizer as its traced input (through the
    pools), no grouped or depthwise conv of the entry left on the decoded path (the block-edge
    rule), and no hook that would see the tensor.  The pools are marked with the same object."""
    for prod, pools, succ in stem_edges(qnn):
        if prod._int_plan is not None or prod.fwd_func is not F.conv2d:
            continue
        if prod.se_module is not None or prod.disable_act_quant:
            continue
        if not prod.epilogue_fusable(prod.weight) or prod.act_code() not in (0, 1, 2):
            continue
        q = prod.act_quantizer
        if fusable_act_quantizer(q, True) is None or _input_reason(q)[0] is None:
            continue
        entry, readers, _ = edge_readers(succ)
        if not readers or any(m._int_plan is None or source.get(m) is not q for m in readers):
            continue
        if _decoded_grouped(entry):
            continue
        if _hooked(prod, succ, entry, *pools, *readers):
            continue
        prod._int_stem = StemCarry(prod, pools, succ, entry, readers)
        for m in pools:
            m._int_stem = prod._int_stem


def head_edges(qnn):
    """The (producer, pool, fc) chains of the pooling head, from the structure alone (no device,
    no forward): the `head_chain()` the model declares on `qnn.model`, [last stage, pool,
    classifier].  The producer is the stage's last child when that is a quant block, or -- an
    nn.Sequential there -- a trailing QuantModule followed by StraightThrough only (MobileNetV2's
    `features.18`); the pool is a K.SsqGlobalAvgPool; the classifier a Linear QuantModule, or an
    nn.Sequential that ends in one behind nn.Dropout / nn.Flatten / identities only.  Empty for
    any other chain and for a model that declares none."""
    from .fold_bn import StraightThrough as FoldedBN
    from .quant_block import BaseQuantBlock
    from .quant_layer import StraightThrough as MovedAct
    ident = (FoldedBN, MovedAct, nn.Identity)
    chain = getattr(getattr(qnn, "model", qnn), "head_chain", None)
    mods = list(chain()) if callable(chain) else []
    if len(mods) != 3:
        return []
    prod, pool, fc = mods
    while isinstance(prod, nn.Sequential) and len(prod):
        kids = list(prod)
        while len(kids) > 1 and isinstance(kids[-1], ident):
            kids.pop()
        prod = kids[-1]
    if not isinstance(prod, (BaseQuantBlock, QuantModule)):
        return []
    if isinstance(prod, QuantModule) and prod.fwd_func is not F.conv2d:
        return []
    if not isinstance(pool, K.SsqGlobalAvgPool):
        return []
    if isinstance(fc, nn.Sequential):
        kids = list(fc)
        if not kids or not all(isinstance(k, ident + (nn.Dropout, nn.Flatten)) for k in kids[:-1]):
            return []
        fc = kids[-1]
    if not isinstance(fc, QuantModule) or fc.fwd_func is not F.linear:
        return []
    return [(prod, pool, fc)]


def _reset_calls(qnn):
    """Zero every forward counter of the installed plan (after the head's dry forward)."""
    from .quant_block import BaseQuantBlock
    for m in qnn.modules():
        p = getattr(m, "_int_plan", None) if isinstance(m, QuantModule) else None
        if p is not None:
            p.calls = 0
            if p.carry is not None:
                p.carry.calls = 0
        s = getattr(m, "_int_stem", None) if isinstance(m, QuantModule) else None
        if s is not None:
            s.calls = 0
            s.pooled = {k: 0 for k in s.pooled}
        t = getattr(m, "_int_tail", None) if isinstance(m, BaseQuantBlock) else None
        if t is not None:
            t.calls, t.residual = 0, None
        h = getattr(m, "_int_head", None) if isinstance(m, K.SsqGlobalAvgPool) else None
        if h is not None:
            h.calls = h.pooled = 0
    if getattr(qnn, "_int_counter", None) is not None:
        qnn._int_counter.zero_()


def _plan_head_carry(qnn, source, heads, report, sample):
    """Install a HeadCarry on every `head_edges` chain whose producer can emit codes for the
    pool: a quant block whose tail emits under the block-edge rules with the fc as its reader
    (ssq_qconv_i8_codes[_res]_fwd; a carried block input is then the RES = 2 residual), or a
    trailing QuantModule under the interior-pair rules (ssq_qconv_i8_codes_fwd); the fc planned
    with the producer's act quantizer as its traced input (through the pool); no hook that would
    see the tensors; and a dry forward of `sample` under the installed plan that shows the
    pooled digits arriving at the fc.  An fc whose edge is not installed loses its plan -- it
    is planned for pooled digits only -- and is reported with the reason."""
    from .quant_block import BaseQuantBlock
    names = {m: n for n, m in qnn.named_modules()}
    for prod, pool, fc in heads:
        if fc._int_plan is None:
            continue        # refused by the weight / input rules: the report says why
        why = None
        if isinstance(prod, BaseQuantBlock):
            q, last = prod.act_quantizer, _emitting_tail(prod)
            if last is None:
                why = "the last block's tail cannot emit codes"
            elif _decoded_grouped(prod):
                why = "the last block holds a grouped conv on the decoded path"
            elif getattr(prod, "_int_tail", None) is not None:
                why = "the last block already emits codes for another edge"
        else:
            q = prod.act_quantizer
            if (prod._int_plan is None or prod.disable_act_quant or prod.se_module is not None
                    or fusable_act_quantizer(q, True) is None
                    or not prod.epilogue_fusable(prod.weight) or prod.act_code() not in (0, 1, 2)
                    or prod._int_plan.carry is not None):
                why = "the last layer cannot emit codes"
        if why is None and source.get(fc) is not q:
            why = "the pool's input is not the last block's act quantizer output"
        if why is None and _hooked(prod, pool, fc, *([last] if isinstance(prod, BaseQuantBlock) else [])):
            why = "a forward hook on the last block, the pool or the fc"
        if why is None:
            head = HeadCarry(prod, pool, fc)
            fc._int_plan.head = pool._int_head = head
            if isinstance(prod, BaseQuantBlock):
                head.emitter = prod._int_tail = TailCarry(last, pool, fc, [fc])
            else:
                head.emitter = prod._int_plan.carry = Carry(fc)
            head.emitter.head = head
            try:
                qnn(sample)
            except K.A.SSQError as e:
                why = f"the dry forward failed: {e}"
            else:
                if not head.calls:
                    why = "the dry forward did not bring pooled codes to the fc"
            _reset_calls(qnn)
            if why is not None:
                pool._int_head = None
                if isinstance(prod, BaseQuantBlock):
                    prod._int_tail = None
                else:
                    prod._int_plan.carry = None
        if why is not None:
            fc._int_plan = None
            report[names[fc]] = f"no head edge: {why}"


def disable_integer_inference(qnn):
    """Every layer back on the decoded fp32 path."""
    from .quant_block import BaseQuantBlock
    for _, m in _layers(qnn):
        m._int_plan = None
        m._int_stem = None
    for m in qnn.modules():
        if isinstance(m, BaseQuantBlock):
            m._int_tail = None
        elif isinstance(m, K.SsqMaxPool2d):
            m._int_stem = None
        elif isinstance(m, K.SsqGlobalAvgPool):
            m._int_head = None
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
        if c is not None and getattr(c, "head", None) is None:
            pairs.append((n, names[c.consumer]))
            calls[n] = c.calls
    return {"pairs": pairs, "calls": calls}


def block_carry_report(qnn):
    """{"edges": [(block name, successor name), ...] whose block tail the installed plan lets
    emit int8 codes, "calls": {block name: forwards whose tail emitted codes}, "residual":
    {block name: "none" | "fp32" | "codes", the residual operand of the emitting tail: as the
    last emitting forward had it, before one as the plan expects it}}; empty without a plan."""
    from .quant_block import BaseQuantBlock
    names = {m: n for n, m in qnn.named_modules()}
    tails = [(n, m) for n, m in qnn.named_modules()
             if isinstance(m, BaseQuantBlock) and getattr(m, "_int_tail", None) is not None
             and getattr(m._int_tail, "head", None) is None]
    fed = {m._int_tail.entry for _, m in tails}
    fed |= {m._int_stem.entry for _, m in _layers(qnn) if getattr(m, "_int_stem", None) is not None}
    edges, calls, residual = [], {}, {}
    for n, blk in tails:
        t = blk._int_tail
        edges.append((n, names[t.successor]))
        calls[n] = t.calls
        kind = t.residual
        if kind is None and blk.identity_input_convs() is not None:
            kind = "codes" if blk in fed else "fp32"
        elif kind is None:
            kind = "none" if getattr(blk, "downsample", None) is None else "fp32"
        residual[n] = kind
    return {"edges": edges, "calls": calls, "residual": residual}


def stem_carry_report(qnn):
    """{"edges": [(producer name, [pool names], successor name), ...] whose producer the
    installed plan lets emit int8 codes, "calls": {producer name: forwards that emitted codes},
    "pooled": {pool name: forwards that pooled codes}}; empty without a plan."""
    names = {m: n for n, m in qnn.named_modules()}
    edges, calls, pooled = [], {}, {}
    for n, m in _layers(qnn):
        s = getattr(m, "_int_stem", None)
        if s is not None:
            edges.append((n, [names[p] for p in s.pools], names[s.successor]))
            calls[n] = s.calls
            pooled.update({names[p]: k for p, k in s.pooled.items()})
    return {"edges": edges, "calls": calls, "pooled": pooled}


def head_carry_report(qnn):
    """{"edges": [(producer name, pool name, fc name), ...] the installed plan carries int8
    codes along, "calls": {producer name: forwards that emitted codes for the pool}, "pooled":
    {pool name: forwards that summed codes (ssq_avgpool_i8_digits_fwd)}, "fc": {fc name: forwards
    on ssq_qlinear_pooled_fwd}}; empty without a plan."""
    names = {m: n for n, m in qnn.named_modules()}
    out = {"edges": [], "calls": {}, "pooled": {}, "fc": {}}
    for m in qnn.modules():
        h = getattr(m, "_int_head", None) if isinstance(m, K.SsqGlobalAvgPool) else None
        if h is not None:
            out["edges"].append((names[h.producer], names[h.pool], names[h.fc]))
            out["calls"][names[h.producer]] = h.emitter.calls
            out["pooled"][names[h.pool]] = h.pooled
            out["fc"][names[h.fc]] = h.calls
    return out
