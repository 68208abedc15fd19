"""Integer inference of a calibrated model (K21-K30, csrc/qinfer*.hip).

A QuantModule whose input is the direct output of a per-tensor act quantizer and whose hard
weight is (q - zero_point[co]) * scale[co] runs its conv / linear on int8 codes and leaves as
fp32(I) * fp32(delta_a * scale[co]); its bias / gamma^z, phi^z / activation / act-quant epilogue is
unchanged.  Every other layer keeps the decoded fp32 path.  `enable_integer_inference` installs
the plan (an IntPlan per layer); it holds the act quantizers' values as of that call, so
re-enable after changing them.  `grouped=True` plans grouped and depthwise convs too (K24-K26);
`colscale=True` plans column-scaled weights (ChannelQuantMSE) whose column scale lies on an
integer grid k[j] / L, L <= 127 (K.colscale_grid), with the centred integer (q - z) * k[j] as the
int8 operand.  `per_ci=True` plans weights whose scale is per (co, ci) on a grid base[co] * k / L
(ChannelQuant's shifted scale; K.perci_grid) the same way, with (q - z) * k[co, ci] as the operand,
and `wide=True` lets either kind of scaled weight whose operand leaves int8 run as two int8
digits (|m| <= 16319) on K23's wide forms; `wide_all=True` (with `wide`) extends that operand to
the grouped and depthwise kernels (K26 / K25) and to the pooled-operand fc (K30), which then also
takes a scaled weight.

The carry flags keep a tensor between integer layers as int8 codes.  Each such tensor is one
Edge: an emitting layer whose kernel applies the epilogue and the act quantizer and stores the
codes, the readers whose planned operand the codes are, and the grid (K.ActQuant: delta, zp,
n_bits, sym) they lie on.  Where the edges are is structural, because the planning trace sees
module inputs, not residual adds or pooling:
  carry         PairEdge  the pairs a block declares (`BaseQuantBlock.interior_chain`)
  carry_blocks  TailEdge  a block's last conv with the residual add, the block's activation and
                          act quantizer in its kernel, read by the next block (`block_edges`)
  carry_stem    StemEdge  the stem conv's fp32 epilogue leaves as codes, max-pools behind it pool
                          the codes, the first block reads them (`stem_edges`); with
                          `fused_stem` the conv itself emits them (K31, fp32 MFMA)
  carry_head    HeadEdge  the global average pool sums the last producer's codes and the fc runs
                          on the sums (`head_edges`); its logits are a function of the codes
                          alone, not bit for bit those of an fp32 mean and GEMM
Two rules decide whether an edge is installed: the emitter can emit onto the quantizer
(`can_emit`) and the readers take the tensor (`readers_refuse`).  One rule decides at run time
whether it still carries (`Edge.live`, over the modules of `Edge.watched`).  A tagged tensor
that arrives where it is not the planned operand is decoded (K.materialize_epi), so a condition
that fails at run time costs time, never correctness.  The installed edges are listed in
`qnn._int_edges`; the marks the forwards read (`_int_plan.carry`, `_int_tail`, `_int_stem`,
`_int_head`) are set and cleared through that list only.

Two opt-in forms for the small planes, where launches and a starved grid cost more than bytes:
`enable_integer_inference(..., splitk=True)` lets a dense layer take K23's split-K form where the
host rule K.qconv_splits asks for it (the same bits; `split_report`), and `IntegerGraph` replays
the whole forward as one captured HIP graph.
"""
import collections
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import kernels as K
from . import quant_layer as L
from .channelQuantAct import ChannelQuantAct
from .export import PackedWeight, dequant_form
from .fold_bn import StraightThrough as FoldedBN
from .quant_block import BaseQuantBlock
from .quant_layer import (QuantModule, StraightThrough, UniformAffineQuantizer, act_code,
                          fusable_act_quantizer)

INT8 = "int8"


class IntPlan:
    """One layer's installed integer route; `grid`: the act quantizer of its input."""

    def __init__(self, prepared, scale, grid, stride, padding, counter):
        self.prepared, self.scale, self.grid = prepared, scale, grid
        self.groups = prepared.groups
        self.kind = K.qconv_kind(prepared)      # "dense" | "depthwise" | "grouped"
        self.stride, self.padding = stride, padding
        self.counter = counter
        # the input operand's arguments of K.qconv / K.qconv_codes
        self._operand = dict(groups=self.groups, act_zp=grid.zp, act_bits=grid.n_bits,
                             act_sym=grid.sym, act_delta=grid.delta, bad=counter)
        self.calls = 0
        self.carry = None                       # a PairEdge when this layer emits codes
        self.head = None                        # a HeadEdge: the fc, on pooled digits only
        self.head_grid = None                   # a scaled fc: (fp32(delta_a * base[co]), L)
        self.splitk = False                     # dense only: ask K.qconv_splits per call
        self.splits = None                      # the Z of the last run / run_codes
        Co, Ci, R, S = prepared.geometry()
        self._Kp = -(-R * S * (-(-Ci // 16) * 16) // 64) * 64     # the blob's padded taps (QLayout)

    def _splits(self, x):
        """{"splits": K.qconv_splits for this call's M = N * OH * OW} (M depends on the batch), the
        Z kept for `split_report`; only a plan with `splitk` comes here."""
        cc = getattr(x, '_ssq_codes', None)
        shape = x.shape if cc is None else cc.shape
        Co, _, R, S = self.prepared.geometry()
        M = int(shape[0])
        if len(shape) == 4:
            M *= (((int(shape[2]) + 2 * self.padding - R) // self.stride + 1)
                  * ((int(shape[3]) + 2 * self.padding - S) // self.stride + 1))
        self.splits = K.qconv_splits(M, Co, self._Kp)
        return {"splits": self.splits}

    # the input grid's fields under the plan's own names (views, not copies)
    delta, zp, n_bits, sym = (property(lambda self, i=i: self.grid[i]) for i in range(4))

    def accepts(self, cc):
        """A carried tensor (K.CarriedCodes) holds this layer's planned operand."""
        return cc.quantizer() == self.grid

    def takes(self, x):
        """`x` is an operand of the code-emitting kernels: the planned codes or an fp32 tensor."""
        cc = getattr(x, '_ssq_codes', None)
        return self.accepts(cc) if cc is not None else x.dtype == torch.float32

    def emit(self, x):
        """QuantModule.forward's question: the forward as carried codes, or None."""
        return None if self.carry is None else self.carry.emit(x)

    def run_codes(self, x, bias, gamma, phi, relu, edge, residual=None):
        """The layer's whole forward as `edge`'s int8 codes (`relu`: the activation's code)."""
        o = edge.grid
        self.calls += 1
        edge.calls += 1
        codes = K.qconv_codes(x, self.prepared, self.scale, self.stride, self.padding, bias=bias,
                              gamma=gamma, phi=phi, relu=relu, out_delta=o.delta, out_zp=o.zp,
                              out_bits=o.n_bits, out_sym=o.sym, residual=residual, **self._operand,
                              **(self._splits(x) if self.splitk else {}))
        N, H, W, _ = codes.shape
        return K.carried(codes, (N, self.prepared.shape[0], H, W), *o)

    def run(self, x):
        self.calls += 1
        if self.splitk:
            return K.qconv(x, self.prepared, self.scale, self.stride, self.padding, **self._operand,
                           **self._splits(x))
        return K.qconv(x, self.prepared, self.scale, self.stride, self.padding, **self._operand)


def _hooked(*mods):
    return any(m._forward_hooks or m._forward_pre_hooks for m in mods)


def can_emit(m, q, own, x=None):
    """Layer `m` can leave as codes of act quantizer `q`: its own (`own`; the layer then has
    act quantization of its own), or its block's, whose tail `m` then is with neither activation
    nor act quantizer of its own.  Its epilogue is one the kernels apply (a conv, no SE module, a
    known activation: epilogue_fusable) and `q` one they apply (fusable_act_quantizer).  `x`: the
    input at run time; None at plan time, where the weight stands in for it and `q`'s values
    must be ones a plan can hold (_input_reason)."""
    if own == m.disable_act_quant or not (own or isinstance(m.activation_function, StraightThrough)):
        return False
    if x is None and _input_reason(q)[0] is None:
        return False
    x = m.weight if x is None else x
    return (isinstance(x, torch.Tensor) and m.epilogue_fusable(x)
            and fusable_act_quantizer(q, True) is not None)


def readers_refuse(q, readers, source, around, watched):
    """Why `readers` do not take a tensor quantized by `q` as codes, None when they do:
    "grouped", a grouped or depthwise conv of `around` left on the decoded path; "readers", none,
    or one not planned or whose traced input (`source`) is not `q`'s output; "hook", a forward
    hook on one of `watched` that would see the tensor."""
    if any(isinstance(m, QuantModule) and m.fwd_kwargs.get("groups", 1) != 1 and m._int_plan is None
           for a in around for m in a.modules()):
        return "grouped"
    if not readers or any(m._int_plan is None or source.get(m) is not q for m in readers):
        return "readers"
    return "hook" if _hooked(*watched) else None


class Edge:
    """One carried tensor of the installed plan: `readers`, the QuantModules whose planned
    operand the codes are; `grid`, the act quantizer the codes lie on, as the readers' plans
    hold it; `pools`, the marked pool modules the codes pass; `at`, the module the reports name
    the edge by.  `marks`: the (object, attribute) pairs that hold the edge while it is
    installed, where the forwards find it.  Counters: `calls`, the emitting forwards (a
    HeadEdge's: the fc's), and `pooled`, per pool the forwards that pooled codes."""
    emitter = None      # the edge a HeadEdge owns: its producer's TailEdge / PairEdge

    def __init__(self, at, readers, watched, marks, pools=()):
        self.at, self.readers, self.pools = at, list(readers), list(pools)
        self.grid = self.readers[0]._int_plan.grid
        self._watched, self._marks = list(dict.fromkeys(watched)), list(marks)
        self.reset()

    def watched(self):
        """Exactly the modules whose run-time state `live` inspects."""
        return self._watched

    def live(self):
        """The run-time state is still the planned one: no grad, no cached convs, no hook that
        would see the tensor, no feature caching, weight and act quantization on, the readers
        still planned and every mark still this edge."""
        if torch.is_grad_enabled() or L._CONV_CACHE is not None:
            return False
        for m in self._watched:
            if (m._forward_hooks or m._forward_pre_hooks
                    or getattr(m, 'cache_features', 'none') != 'none'
                    or not (getattr(m, 'use_weight_quant', True) and getattr(m, 'use_act_quant', True))):
                return False
        for m in self.readers:
            if m._int_plan is None:
                return False
        for o, a in self._marks:
            if getattr(o, a) is not self:
                return False
        return True

    def reset(self):
        self.calls = 0
        self.pooled = {m: 0 for m in self.pools}
        if self.emitter is not None:
            self.emitter.reset()

    def install(self, on=True):
        for o, a in self._marks:
            setattr(o, a, self if on else None)
        if self.emitter is not None:
            self.emitter.install(on)


class PairEdge(Edge):
    """A layer that emits with its own act quantizer for one reader: a block's interior pair
    (carry), or the trailing layer in front of a carried head."""

    def __init__(self, producer, consumer):
        super().__init__(producer, [consumer], [producer, consumer], [(producer._int_plan, "carry")])

    def emit(self, x):
        """K.qconv_codes: conv, epilogue and act quantizer in one kernel."""
        m = self.at
        plan = m._int_plan
        if not (self.live() and can_emit(m, m.act_quantizer, True, x) and plan.takes(x)):
            return None
        gamma, phi = m.affine()
        return plan.run_codes(x, m.bias, gamma, phi, m.act_code(), self)


class TailEdge(Edge):
    """A block's carried output (carry_blocks): the block's last conv emits for the successor's
    readers behind its `entry`; `residual`: the kind the last emitting forward added."""

    def __init__(self, block, last, successor, entry, readers):
        super().__init__(block, readers, [block, successor, last, entry, *readers],
                         [(block, "_int_tail")])
        self.last, self.successor, self.entry = last, successor, entry

    def reset(self):
        super().reset()
        self.residual = None

    def emit(self, last, x, residual):
        """K.qconv_codes with the residual: conv, bias, gamma^z / phi^z, residual add, block
        activation and block act quantizer in one kernel."""
        blk, plan = self.at, last._int_plan
        relu = act_code(blk.activation_function)
        if (last is not self.last or plan is None or relu is None or not self.live()
                or not can_emit(last, blk.act_quantizer, False, x) or not plan.takes(x)):
            return None
        if residual is None:
            kind = "none"
        elif not isinstance(residual, torch.Tensor):
            return None
        elif getattr(residual, '_ssq_codes', None) is not None:
            kind = "codes"
        elif residual.dtype == torch.float32 and residual.is_cuda:
            kind = "fp32"
        else:
            return None
        gamma, phi = last.affine()
        out = plan.run_codes(x, last.bias, gamma, phi, relu, self, residual=residual)
        self.residual = kind
        return out


class StemEdge(Edge):
    """The stem's carried output (carry_stem): the producing conv stays on the fp32 route (its
    input is an unquantized image), its epilogue emits, the pools pool the codes (a max-pool
    commutes with the decode, which is non-decreasing in the code) and the successor's readers
    behind its `entry` take them."""

    def __init__(self, producer, pools, successor, entry, readers):
        super().__init__(producer, readers, [producer, successor, *pools, entry, *readers],
                         [(m, "_int_stem") for m in (producer, *pools)], pools)
        self.successor, self.entry = successor, entry
        self.counter = readers[0]._int_plan.counter

    def live(self):
        return super().live() and all(m._plan() is not None for m in self.pools)

    def emit(self, x):
        """The conv on its fp32 route, then K.epilogue_codes."""
        m = self.at
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 4
                and self.live() and can_emit(m, m.act_quantizer, True, x)):
            return None
        out, bias = m.forward_raw(x)
        gamma, phi = m.affine()
        self.calls += 1
        codes = K.epilogue_codes(out, bias, gamma, phi, m.act_code(), *self.grid, self.counter)
        return K.carried(codes, tuple(out.shape), *self.grid)

    # fused_stem: `fuse` replaces `emit` on this instance; an edge planned without it has neither
    # attribute below and runs the method above
    def fuse(self, blob, stride, padding):
        """From now on the conv itself emits (K31) wherever `stem_fused_takes` lets it."""
        self.blob, self.stride, self.padding = blob, stride, padding
        self.fused, self.unfused = 0, {}
        self.emit = self.emit_fused

    def emit_fused(self, x):
        """K.stem_conv_codes: conv, epilogue and act quantizer in one kernel; an input or a
        shape K31 is not to take goes the K27 way, counted by reason."""
        m = self.at
        why = None
        if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.is_cuda):
            why = "input is not a 4-D device tensor"
        elif x.dtype != torch.float32 or not x.is_contiguous():
            why = "non-contiguous / non-fp32 input"
        elif not stem_fused_takes(self.blob.shape, x.shape, self.stride, self.padding):
            why = "shape rule: K27 is faster here (SSQ_STEM_FUSED=1 overrides)"
        if why is None and not (self.live() and can_emit(m, m.act_quantizer, True, x)):
            return None
        if why is not None:
            self.unfused[why] = self.unfused.get(why, 0) + 1
            return StemEdge.emit(self, x)
        gamma, phi = m.affine()
        self.calls += 1
        self.fused += 1
        codes = K.stem_conv_codes(x, self.blob, m.bias, gamma, phi, m.act_code(), *self.grid,
                                  self.counter, stride=self.stride, padding=self.padding)
        N, H, W, _ = codes.shape
        return K.carried(codes, (N, self.blob.shape[0], H, W), *self.grid)

    # image_u8: `take_u8` puts `emit_u8` in front of whichever emit the edge has; an edge planned
    # without it has none of the attributes below
    def take_u8(self, norm, why, prepared=None, tables=None, stride=None, padding=None):
        """From now on a uint8 image goes to K32 wherever `stem_u8_takes` lets it; `why`: what
        keeps this edge's conv off K32 altogether (`u8_stem_reason`), its uint8 batches are then
        normalised (`norm`: mean, std as (1, Ci, 1, 1) device tensors) for the fp32 emit."""
        self.u8_norm, self.u8_why = norm, why
        self.u8_blob, self.u8_tables, self.u8_geo = prepared, tables, (stride, padding)
        self.u8, self.un_u8 = 0, ({} if why is None else {why: 0})
        self.u8_form = {}               # {staging form: forwards on K32} (K.stem_u8_view_form)
        self._emit_f32, self._u8_declined = self.emit, False
        self.emit = self.emit_u8

    def emit_u8(self, x):
        """K.stem_conv_u8_codes on a uint8 image: conv, epilogue and act quantizer in one kernel on
        the int8 MFMA; an fp32 input takes the edge's fp32 emit untouched, a uint8 input K32 is
        not to take is normalised on the device and takes it too, counted by reason.  A view that is
        not dense NCHW (an HWC batch as `hwc.permute(0, 3, 1, 2)`, an RGBA batch's first three
        channels, a crop of a larger frame) is read in place where `stem_u8_takes` lets its staging
        form, copied dense for K32 under SSQ_STEM_U8_STRIDED=0, and otherwise normalised as before;
        the K32 forwards are counted by form (`u8_form`)."""
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.uint8):
            # the normalised batch of the branch below, back through the module's forward: its
            # fp32 emit has already declined it
            return None if self._u8_declined else self._emit_f32(x)
        m = self.at
        why = self.u8_why
        if why is None:
            if not (x.dim() == 4 and x.is_cuda):
                why = U8_NOT_4D
            else:
                takes = stem_u8_takes(self.u8_blob.shape, x.shape, *self.u8_geo)
                # a view reaches K32 only where K32 takes the shape at all: elsewhere it keeps the
                # reason it had
                form = "planar" if x.is_contiguous() else None
                if form is None and takes:
                    form = stem_u8_view_route(K.stem_u8_view_form(x), self.u8_blob.shape, x.shape,
                                              *self.u8_geo)
                if form is None:
                    why = (U8_NHWC if x.is_contiguous(memory_format=torch.channels_last)
                           else U8_STRIDED)
                elif not takes:
                    why = U8_SHAPE_RULE
                elif not (self.live() and can_emit(m, m.act_quantizer, True, x)):
                    why = U8_NOT_LIVE
        if why is not None:
            self.un_u8[why] = self.un_u8.get(why, 0) + 1
            # contiguous first (a quarter of the fp32 copy's bytes): the fp32 emit's own rules then
            # see the layout K31 takes
            xf = normalise_u8(x.contiguous(), *self.u8_norm)
            out = self._emit_f32(xf)
            if out is not None:
                return out
            self._u8_declined = True        # the fp32 emit is asked once per forward
            try:
                return m.forward(xf)
            finally:
                self._u8_declined = False
        gamma, phi = m.affine()
        self.calls += 1
        self.u8 += 1
        if form == "copied":
            x = x.contiguous()
        self.u8_form[form] = self.u8_form.get(form, 0) + 1
        stride, padding = self.u8_geo
        codes = K.stem_conv_u8_codes(x, self.u8_blob, *self.u8_tables, m.bias, gamma, phi,
                                     m.act_code(), *self.grid, self.counter, stride=stride,
                                     padding=padding)
        N, H, W, _ = codes.shape
        return K.carried(codes, (N, self.u8_blob.shape[0], H, W), *self.grid)

    def reset(self):
        super().reset()
        if "fused" in self.__dict__:
            self.fused, self.unfused = 0, {}
        if "u8" in self.__dict__:
            self.u8, self.un_u8 = 0, ({} if self.u8_why is None else {self.u8_why: 0})
            self.u8_form = {}


# what keeps one uint8 forward of an edge that takes K32 off it (`un_u8`'s per-forward reasons)
U8_NOT_4D = "input is not a 4-D device tensor"
U8_NHWC, U8_STRIDED = "channels-last input", "non-contiguous input"
U8_SHAPE_RULE = "shape rule: K31 is faster here (SSQ_STEM_U8=1 overrides)"
U8_NOT_LIVE = "the stem edge does not carry in this state"
U8_FORWARD_REASONS = (U8_NOT_4D, U8_NHWC, U8_STRIDED, U8_SHAPE_RULE, U8_NOT_LIVE)
# how a K32 forward staged its image (`u8_form`): K.stem_u8_view_form's
U8_FORMS = ("planar", "interleaved", "generic", "copied")


def normalise_u8(u, mean, std):
    """The loader's normalisation of a uint8 image batch as three torch operations:
    (u.float() / 255 - mean) / std."""
    return (u.float() / 255 - mean) / std


def u8_stem_reason(m, fields=None):
    """Why K32 cannot run QuantModule `m`'s conv on a uint8 image, None when it can: an ungrouped
    F.conv2d inside ssq_stem_conv_u8_fwd's geometry (K.stem_u8_geometry_reason), no forward hook
    on it, and -- `fields`, the hard weight's dequant fields -- a weight without a column scale
    whose zero points are integer codes."""
    if m.fwd_func is not F.conv2d:
        return "not a conv"
    kw = m.fwd_kwargs
    if isinstance(kw.get("padding", 0), str):
        return "padding given as a string"
    Co, Ci, R, S = (int(v) for v in m.weight.shape)
    why = K.stem_u8_geometry_reason(Co, Ci, R, S, kw.get("stride", 1), kw.get("padding", 0),
                                    kw.get("dilation", 1), int(kw.get("groups", 1)))
    if why is not None:
        return why
    if _hooked(m):
        return "a forward hook on the producer"
    if fields is not None:
        if fields["col_scale"] is not None:
            return (f"weight has a column scale ({fields['kind']}): (q - z) * k leaves int8 at 8 "
                    "bits and would need the two-digit operand")
        zp, qmin = fields["zero_point"].detach().float().reshape(-1), int(fields["qmin"])
        if not bool(((zp == zp.round()) & (zp >= qmin - 256) & (zp <= qmin + 511)).all()):
            return "weight zero point is not an integer code"
    return None


def stem_u8_takes(wshape, xshape, stride, padding, form=None):
    """The host shape rule of a uint8 stem edge ("uint8 stem (K32)"): K32 takes a shape
    class only where its measured median saving over K31 fed the normalised image exceeded that
    baseline's min-max spread (profiles/int_infer_u8_stem_rate.txt); elsewhere the batch is
    normalised on the device and takes K31.  Measured at batch 64: the 7x7/2 stem on a 32 x 32
    image clears it (36.8 -> 34.3 us, spread 0.1), on a 224 x 224 image it does not (280.4 ->
    283.3), nor does the 3x3/2 stem there (62.3 -> 129.0: nine of the k step's 64 taps are
    real).  So auto takes K32 for the measured class, a 7x7 kernel at stride 2 on at most
    64 x 16 x 16 output pixels, and nothing else; a smaller batch of that class is taken by
    extrapolation (fewer pixels are more launch-bound, not measured).  SSQ_STEM_U8=1 / 0 forces
    K32 / the normalised route for an A/B run; auto (the default) asks the rule.

    `form` (None: the question above, of a dense NCHW batch): whether K32 reads a view of that
    staging form ("planar", "interleaved", "generic": K.stem_u8_view_form) in place instead of a
    dense copy of it ("uint8 stem (K32)", Strided views).  The same keep rule against the
    copy route, torch's .contiguous() followed by the dense launch
    (profiles/int_infer_u8_layout_rate.txt): a form is taken for a shape class where its median
    beat the copy route's by more than that route's min-max spread, `U8_VIEW_CLASSES`; an
    unmeasured class is not taken.  Measured at batch 64 on 224 x 224: the 7x7/2 stem saves
    17.0 us on 3-byte pixels (303.2 -> 286.2, spread 0.3), 7.0 on 4-byte pixels (303.3 -> 296.3,
    0.9), 18.1 on a planar 256 -> 224 crop (304.1 -> 286.0, 0.5) and 13.9 on an interleaved one;
    the 3x3/2 stem 16.5, 10.8, 18.2 and 14.1 (spreads <= 0.4).  So auto takes the planar and the
    interleaved form for these two classes from that many image pixels up; the generic form and
    smaller batches were not measured.  SSQ_STEM_U8_STRIDED=1 / 0 forces the view / the copy; auto
    asks the rule."""
    if form is not None:
        knob = os.environ.get("SSQ_STEM_U8_STRIDED", "auto")
        if knob in ("0", "1"):
            return knob == "1" and form in U8_FORMS[:3]
        (_, _, R, S), (N, _, H, W), (sh, sw) = wshape, xshape, stride
        return any(tuple(c) == (form, R, S, sh, sw) and int(N) * int(H) * int(W) >= px
                   for *c, px in U8_VIEW_CLASSES)
    knob = os.environ.get("SSQ_STEM_U8", "auto")
    if knob in ("0", "1"):
        return knob == "1"
    (_, _, R, S), (N, _, H, W), (sh, sw), (ph, pw) = wshape, xshape, stride, padding
    pixels = int(N) * ((int(H) + 2 * ph - R) // sh + 1) * ((int(W) + 2 * pw - S) // sw + 1)
    return (R, S, sh, sw) == (7, 7, 2, 2) and pixels <= 64 * 16 * 16


# (form, R, S, stride h, stride w, the fewest image pixels N * H * W measured): the classes whose
# in-place form cleared the keep rule against the copy route at batch 64 on 224 x 224
# (profiles/int_infer_u8_layout_rate.txt).  A smaller batch was not measured and is not taken.
U8_VIEW_CLASSES = (("planar", 7, 7, 2, 2, 64 * 224 * 224), ("interleaved", 7, 7, 2, 2, 64 * 224 * 224),
                   ("planar", 3, 3, 2, 2, 64 * 224 * 224), ("interleaved", 3, 3, 2, 2, 64 * 224 * 224))


def stem_u8_view_route(form, wshape, xshape, stride, padding):
    """How a uint8 view that is not dense NCHW reaches K32: `form` itself (read in place), "copied"
    (made dense first: SSQ_STEM_U8_STRIDED=0, or a view the ABI refuses), or None: auto on a class
    `stem_u8_takes` does not take in place, whose batch is normalised for the fp32 emit as before
    strided views were read."""
    knob = os.environ.get("SSQ_STEM_U8_STRIDED", "auto")
    if form == "copied" or knob == "0":
        return "copied" if knob in ("0", "1") else None
    return form if stem_u8_takes(wshape, xshape, stride, padding, form) else None


def fused_stem_reason(m):
    """Why K31 cannot run QuantModule `m`'s conv, None when it can: an ungrouped F.conv2d inside
    ssq_stem_conv_fwd's geometry (K.stem_geometry_reason)."""
    if m.fwd_func is not F.conv2d:
        return "not a conv"
    kw = m.fwd_kwargs
    if isinstance(kw.get("padding", 0), str):
        return "geometry (padding given as a string)"
    Co, Ci, R, S = (int(v) for v in m.weight.shape)
    return K.stem_geometry_reason(Co, Ci, R, S, kw.get("stride", 1), kw.get("padding", 0),
                                  kw.get("dilation", 1), int(kw.get("groups", 1)))


def stem_fused_takes(wshape, xshape, stride, padding):
    """The host shape rule of a fused stem edge ("Fused stem (K31)"): K31 takes every
    shape class whose measured median saving over MIOpen + K27 exceeded that baseline's min-max
    spread (profiles/int_infer_fused_stem_rate.txt).  SSQ_STEM_FUSED=1 / 0 forces K31 / K27 for
    an A/B run; auto (the default) asks the rule."""
    knob = os.environ.get("SSQ_STEM_FUSED", "auto")
    if knob in ("0", "1"):
        return knob == "1"
    return True


class HeadEdge(Edge):
    """The carried head (carry_head): the pool sums the codes that `emitter`, the edge of the
    producer (the last quant block, or a trailing QuantModule), emits for it, and the fc reads
    the sums; named by the pool."""

    def __init__(self, producer, pool, fc, emitter):
        self.emitter = emitter
        super().__init__(pool, [fc], [pool, fc], [(pool, "_int_head"), (fc._int_plan, "head")], [pool])
        self.producer, self.fc = producer, fc
        self._scale_h = {}      # HW -> K.head_scale(plan.scale, HW)

    def accepts(self, pc):
        """A pooled digit tensor (K.PooledCodes) holds the fc's planned operand."""
        return (pc.quantizer() == self.grid and pc.shape[1] == self.fc._int_plan.prepared.shape[1]
                and 1 <= pc.HW <= K.HEAD_MAX_HW)

    def run(self, hi, pc):
        p, g = self.fc._int_plan, self.grid
        sh = self._scale_h.get(pc.HW)
        if sh is None:
            # a scaled fc: one division by fp32(L * HW), exact for L <= 1024, HW <= 126
            sh = self._scale_h[pc.HW] = (K.head_scale(p.scale, pc.HW) if p.head_grid is None else
                                         K.head_scale(p.head_grid[0], p.head_grid[1] * pc.HW))
        self.calls += 1
        p.calls += 1
        if p.head_grid is None:
            return K.qlinear_pooled(hi, pc.lo, pc.sp, p.prepared, sh, pc.HW, g.zp, g.n_bits, g.sym)
        return K.qlinear_pooled(hi, pc.lo, pc.sp, p.prepared, sh, pc.HW, g.zp, g.n_bits, g.sym,
                                wide_all=True)


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
    if isinstance(q, ChannelQuantAct) and q.opt_mode == "shiftFeature":
        # (the follow-up, DESIGN.md section 8: fold s[ci] into the consumer's per-ci grid, L = 2)
        return None, ("input is a per-channel shifted act quantizer (ChannelQuantAct "
                      "'shiftFeature'): the integer route does not cover shifted activations")
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
    return K.ActQuant(delta, zp, q.n_bits, q.sym), None


def _weight_codes(m, colscale=False, per_ci=False):
    """(packed codes, fields) of the module's hard weight: a restored model's PackedWeight as
    stored, a live quantizer through dequant_form + pack_encode (soft state is refused there).
    A column-scaled weight is encoded only with `colscale`, one scaled per (co, ci) only with
    `per_ci` (the caller refuses them otherwise)."""
    q = m.weight_quantizer
    if isinstance(q, PackedWeight):
        return q.packed, q.fields()
    what, f = dequant_form(m)
    if (f["per_ci"] and not per_ci) or (f["col_scale"] is not None and not colscale):
        return None, f
    packed, bad = K.pack_encode(what, f["zero_point"], f["scale"], f["per_ci"], f["col_scale"],
                                f["n_bits"], f["qmin"], f["qmax"])
    if bad:
        raise ValueError(f"{m.pathName or 'layer'}: {bad} weights are not integer codes of the "
                         f"{f['kind']} quantizer (soft state?)")
    return packed, f


@torch.no_grad()
def enable_integer_inference(qnn, sample, grouped=False, carry=False, carry_blocks=False,
                             carry_stem=False, carry_head=False, colscale=False, splitk=False,
                             per_ci=False, wide=False, fused_stem=False, image_u8=None,
                             wide_all=False):
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
    a plain weight and takes the plain route.  `splitk`: a dense layer asks the host rule
    K.qconv_splits on every forward and takes K23's split-K form where it returns Z > 1
    (bit-identical; `split_report`); off, no layer does.  `per_ci`: also plan weights whose scale
    is per (co, ci) (ChannelQuant's shifted scale) and lies on a grid base[co] * k / L
    (K.perci_grid), with (q - z) * k[co, ci] as the operand and
    scale[co] = fp32(fp32(delta_a * base[co]) / fp32(L)); off, they are reported as refused.  Every
    k equal to L is a plain weight.  `wide`: a scaled weight of either kind whose operand leaves
    int8 (|m| > 127, or a grid beyond 127) runs as two int8 digits, |m| <= 16319, L <= 1024, on
    K23's wide forms (dense layers only: never split along K, not the grouped kernels, not the
    pooled-operand fc); off, it is refused as leaving int8.  A weight with both a column scale and
    a per-(co, ci) scale is refused.  `wide_all` (with `wide`; nothing changes without it): the
    wide operand also on grouped convs (K26, two digit planes), on column-scaled depthwise convs
    (K25, its int32 blob with |m| <= 16319) and on the pooled-operand fc (K30), and a scaled fc is
    planned under `carry_head` at all -- on its centred int8 blob where (q - z) * k fits int8, on
    the dense wide blob beyond, with sh[co] = fp32(fp32(delta_a * base[co]) / fp32(L * HW)).
    SSQ_QCONV_WIDE=auto|1 governs these blobs as it does the dense one.
    `fused_stem`: on every stem edge that `carry_stem` (or `carry_head`) installs and whose producer is an ungrouped conv inside K31's geometry
    (`fused_stem_reason`), the conv itself emits the codes (K.stem_conv_codes, a weight blob
    prepared here from the producer's hard weight) instead of the fp32 conv + K27; it plans no
    edge of its own, and `stem_carry_report` then also counts the fused forwards and names what
    kept an edge or a forward on K27.  The stem's fp32 values are K31's fma chain, not the
    library conv's: the logits are those of the `carry_stem` route up to that summation order.
    `image_u8` = (mean, std), the loader's per-channel normalisation: a forward whose input is a
    uint8 image batch (N, Ci, H, W; x = (u/255 - mean)/std) runs the stem conv on the int8 MFMA
    (K32, K.stem_conv_u8_codes; DESIGN 4 "uint8 stem (K32)") on every stem edge whose producer
    passes `u8_stem_reason`, its blob and tables prepared here.  It plans no edge of its own and
    needs `carry_stem` and an installed stem edge (ValueError without either, the plan removed); it is independent of `fused_stem`.  An fp32 input
    takes exactly the path it takes without the keyword; a uint8 input K32 does not take is
    normalised on the device and takes that path too.  `stem_carry_report` then also counts the
    K32 forwards ("u8") and the normalised ones by reason ("un_u8").  The stem codes of a uint8
    forward are K32's own contract's, not pinned to the fp32 routes'; `sample` may be uint8."""
    carry_stem = carry_stem or carry_head
    wide_all = bool(wide and wide_all)
    if image_u8 is not None:
        if not carry_stem:
            raise ValueError("enable_integer_inference: image_u8 needs a stem edge (carry_stem or "
                             "carry_head)")
        if isinstance(sample, torch.Tensor) and sample.dtype == torch.uint8:
            sample = normalise_u8(sample, *_u8_norm(image_u8, sample.shape[1], sample.device))
    carry_blocks = carry_blocks or carry_stem
    carry = carry or carry_blocks
    disable_integer_inference(qnn)
    layers = _layers(qnn)
    if not layers:
        return {}
    qnn._int_edges = []
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
            packed, f = _weight_codes(m, colscale, per_ci)
        except TypeError as e:
            report[name] = str(e)
            continue
        if f["per_ci"] and not per_ci:
            report[name] = f"weight scale is per (co, ci) ({f['kind']})"
            continue
        if f["per_ci"] and f["col_scale"] is not None:
            report[name] = f"weight has both a column scale and a per-(co, ci) scale ({f['kind']})"
            continue
        kcol, kfac, L, d1 = None, None, 1, f["scale"]
        max_l = K.QWIDE_MAX_L if wide else K.COLSCALE_MAX_L
        if f["per_ci"]:
            Co, Cig = int(m.weight.shape[0]), int(m.weight.shape[1])
            grid = K.perci_grid(f["scale"], Co, Cig)
            if grid is None and wide:
                grid = K.perci_grid(f["scale"], Co, Cig, K.QWIDE_MAX)
            if grid is None:
                report[name] = (f"weight scale is per (co, ci) ({f['kind']}) and not on an integer "
                                f"grid base[co] * k / L, L <= {max_l}")
                continue
            L, d1, kfac = grid
            d1 = d1.to(dev)
            if K.perci_plain(grid):
                kfac, L = None, 1               # every k = L: a plain weight with scale = base
        elif f["col_scale"] is not None:
            grid = K.colscale_grid(f["col_scale"]) if colscale else None
            if grid is None and colscale and wide:
                grid = K.colscale_grid(f["col_scale"], K.QWIDE_MAX_L, K.QWIDE_MAX)
            if grid is None:
                report[name] = f"weight has a column scale ({f['kind']})" + (
                    f" that is not on an integer grid k / L, L <= {max_l}" if colscale else "")
                continue
            L, kcol = grid
            if L == 1 and int(kcol.max()) == 1:
                kcol = None                     # all ones: a plain weight, the plain K22 blob
        scaled = kcol is not None or kfac is not None
        if scaled and m in head_fc and not wide_all:
            report[name] = ((f"weight has a column scale ({f['kind']})" if kcol is not None else
                             f"weight scale is per (co, ci) ({f['kind']})")
                            + ": the pooled-operand fc takes plain weights only")
            continue
        if not scaled:
            prep = K.qweight_prepare(packed, tuple(m.weight.shape), f["zero_point"], f["n_bits"],
                                     f["qmin"], groups=groups)
        else:
            prep = K.qweight_prepare_scaled(packed, tuple(m.weight.shape), f["zero_point"],
                                            f["n_bits"], f["qmin"], groups=groups, kcol=kcol,
                                            kfac=kfac, wide=wide, wide_all=wide_all)
        if prep is None:
            report[name] = ("scaled weight's grid leaves int8 (k > 127): the wide operand is dense "
                            "only, the grouped kernels (K26) read int8")
            continue
        if int(prep.bad.item()):
            report[name] = ("weight zero point is not an integer code" if not scaled else
                            "scaled weight (q - z) * k leaves the wide operand (|m| > 16319), or a "
                            "zero point is not an integer code" if prep.wide else
                            "scaled weight (q - z) * k leaves int8 (|m| > 127), or a zero point "
                            "is not an integer code")
            if scaled and wide and groups != 1 and not wide_all:
                report[name] += "; the wide operand is dense only, the grouped kernels (K26) read int8"
            continue
        # s[co] = fp32(delta_a * d1[co]): one fp32 product of the two stored fp32 values (per
        # (co, ci): of delta_a and the grid's base[co])
        scale = (torch.full((1,), act.delta, dtype=torch.float32, device=dev)
                 * d1.detach().reshape(-1).float()).contiguous()
        scale0 = scale
        if scaled:
            # ... / fp32(L): the grid's common denominator, one more rounding
            scale = (scale / torch.full((1,), float(L), dtype=torch.float32, device=dev)).contiguous()
        m._int_plan = IntPlan(prep, scale, act, stride, padding, counter)
        if scaled and m in head_fc:
            m._int_plan.head_grid = (scale0, int(L))
        # a wide layer is never asked to split: K23's split form holds one accumulator set
        m._int_plan.splitk = bool(splitk) and m._int_plan.kind == "dense" and not prep.wide
        report[name] = INT8
    if carry:
        _plan_carry(qnn, source)
    if carry_blocks:
        _plan_block_carry(qnn, source)
    if carry_stem:
        _plan_stem_carry(qnn, source)
    if fused_stem:
        _fuse_stems(qnn)
    if image_u8 is not None:
        _u8_stems(qnn, image_u8)
    if carry_head:
        _plan_head_carry(qnn, source, heads, report, sample)
    order = {m: i for i, m in enumerate(qnn.modules())}
    qnn._int_edges.sort(key=lambda e: order[e.at])      # the reports list them in module order
    return report


def _install(qnn, edge):
    edge.install()
    qnn._int_edges.append(edge)
    return edge


def _edges(qnn, kind):
    return [e for e in getattr(qnn, "_int_edges", ()) if type(e) is kind]


def _plan_carry(qnn, source):
    """A PairEdge on every producer of a block's interior chain whose pair can stay int8."""
    for blk in qnn.modules():
        for prod, cons in blk.interior_chain() if isinstance(blk, BaseQuantBlock) else ():
            q = prod.act_quantizer
            if (prod._int_plan is not None and can_emit(prod, q, True)
                    and readers_refuse(q, [cons], source, (), (prod, cons)) is None):
                _install(qnn, PairEdge(prod, cons))


def _edge_entry(m):
    """The module a successor hands its input to and to nothing else: a quant block or a
    QuantModule itself, the first child (recursively) of an nn.Sequential; None otherwise."""
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


def edge_readers(successor):
    """(entry module, the QuantModules that read the successor's input, whether the input is
    also an identity residual); readers None when the input has a reader that is not known."""
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


def _emitting_tail(blk):
    """The block's last conv when its tail can emit codes onto the block's act quantizer: a
    planned dense conv under `can_emit`, the block's activation one the kernel applies."""
    last = blk.last_conv()
    plan = None if last is None else last._int_plan
    if plan is None or plan.kind != "dense" or act_code(blk.activation_function) is None:
        return None
    return last if can_emit(last, blk.act_quantizer, False) else None


def _plan_block_carry(qnn, source):
    """A TailEdge on every block of `block_edges` whose tail can emit and whose successor's
    readers take the codes.  No grouped or depthwise conv of either side may be left on the
    decoded path: without `grouped=True` a MobileNetV2 / RegNetX block has one in its middle,
    and such a block keeps its fp32 edges."""
    for blk, succ in block_edges(qnn):
        last = _emitting_tail(blk)
        entry, readers, _ = edge_readers(succ)
        if last is not None and readers_refuse(blk.act_quantizer, readers, source, (blk, entry),
                                               (blk, last, succ, entry, *(readers or ()))) is None:
            _install(qnn, TailEdge(blk, last, succ, entry, readers))


def stem_edges(qnn):
    """The (producer QuantModule, [max-pools], successor) chains from the stem conv to the first
    stage, from the structure alone (no device, no forward): the `stem_chain()` the model
    declares on `qnn.model`, whose first entry is a QuantModule -- itself, or an nn.Sequential
    of one followed by StraightThrough only --, whose entries in between are StraightThrough or
    a max-pool the code kernel can run (SsqMaxPool2d with a plan), and whose last entry has an
    `_edge_entry`.  Empty for any other chain and for a model that declares none."""
    ident = (FoldedBN, StraightThrough)     # a folded BN's and a moved activation's identity
    chain = getattr(getattr(qnn, "model", qnn), "stem_chain", None)
    mods = list(chain()) if callable(chain) else []
    if len(mods) < 2:
        return []
    prod = mods[0]
    if isinstance(prod, nn.Sequential):
        kids = list(prod)
        if not kids or not all(isinstance(k, ident) for k in kids[1:]):
            return []
        prod = kids[0]
    if not isinstance(prod, QuantModule):
        return []
    pools = []
    for m in mods[1:-1]:
        if isinstance(m, K.SsqMaxPool2d) and m._plan() is not None:
            pools.append(m)
        elif not isinstance(m, ident):
            return []
    if _edge_entry(mods[-1]) is None:
        return []
    return [(prod, pools, mods[-1])]


def _plan_stem_carry(qnn, source):
    """A StemEdge on the producer of every `stem_edges` chain: a conv on the fp32 route that can
    emit and whose successor's readers take the codes (their traced input is the producer's act
    quantizer through the pools), with no grouped or depthwise conv of the entry left on the
    decoded path."""
    for prod, pools, succ in stem_edges(qnn):
        q = prod.act_quantizer
        entry, readers, _ = edge_readers(succ)
        if (prod._int_plan is None and can_emit(prod, q, True)
                and readers_refuse(q, readers, source, (entry,),
                                   (prod, succ, entry, *pools, *(readers or ()))) is None):
            _install(qnn, StemEdge(prod, pools, succ, entry, readers))


def _fuse_stems(qnn):
    """fused_stem: every installed StemEdge whose producer K31 can run gets its weight blob and
    emits through K.stem_conv_codes; `qnn._int_fused_stem`: {producer name: why not, or None}."""
    names = {m: n for n, m in qnn.named_modules()}
    qnn._int_fused_stem = {}
    for e in _edges(qnn, StemEdge):
        m = e.at
        why = fused_stem_reason(m)
        if why is None:
            kw = m.fwd_kwargs
            e.fuse(K.stem_weight_prepare(m._weight_bias()[0]), tuple(kw["stride"]),
                   tuple(kw["padding"]))
        qnn._int_fused_stem[names[m]] = why


def _u8_norm(image_u8, Ci, dev):
    """(mean, std) of `image_u8` as fp32 (1, Ci, 1, 1) tensors on `dev`."""
    mean, std = (torch.as_tensor(v, dtype=torch.float32).detach().reshape(-1).to(dev)
                 for v in image_u8)
    if mean.numel() != Ci or std.numel() != Ci:
        raise ValueError(f"image_u8: mean and std must have one entry per input channel ({Ci})")
    return mean.reshape(1, Ci, 1, 1), std.reshape(1, Ci, 1, 1)


def _u8_stems(qnn, image_u8):
    """image_u8: every installed StemEdge takes uint8 images from now on -- on K32 where its
    producer passes `u8_stem_reason` (the blob from the hard weight's packed codes, the tables from
    its scale and the caller's mean / std), normalised for its fp32 emit elsewhere;
    `qnn._int_u8`: {producer name: why not, or None}."""
    names = {m: n for n, m in qnn.named_modules()}
    stems = _edges(qnn, StemEdge)
    if not stems:
        disable_integer_inference(qnn)
        raise ValueError("enable_integer_inference: image_u8 found no stem edge installed on this "
                         "model (no stem_chain, a stem that cannot emit, or readers that refuse the "
                         "codes): a uint8 batch would have no route")
    qnn._int_u8 = {}
    for e in stems:
        m = e.at
        Co, Ci = int(m.weight.shape[0]), int(m.weight.shape[1])
        norm = _u8_norm(image_u8, Ci, m.weight.device)
        why = u8_stem_reason(m)
        prep = tables = None
        if why is None:
            try:
                packed, f = _weight_codes(m, per_ci=True)
                why = u8_stem_reason(m, f)
            except (TypeError, ValueError) as err:
                why = str(err)
        if why is None:
            prep = K.stem_u8_weight_prepare(packed, tuple(m.weight.shape), f["zero_point"],
                                            f["n_bits"], f["qmin"])
            if int(prep.bad.item()):
                why = "weight zero point is not an integer code"
        if why is None:
            tables = K.stem_u8_tables(norm[0], norm[1], f["scale"].to(m.weight.device), Co, Ci)
            kw = m.fwd_kwargs
            e.take_u8(norm, None, prep, tables, tuple(K._pair(kw.get("stride", 1))),
                      tuple(K._pair(kw.get("padding", 0))))
        else:
            e.take_u8(norm, why)
        qnn._int_u8[names[m]] = why


def head_edges(qnn):
    """The (producer, pool, fc) chains of the pooling head, from the structure alone (no device,
    no forward): the `head_chain()` the model declares on `qnn.model`, [last stage, pool,
    classifier].  The producer is the stage's last child when that is a quant block, or -- an
    nn.Sequential there -- a trailing QuantModule followed by StraightThrough only (MobileNetV2's
    `features.18`); the pool is a K.SsqGlobalAvgPool; the classifier a Linear QuantModule, or an
    nn.Sequential that ends in one behind nn.Dropout / nn.Flatten / identities only.  Empty for
    any other chain and for a model that declares none."""
    ident = (FoldedBN, StraightThrough, nn.Identity)
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


def _plans(qnn):
    return [(n, m._int_plan) for n, m in _layers(qnn) if getattr(m, "_int_plan", None) is not None]


def _reset_calls(qnn):
    """Zero every forward counter of the installed plan (after the head's dry forward)."""
    for _, p in _plans(qnn):
        p.calls = 0
    for e in qnn._int_edges:
        e.reset()
    qnn._int_counter.zero_()


HEAD_REFUSALS = {"grouped": "the last block holds a grouped conv on the decoded path",
                 "readers": "the pool's input is not the last block's act quantizer output",
                 "hook": "a forward hook on the last block, the pool or the fc"}


def _plan_head_carry(qnn, source, heads, report, sample):
    """A HeadEdge on every `head_edges` chain whose producer can emit codes for the pool -- a
    quant block's tail (a carried block input is then the RES = 2 residual) or a trailing
    QuantModule, not already emitting for another edge -- whose fc takes them through the pool,
    and whose dry forward of `sample` under the installed plan shows the pooled digits arriving
    at the fc.  An fc whose edge is not installed loses its plan -- it is planned for pooled
    digits only -- and is reported with the reason."""
    names = {m: n for n, m in qnn.named_modules()}
    for prod, pool, fc in heads:
        if fc._int_plan is None:
            continue        # refused by the weight / input rules: the report says why
        q, why = prod.act_quantizer, None
        if isinstance(prod, BaseQuantBlock):
            last = _emitting_tail(prod)
            if last is None:
                why = "the last block's tail cannot emit codes"
            elif prod._int_tail is not None:
                why = "the last block already emits codes for another edge"
            watched = (prod, pool, fc, last)
        else:
            if prod._int_plan is None or not can_emit(prod, q, True) or prod._int_plan.carry is not None:
                why = "the last layer cannot emit codes"
            watched = (prod, pool, fc)
        if why is None:
            why = HEAD_REFUSALS.get(readers_refuse(q, [fc], source, (prod,), watched))
        if why is None:
            emitter = (TailEdge(prod, last, pool, fc, [fc]) if isinstance(prod, BaseQuantBlock)
                       else PairEdge(prod, fc))
            head = _install(qnn, HeadEdge(prod, pool, fc, emitter))
            try:
                qnn(sample)
            except K.A.SSQError as e:
                why = f"the dry forward failed: {e}"
            else:
                if not head.calls:
                    why = "the dry forward did not bring pooled codes to the fc"
            _reset_calls(qnn)
            if why is not None:
                head.install(False)
                qnn._int_edges.remove(head)
        if why is not None:
            fc._int_plan = None
            report[names[fc]] = f"no head edge: {why}"


def disable_integer_inference(qnn):
    """Every layer back on the decoded fp32 path."""
    for e in getattr(qnn, "_int_edges", ()):
        e.install(False)
    for _, m in _layers(qnn):
        m._int_plan = None
    qnn._int_edges, qnn._int_counter = [], None
    qnn._int_fused_stem = None
    qnn._int_u8 = None
    # every enable passes here: a captured forward (IntegerGraph) of the previous plan is stale
    qnn._int_epoch = getattr(qnn, "_int_epoch", 0) + 1


def integer_report(qnn):
    """{"off_grid": elements seen by the integer layers that were not on their act quantizer's
    grid (0 = every integer layer computed what the decoded path computes up to fp32
    rounding), "calls": {layer name: forwards taken on the integer route}}.  Reads one device
    word (the only sync of the integer path).  Under a plan installed with `image_u8`, also
    "u8_form": {producer name: {staging form: forwards of a uint8 batch on K32}}, the forms
    K.stem_u8_view_form's: "planar", "interleaved", "generic" read in place, "copied" made dense
    first; they sum to stem_carry_report's "u8"."""
    counter = getattr(qnn, "_int_counter", None)
    rep = {"off_grid": int(counter.item()) if counter is not None else 0,
           "calls": {n: p.calls for n, p in _plans(qnn)}}
    if getattr(qnn, "_int_u8", None) is not None:
        names = {m: n for n, m in qnn.named_modules()}
        rep["u8_form"] = {names[e.at]: dict(e.u8_form) for e in _edges(qnn, StemEdge)}
    return rep


def split_report(qnn):
    """{layer name: the Z of its last forward} for the dense layers planned with `splitk` that
    have run (1: the one-kernel form); empty without `splitk`."""
    return {n: p.splits for n, p in _plans(qnn) if p.splitk and p.splits is not None}


def carry_report(qnn):
    """{"pairs": [(producer name, consumer name), ...] the installed plan carries int8 codes
    between, "calls": {producer name: forwards that emitted codes}}; empty without a plan."""
    names = {m: n for n, m in qnn.named_modules()}
    pairs = _edges(qnn, PairEdge)
    return {"pairs": [(names[e.at], names[e.readers[0]]) for e in pairs],
            "calls": {names[e.at]: e.calls for e in pairs}}


def block_carry_report(qnn):
    """{"edges": [(block name, successor name), ...] whose block tail the installed plan lets
    emit int8 codes, "calls": {block name: forwards whose tail emitted codes}, "residual":
    {block name: "none" | "fp32" | "codes", the residual operand of the emitting tail: as the
    last emitting forward had it, before one as the plan expects it}}; empty without a plan."""
    names = {m: n for n, m in qnn.named_modules()}
    tails = _edges(qnn, TailEdge)
    fed = {e.entry for e in tails + _edges(qnn, StemEdge)}
    residual = {}
    for e in tails:
        kind, blk = e.residual, e.at
        if kind is None and blk.identity_input_convs() is not None:
            kind = "codes" if blk in fed else "fp32"
        elif kind is None:
            kind = "none" if getattr(blk, "downsample", None) is None else "fp32"
        residual[names[blk]] = kind
    return {"edges": [(names[e.at], names[e.successor]) for e in tails],
            "calls": {names[e.at]: e.calls for e in tails}, "residual": residual}


def stem_carry_report(qnn):
    """{"edges": [(producer name, [pool names], successor name), ...] whose producer the
    installed plan lets emit int8 codes, "calls": {producer name: forwards that emitted codes},
    "pooled": {pool name: forwards that pooled codes}}; empty without a plan.  Under a plan
    installed with `fused_stem`, also "fused": {producer name: forwards whose conv emitted the
    codes itself (K31)} and "unfused": {producer name: why the edge stays on K27 (geometry,
    grouped conv), or {reason: forwards of a fused edge that took K27 (non-contiguous / non-fp32
    input, the shape rule)}}.  Under a plan installed with `image_u8`, also "u8": {producer name:
    forwards of a uint8 batch on K32} and "un_u8": {producer name: {reason: forwards whose uint8
    batch was normalised on the device for the fp32 emit}}, a producer K32 does not take at all
    (`u8_stem_reason`) listed with its reason from the start."""
    names = {m: n for n, m in qnn.named_modules()}
    stems = _edges(qnn, StemEdge)
    rep = {"edges": [(names[e.at], [names[p] for p in e.pools], names[e.successor]) for e in stems],
           "calls": {names[e.at]: e.calls for e in stems},
           "pooled": {names[p]: k for e in stems for p, k in e.pooled.items()}}
    why = getattr(qnn, "_int_fused_stem", None)
    if why is not None:
        rep["fused"] = {names[e.at]: getattr(e, "fused", 0) for e in stems}
        rep["unfused"] = {names[e.at]: why[names[e.at]] or dict(e.unfused) for e in stems}
    if getattr(qnn, "_int_u8", None) is not None:
        rep["u8"] = {names[e.at]: e.u8 for e in stems}
        rep["un_u8"] = {names[e.at]: dict(e.un_u8) for e in stems}
    return rep


def head_carry_report(qnn):
    """{"edges": [(producer name, pool name, fc name), ...] the installed plan carries int8
    codes along, "calls": {producer name: forwards that emitted codes for the pool}, "pooled":
    {pool name: forwards that summed codes (ssq_avgpool_i8_digits_fwd)}, "fc": {fc name: forwards
    on ssq_qlinear_pooled_fwd}}; empty without a plan."""
    names = {m: n for n, m in qnn.named_modules()}
    heads = _edges(qnn, HeadEdge)
    return {"edges": [(names[e.producer], names[e.at], names[e.fc]) for e in heads],
            "calls": {names[e.producer]: e.emitter.calls for e in heads},
            "pooled": {names[e.at]: e.pooled[e.at] for e in heads},
            "fc": {names[e.fc]: e.calls for e in heads}}


class IntegerGraph:
    """The integer forward of `qnn` as one replayed HIP graph: `graph(x)` copies `x` into a static
    input, replays the capture for `x.shape` and returns the static logits tensor, which is valid
    until the next call.  Every kernel of the route is capturable (no allocation, no sync, no
    float atomics); what replay removes is the per-launch host cost, which bounds the small planes.

    The first call for a shape warms up with two eager forwards on a side stream (MIOpen's solver
    choice for the decoded layers, every once-per-tensor check) and captures `qnn(static_in)` under
    no_grad, eval mode and frozen_weight_cache in one torch.cuda.graph: one stream, no parallel
    branches.  At most `MAX_SHAPES` shapes are kept, the least recently used evicted (a validation
    pass's last batch is partial).

    Ownership: the object holds what the captured kernels read and the graph's pool does not own:
    the static input, the decoded layers' frozen W_hat (the frozen-weight dictionary is dropped
    when its context exits), the split-K and kernel workspaces.  Counters: the off-grid device word
    is written by the replayed kernels and keeps accumulating; the Python-side `calls` of plans and
    edges advance only at capture, so their increments during capture are recorded and added on
    every replay, and the five reports mean what they mean eagerly.

    Staleness: enable_integer_inference / disable_integer_inference bump an epoch on `qnn`; a call
    under another epoch than the construction's raises SSQError.  Beyond that the contract is
    frozen_weight_cache's: nothing -- no weight, quantizer, flag, hook or module -- may change
    between capture and replay; the modules are not walked on a replay.

    Raises ValueError without an installed plan, and, naming it, for a module of `qnn` with a
    forward hook or pre-hook (it would run once, at capture)."""
    MAX_SHAPES = 4

    def __init__(self, qnn):
        if not _plans(qnn) and not getattr(qnn, "_int_edges", None):
            raise ValueError("IntegerGraph: no integer plan installed (enable_integer_inference)")
        for name, m in qnn.named_modules():
            if _hooked(m):
                raise ValueError(f"IntegerGraph: module {name or type(m).__name__!r} carries a forward "
                                 "hook, which would run once, at capture")
        self.qnn, self.epoch = qnn, qnn._int_epoch
        self._shapes = collections.OrderedDict()     # (shape, dtype, strides) -> the captured entry

    def shapes(self):
        """The captured input shapes, least recently used first."""
        return [k[0] for k in self._shapes]

    def _cells(self):
        """The Python-side forward counters: (object, None) for `calls`, (edge, name) for a named
        counter, (edge, (name, key)) for one entry of a named {reason: count}, (edge, pool) for
        `pooled[pool]`."""
        qnn = self.qnn
        edges = list(qnn._int_edges) + [e.emitter for e in qnn._int_edges if e.emitter is not None]
        cells = [(p, None) for _, p in _plans(qnn)] + [(e, None) for e in edges]
        cells += [(e, "fused") for e in edges if "fused" in e.__dict__]   # a fused StemEdge
        for e in edges:
            if "u8" in e.__dict__:                                        # one that takes uint8
                whys = U8_FORWARD_REASONS + ((e.u8_why,) if e.u8_why is not None else ())
                cells += [(e, "u8")] + [(e, ("un_u8", w)) for w in whys]
                cells += [(e, ("u8_form", f)) for f in U8_FORMS]
        return cells + [(e, m) for e in edges for m in e.pools]

    @staticmethod
    def _read(cells):
        return [o.calls if m is None else getattr(o, m) if isinstance(m, str)
                else getattr(o, m[0]).get(m[1], 0) if isinstance(m, tuple) else o.pooled[m]
                for o, m in cells]

    @staticmethod
    def _add(cells, by):
        for (o, m), d in zip(cells, by):
            if m is None:
                o.calls += d
            elif isinstance(m, str):
                setattr(o, m, getattr(o, m) + d)
            elif isinstance(m, tuple):      # a {reason: count}: a reason at 0 is not listed
                counts, v = getattr(o, m[0]), getattr(o, m[0]).get(m[1], 0) + d
                if v or m[1] == o.u8_why:
                    counts[m[1]] = v
                else:
                    counts.pop(m[1], None)
            else:
                o.pooled[m] += d

    @staticmethod
    def _static_like(x):
        """A dense copy of `x` in `x`'s dimension order: a dense NCHW or HWC batch keeps its
        strides (a later `copy_` is flat and the replay stages the same form), a crop view gets a
        dense buffer with its dimensions in the same order."""
        order = sorted(range(x.dim()), key=lambda d: (x.stride(d), -d))      # innermost first
        strides, step = [0] * x.dim(), 1
        for d in order:
            strides[d], step = step, step * int(x.shape[d])
        buf = torch.empty_strided(tuple(x.shape), strides, dtype=x.dtype, device=x.device)
        return buf.copy_(x)

    @torch.no_grad()
    def _capture(self, x):
        qnn = self.qnn
        qnn.eval()
        cells = self._cells()
        before, word = self._read(cells), qnn._int_counter.clone()
        e = {"in": self._static_like(x), "ws": {}}
        with L.frozen_weight_cache(), K.A.workspace_scope(e["ws"]):
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream(x.device))
            with torch.cuda.stream(side):
                for _ in range(2):
                    qnn(e["in"])
            torch.cuda.current_stream(x.device).wait_stream(side)
            mid = self._read(cells)
            e["graph"] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(e["graph"]):
                e["out"] = qnn(e["in"])
            e["frozen"] = dict(L._FROZEN_W)
        after = self._read(cells)
        e["cells"], e["by"] = cells, [a - b for a, b in zip(after, mid)]
        e["residual"] = [(t, t.residual) for t in {c[0] for c in cells} if isinstance(t, TailEdge)]
        # the warm-up and the capture count as no forward: the first replay is the first
        self._add(cells, [b - a for a, b in zip(after, before)])
        qnn._int_counter.copy_(word)
        return e

    def __call__(self, x):
        qnn = self.qnn
        if getattr(qnn, "_int_epoch", 0) != self.epoch:
            raise K.A.SSQError("IntegerGraph: the integer plan was re-installed or removed since "
                               "this graph was built (enable / disable_integer_inference)")
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise K.A.SSQError("IntegerGraph: the input must be a tensor on the HIP device")
        key = (tuple(x.shape), x.dtype, tuple(x.stride()))
        e = self._shapes.get(key)
        if e is None:
            e = self._shapes[key] = self._capture(x)
            while len(self._shapes) > self.MAX_SHAPES:
                self._shapes.popitem(last=False)
        else:
            self._shapes.move_to_end(key)
            e["in"].copy_(x)
        e["graph"].replay()
        self._add(e["cells"], e["by"])
        for t, kind in e["residual"]:
            t.residual = kind
        return e["out"]
