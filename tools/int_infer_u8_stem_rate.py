"""What the uint8 stem (K32, image_u8) saves over K31 fed the same image normalised, batch 64.

    python tools/int_infer_u8_stem_rate.py [--batch 64] [--wbits 2] [--abits 4] [--rounds 7]
                                           [--out profiles/int_infer_u8_stem_rate.txt]
                                           [--parity profiles/int_infer_u8_stem_parity.jsonl]
    python tools/int_infer_u8_stem_rate.py --layouts [--out profiles/int_infer_u8_layout_rate.txt]

Kernel rows: the stem conv leaving as int8 codes from a uint8 image, K32
(ssq_stem_conv_u8_codes_fwd), against K31's code form (ssq_stem_conv_codes_fwd, the parent
commit's kernel: this tree builds it from the unchanged source) fed the same image already
normalised to fp32, with the three torch operations of the normalisation in front of K31 as a row
of its own (what a uint8 loader pays today), K32 with every tile on the border path, and K32's
fp32 form.  Bytes are the algorithmic ones (each tensor read or written once, the weight
included).  The share of codes that differs between the two routes is printed: they are two
contracts.

Chain rows: the three fronts of tools/int_infer_stem_rate.py (the model's own modules, 224 x 224
inputs) under carry_stem=True, fused_stem=True fed the normalised fp32 batch, and under the same
plan with image_u8 fed the uint8 batch (SSQ_STEM_U8=1 and SSQ_STEM_FUSED=1, so the host shape
rules do not choose), alternated round by round in one process per chain.

Parity rows (--parity): per shape, how far K32's fp32 form and the fp32 pipeline (torch
u.float() / 255, - mean, / std, then K31's fp32 form on the decoded weight) land from the float64
decoded conv Y64, in units of 2^-24 * sum |W_hat| (u + |M|) / (255 std).

Model rows: per test model (ResNet-18, MobileNetV2, RegNetX-600M, restored from packed exports,
batch 8) at 32 x 32 and 224 x 224, the share of stem code bytes that differ between the two routes.

Layout rows (--layouts, a table of its own, profiles/int_infer_u8_layout_rate.txt): per stem shape
at 224 x 224 and per view of the uint8 batch -- interleaved 3-byte pixels, 4-byte pixels with a pad
byte, a 256 -> 224 centre crop of planar and of interleaved frames -- K32's code form reading the
view in place against the copy route, torch's .contiguous() of the view followed by the dense
launch, timed together, and the dense launch alone.  The interleaved staging loads single bytes;
aligned wider loads were not tried.  The keep rule is the same: the in-place form is taken for a
shape class when the median it saves exceeds the copy route's min-max spread.

Every sample is a device-event time over enough back-to-back calls to fill >= 50 ms, after a
warm-up of every form; the table holds medians over the rounds with min-max.  The keep rule is
the project's: K32 takes a shape class when the median it saves exceeds the baseline's min-max
spread.  The parent process never opens the GPU: each part runs in a child under its own time
limit, and the first failing child ends the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import int_infer_stem_rate as base  # noqa: E402

# (name, Co, kernel, stride, pad, plane)
KERNEL_SHAPES = [("3->64 7x7/2 @224", 64, 7, 2, 3, 224), ("3->32 3x3/2 @224", 32, 3, 2, 1, 224),
                 ("3->64 7x7/2 @32", 64, 7, 2, 3, 32)]
FORMS = ("K31", "normalise + K31", "K32", "K32 all border", "K32 fp32")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def stem_weight(torch, K, Co, R, g):
    """A W8 asymmetric stem weight as (decoded fp32 weight, StemU8Weight, scale[co])."""
    qw = torch.randint(0, 256, (Co, 3, R, R), generator=g)
    zw = torch.randint(96, 160, (Co,), generator=g).float()
    d = (torch.rand(Co, generator=g) * 0.5 + 0.75) / (128.0 * (3 * R * R) ** 0.5)
    what = ((qw.float() - zw.view(-1, 1, 1, 1)) * d.view(-1, 1, 1, 1)).cuda()
    packed = qw.to(torch.uint8).reshape(-1).cuda()
    prep = K.stem_u8_weight_prepare(packed, (Co, 3, R, R), zw.cuda(), 8, 0)
    assert int(prep.bad.item()) == 0
    return what, prep, d.cuda()


def run_kernels(args):
    import torch
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    N = args.batch
    g = torch.Generator().manual_seed(6105)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    mean = torch.tensor(MEAN, device="cuda").reshape(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").reshape(1, 3, 1, 1)
    rows = []
    for name, Co, R, st, pd, H in KERNEL_SHAPES:
        u = torch.randint(0, 256, (N, 3, H, H), generator=g, dtype=torch.uint8).cuda()
        what, prep, d = stem_weight(torch, K, Co, R, g)
        bias = (torch.randn(Co, generator=g) * 0.1).cuda()
        M, s = K.stem_u8_tables(MEAN, STD, d, Co, 3)
        blob = K.stem_weight_prepare(what)
        norm = lambda: (u.float() / 255 - mean) / std
        with torch.no_grad():
            x = norm()
            y = K.stem_conv_u8(u, prep, M, s, st, pd)
            hi = float(torch.clamp(y + bias.view(1, -1, 1, 1), min=0.0).max())
            dq, z = hi / 255.0, 0.0                    # the stem's 8-bit quantizer behind a ReLU
            epi = (bias, None, None, 1, dq, z, 8, False, counter)
            forms = {
                "K31": lambda: K.stem_conv_codes(x, blob, *epi, stride=st, padding=pd),
                "normalise + K31": lambda: K.stem_conv_codes(norm(), blob, *epi, stride=st,
                                                             padding=pd),
                "K32": lambda: K.stem_conv_u8_codes(u, prep, M, s, *epi, stride=st, padding=pd),
                "K32 all border": lambda: K.stem_conv_u8_codes(u, prep, M, s, *epi, stride=st,
                                                               padding=pd, every_tile_border=True),
                "K32 fp32": lambda: K.stem_conv_u8(u, prep, M, s, st, pd),
            }
            mine, old = forms["K32"](), forms["K31"]()
            exact = bool(torch.equal(mine, K.epilogue_codes(y, *epi))
                         and torch.equal(mine, forms["K32 all border"]()))
            assert exact and int(counter.item()) == 0, (exact, int(counter.item()))
            differing = float((mine != old).float().mean())
            us = base.measure(torch, forms, args.rounds)
        OH = y.shape[2]
        Cp = (Co + 15) // 16 * 16
        e_x, e_w, e_y, p_y = N * 3 * H * H, Co * 3 * R * R, N * Co * OH * OH, N * Cp * OH * OH
        nbytes = {"K31": 4 * (e_x + e_w) + p_y, "normalise + K31": e_x + 4 * e_x * 6 + 4 * (e_x + e_w) + p_y,
                  "K32": e_x + e_w + p_y, "K32 all border": e_x + e_w + p_y,
                  "K32 fp32": e_x + e_w + 4 * e_y}
        rows.append({"shape": name, "N": N, "k32_equals_k27_of_its_fp32_form": exact,
                     "tiles_interior_border": list(K.stem_u8_tiles(prep, u.shape, st, pd)),
                     "codes_differing_from_k31_route": differing, "us": us, "bytes": nbytes,
                     "op": 2.0 * N * OH * OH * Co * 3 * R * R})
    print(json.dumps({"rows": rows}), flush=True)


LAYOUTS = ("HWC-3", "RGBA", "crop 256->224", "HWC crop 256->224")


def layout_view(torch, u, layout, frame=256):
    """The dense device batch u (N, 3, H, W) as a view of that layout, everything around it 255."""
    N, C, H, W = u.shape
    px = u.permute(0, 2, 3, 1)
    top, left = (frame - H) // 2, (frame - W) // 2
    if layout == "HWC-3":
        return px.contiguous().permute(0, 3, 1, 2)
    if layout == "RGBA":
        return torch.cat([px, torch.full_like(px[..., :1], 255)], 3).contiguous()[..., :3].permute(0, 3, 1, 2)
    if layout == "crop 256->224":
        fr = torch.full((N, C, frame, frame), 255, dtype=torch.uint8, device=u.device)
        fr[:, :, top:top + H, left:left + W] = u
        return fr[:, :, top:top + H, left:left + W]
    fr = torch.full((N, frame, frame, C), 255, dtype=torch.uint8, device=u.device)
    fr[:, top:top + H, left:left + W, :] = px
    return fr[:, top:top + H, left:left + W, :].permute(0, 3, 1, 2)


def run_layouts(args):
    import torch
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    N = args.batch
    g = torch.Generator().manual_seed(6705)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = []
    for name, Co, R, st, pd, H in KERNEL_SHAPES[:2]:
        u = torch.randint(0, 256, (N, 3, H, H), generator=g, dtype=torch.uint8).cuda()
        _, prep, d = stem_weight(torch, K, Co, R, g)
        bias = (torch.randn(Co, generator=g) * 0.1).cuda()
        M, s = K.stem_u8_tables(MEAN, STD, d, Co, 3)
        with torch.no_grad():
            y = K.stem_conv_u8(u, prep, M, s, st, pd)
            hi = float(torch.clamp(y + bias.view(1, -1, 1, 1), min=0.0).max())
            epi = (bias, None, None, 1, hi / 255.0, 0.0, 8, False, counter)
            run = lambda v: K.stem_conv_u8_codes(v, prep, M, s, *epi, stride=st, padding=pd)
            dense = run(u)
            for layout in LAYOUTS:
                v = layout_view(torch, u, layout)
                form = K.stem_u8_view_form(v)
                assert torch.equal(v, u) and form != "copied" and not v.is_contiguous()
                assert torch.equal(run(v), dense) and torch.equal(run(v.contiguous()), dense)
                us = base.measure(torch, {"dense": lambda: run(u),
                                          "copy + dense": lambda v=v: run(v.contiguous()),
                                          "in place": lambda v=v: run(v)}, args.rounds)
                rows.append({"shape": name, "N": N, "kernel": [R, R, st, st], "layout": layout,
                             "form": form, "us": us})
            assert int(counter.item()) == 0
    print(json.dumps({"rows": rows}), flush=True)


def layouts_table(args):
    """The parent of --layouts: one child, the table, the keep rule per form and shape class."""
    rows = child(["--layouts-child"], args)["rows"]
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(26)

    lines = [f"provenance {json.dumps(provenance())}",
             f"uint8 stem (K32) on views of the image batch, batch {args.batch} at 224 x 224, code form, "
             f"a W8 asymmetric stem weight; median us over {args.rounds} rounds (min-max), forms "
             "alternated round by round; every form's codes equal the dense launch's byte for byte",
             "copy + dense: torch .contiguous() of the view, then the dense launch, timed together "
             "(the route before views were read in place); in place: the strided launch on the view",
             "the interleaved staging loads single bytes; aligned wider loads: not tried",
             "",
             f"{'shape':<20}{'view':<20}{'form':<13}{'dense us':>26}{'copy + dense us':>26}"
             f"{'in place us':>26} {'saved':>8} {'spread':>8} {'old/new':>8} {'clear':>6}"]
    for r in rows:
        b, t = r["us"]["copy + dense"], r["us"]["in place"]
        saved, spread = b["median"] - t["median"], b["max"] - b["min"]
        lines.append(f"{r['shape']:<20}{r['layout']:<20}{r['form']:<13}{cell(r['us']['dense'])}{cell(b)}"
                     f"{cell(t)} {saved:8.1f} {spread:8.1f} {b['median'] / t['median']:8.2f} "
                     f"{'yes' if saved > spread else 'NO':>6}")
    lines.append("saved: copy + dense - in place medians; spread: copy + dense's max - min; clear: saved "
                 "> spread (the keep rule: auto reads a form in place for a shape class only where "
                 "every measured view of that form clears it)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


def run_parity(args):
    """Per shape (batch 2): the worst |y - Y64| of K32's fp32 form and of the fp32 pipeline, in
    units of 2^-24 * the bound's magnitude."""
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    g = torch.Generator().manual_seed(6205)
    mean = torch.tensor(MEAN, device="cuda").reshape(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").reshape(1, 3, 1, 1)
    recs = []
    for name, Co, R, st, pd, H in KERNEL_SHAPES:
        u = torch.randint(0, 256, (2, 3, H, H), generator=g, dtype=torch.uint8).cuda()
        what, prep, d = stem_weight(torch, K, Co, R, g)
        M, s = K.stem_u8_tables(MEAN, STD, d, Co, 3)
        with torch.no_grad():
            y32 = K.stem_conv_u8(u, prep, M, s, st, pd).double()
            pipe = K.stem_conv((u.float() / 255 - mean) / std, K.stem_weight_prepare(what), st, pd).double()
            x64 = (u.double() / 255 - mean.double()) / std.double()
            y64 = F.conv2d(x64, what.double(), None, st, pd)
            mag_in = (u.double() + M.double().abs().reshape(1, 3, 1, 1)) / (255 * std.double())
            mag = F.conv2d(mag_in, what.double().abs(), None, st, pd) * 2.0 ** -24
        recs.append({"test": "int_infer_u8_stem_parity", "shape": name, "N": 2,
                     "bound_roundings": 11,
                     "k32_worst_err_over_mag_in_2^-24": float(((y32 - y64).abs() / mag).max()),
                     "fp32_pipeline_worst_err_over_mag_in_2^-24": float(((pipe - y64).abs() / mag).max())})
    print(json.dumps({"parity": recs}), flush=True)


MODELS = (("resnet18", False), ("mobilenetv2", True), ("regnetx_600m", True))


def run_models(args):
    """Per test model (restored from its packed export, batch 8) at 32 x 32 and 224 x 224: the share
    of stem code bytes that differ between a uint8 forward on K32 and the same plan's fp32 emit
    (K31) fed the batch normalised.  Recorded, not a pass / fail figure."""
    import torch
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd import quant as Q
    from shiftedscalequantization_amd.quant.integer import StemEdge, normalise_u8

    os.environ["SSQ_STEM_FUSED"] = "1"
    os.environ["SSQ_STEM_U8"] = "1"
    mean = torch.tensor(MEAN, device="cuda").reshape(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").reshape(1, 3, 1, 1)
    recs = []
    for i, (arch, grouped) in enumerate(MODELS):
        for H in (32, 224):
            torch.manual_seed(6505 + i)
            u = torch.randint(0, 256, (8, 3, H, H), dtype=torch.uint8,
                              generator=torch.Generator().manual_seed(6605 + i)).cuda()
            x = normalise_u8(u, mean, std)
            src = D.build_qnn(arch, args.wbits, args.abits, device="cuda")
            src.set_quant_state(True, True)
            with torch.no_grad():
                src(x)                                 # initialises every quantizer
            qnn = D.build_qnn(arch, args.wbits, args.abits, device="cuda")
            Q.load_quantized(qnn, Q.export_quantized(src))
            qnn.set_quant_state(True, True)
            qnn.eval()
            del src
            Q.enable_integer_inference(qnn, x, grouped=grouped, carry_stem=True, fused_stem=True,
                                       image_u8=(MEAN, STD))
            edge, = [e for e in qnn._int_edges if type(e) is StemEdge]
            with torch.no_grad():
                k32, k31 = edge.emit(u), edge.emit(x)
            rep = Q.stem_carry_report(qnn)
            assert list(rep["u8"].values()) == [1] and list(rep["fused"].values()) == [1], rep
            diff = (k32.to(torch.int32) - k31.to(torch.int32)).abs()
            recs.append({"test": "int_infer_u8_stem_code_share", "arch": arch, "batch": [8, 3, H, H],
                         "stem_code_bytes": int(k32.numel()),
                         "share_differing_from_k31_route": float((diff != 0).float().mean()),
                         "max_code_difference": int(diff.max())})
            Q.disable_integer_inference(qnn)
            del qnn
    print(json.dumps({"models": recs}), flush=True)


def run_chain(i, args):
    import torch
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd import quant as Q

    os.environ["SSQ_STEM_FUSED"] = "1"
    os.environ["SSQ_STEM_U8"] = "1"
    name, arch, grouped, front_of = base.CHAINS[i]
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(6305 + i)
    u = torch.randint(0, 256, (args.batch, 3, 224, 224), dtype=torch.uint8,
                      generator=torch.Generator().manual_seed(6405 + i)).cuda()
    mean = torch.tensor(MEAN, device="cuda").reshape(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").reshape(1, 3, 1, 1)
    x = (u.float() / 255 - mean) / std
    src = D.build_qnn(arch, args.wbits, args.abits, device="cuda")
    src.set_quant_state(True, True)
    with torch.no_grad():
        src(x[:8])                                     # initialises every quantizer
    qnn = D.build_qnn(arch, args.wbits, args.abits, device="cuda")
    Q.load_quantized(qnn, Q.export_quantized(src))
    qnn.set_quant_state(True, True)
    qnn.eval()
    del src
    front = nn.Sequential(*front_of(qnn.model))
    Q.enable_integer_inference(qnn, x[:8], grouped=grouped, carry_stem=True, fused_stem=True,
                               image_u8=(MEAN, STD))
    feeds = {"K31 (fp32 image)": x, "K32 (uint8 image)": u}

    def run(inp):
        with torch.no_grad():
            return front(inp)

    outs = {k: K.materialize_epi(run(v)).clone() for k, v in feeds.items()}
    rep = Q.stem_carry_report(qnn)
    assert Q.integer_report(qnn)["off_grid"] == 0 and list(rep["u8"].values()) == [1], rep
    assert list(rep["fused"].values()) == [1] and all(not v for v in rep["un_u8"].values()), rep
    us = base.measure(torch, {k: (lambda v=v: run(v)) for k, v in feeds.items()}, args.rounds)
    diff = (outs["K32 (uint8 image)"] - outs["K31 (fp32 image)"]).abs()
    print(json.dumps({"chain": name, "N": args.batch, "edge": rep["edges"],
                      "max_abs_diff": float(diff.max()),
                      "share_differing": float((diff != 0).float().mean()),
                      "max_abs_output": float(outs["K31 (fp32 image)"].abs().max()), "us": us}),
          flush=True)


def child(extra, args):
    cmd = [sys.executable, os.path.abspath(__file__), *extra, "--batch", str(args.batch), "--wbits",
           str(args.wbits), "--abits", str(args.abits), "--rounds", str(args.rounds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"{' '.join(extra)} failed (rc={r.returncode}); stopping")
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out, flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--wbits", type=int, default=2)
    ap.add_argument("--abits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=150, help="seconds per child")
    ap.add_argument("--kernels", action="store_true", help="(child) the kernel rows only")
    ap.add_argument("--parity-child", action="store_true", help="(child) the parity rows only")
    ap.add_argument("--models-child", action="store_true", help="(child) the per-model code shares")
    ap.add_argument("--chain", type=int, default=None, help="(child) run this chain only")
    ap.add_argument("--no-chains", action="store_true", help="skip the model fronts")
    ap.add_argument("--layouts", action="store_true",
                    help="the strided-view table instead (profiles/int_infer_u8_layout_rate.txt)")
    ap.add_argument("--layouts-child", action="store_true", help="(child) the layout rows only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity", default=None, help="append the parity records to this jsonl file")
    args = ap.parse_args(argv)
    if args.kernels:
        return run_kernels(args)
    if args.parity_child:
        return run_parity(args)
    if args.models_child:
        return run_models(args)
    if args.chain is not None:
        return run_chain(args.chain, args)
    if args.layouts_child:
        return run_layouts(args)
    if args.layouts:
        return layouts_table(args)
    kern = child(["--kernels"], args)
    par = child(["--parity-child"], args)["parity"]
    models = child(["--models-child"], args)["models"]
    chains = [] if args.no_chains else [child(["--chain", str(i)], args)
                                        for i in range(len(base.CHAINS))]
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance
    if args.parity:
        with open(args.parity, "a") as fh:
            for rec in par + models:
                fh.write(json.dumps(dict(rec, **provenance())) + "\n")

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(26)

    def verdict(b, s):
        saved, spread = b["median"] - s["median"], b["max"] - b["min"]
        return (f"{saved:8.1f} {spread:8.1f} {b['median'] / s['median']:8.2f} "
                f"{'yes' if saved > spread else 'NO':>6}")

    lines = [f"provenance {json.dumps(provenance())}",
             f"uint8 stem (image_u8, K32), batch {args.batch}, a W8 asymmetric stem weight with the "
             f"8-bit stem quantizer; median us over {args.rounds} rounds (min-max), forms alternated "
             "round by round",
             "",
             "kernels: the bytes are the algorithmic ones (each tensor read or written once; the three "
             "torch operations of the normalisation each read and write the fp32 image); K32's codes "
             "equal K27's of its own fp32 form, and its all-border run, byte for byte on every shape",
             f"{'shape':<20}{'form':<17}{'us':>26} {'MB':>8} {'TB/s':>6} {'Top/s':>7} {'saved':>8} "
             f"{'spread':>8} {'old/new':>8} {'clear':>6}"]
    for r in kern["rows"]:
        for form in FORMS:
            t, nb = r["us"][form], r["bytes"][form]
            ref = {"K32": "K31", "K32 all border": "K31"}.get(form)
            lines.append(f"{r['shape']:<20}{form:<17}{cell(t)} {nb / 1e6:8.1f} "
                         f"{nb / t['median'] / 1e6:6.2f} {r['op'] / t['median'] / 1e6:7.1f} "
                         + (verdict(r["us"][ref], t) if ref else ""))
        lines.append(f"    workgroups on the interior / border path: {r['tiles_interior_border']}; "
                     f"stem codes differing from K31's of the normalised image: "
                     f"{100 * r['codes_differing_from_k31_route']:.4f}%")
    lines += ["", "distance from the float64 decoded conv, worst element, in 2^-24 * sum |W_hat| (u + |M|) "
              "/ (255 std) (the bound counts 11 roundings at Ci = 3):"]
    for rec in par:
        lines.append(f"{rec['shape']:<20} K32 {rec['k32_worst_err_over_mag_in_2^-24']:.3f}   fp32 "
                     f"pipeline (torch normalise + K31 fp32 form) "
                     f"{rec['fp32_pipeline_worst_err_over_mag_in_2^-24']:.3f}")
    lines += ["", "stem codes differing between K32 (uint8 batch) and the same plan's K31 (the batch "
              "normalised), per test model restored from its packed export, batch 8:"]
    for rec in models:
        lines.append(f"{rec['arch']:<14} @{rec['batch'][2]:<4} {100 * rec['share_differing_from_k31_route']:.4f}% of "
                     f"{rec['stem_code_bytes']} bytes (largest difference {rec['max_code_difference']})")
    if chains:
        lines += ["",
                  "chains (carry_stem, fused_stem, image_u8; the same plan fed the fp32 and the uint8 batch)",
                  f"{'chain':<40}{'K31, fp32 image us':>26}{'K32, uint8 image us':>26} {'saved':>8} "
                  f"{'spread':>8} {'old/new':>8} {'clear':>6}"]
        for r in chains:
            b, s = r["us"]["K31 (fp32 image)"], r["us"]["K32 (uint8 image)"]
            lines.append(f"{r['chain']:<40}{cell(b)}{cell(s)} {verdict(b, s)}")
            lines.append(f"    edge {r['edge']}; max |difference| {r['max_abs_diff']:.3g} on "
                         f"{100 * r['share_differing']:.4f}% of the outputs (max |output| "
                         f"{r['max_abs_output']:.3g})")
    lines.append("saved: K31 - K32 medians; spread: K31's max - min; clear: saved > spread (the keep "
                 "rule)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
