"""What graph replay and the split-K form of K23 move on the small planes.

    python tools/int_infer_smallplane_rate.py [--rounds 7] [--parent DIR]
                                              [--out profiles/int_infer_smallplane_rate.txt]

Kernel rows: the dense int8 conv (K23) at the small planes of a 224 x 224 forward, W2A4, batch 64
and batch 8 -- ResNet-18 layer3's 3x3 (256 ch @14), the 512-channel 3x3 on the 7 x 7 plane
(ResNet-18 layer4; ResNet-50's layer4 conv2) and ResNet-50's 1x1 2048 -> 512 @7 -- with Z = 1 (the
one-kernel form, the parent's kernel) and the split-K form at Z = 2, 4, 8, as the fp32 form and as
the code-emitting form, timed through the Python wrappers and inside a captured graph of 20
back-to-back calls.  The in-graph number decides (the keep rule of kernels.qconv_splits): a Z
clears where the unsplit median exceeds its median by more than the unsplit form's spread.  Every
split output is compared with the unsplit one bit for bit before anything is timed.

Model rows: ResNet-18, MobileNetV2 (grouped) and RegNetX-3200M (grouped), restored from an export
calibrated on 64 x 64 inputs, every carry flag on, on 224 x 224 batches of 64 and 8: the eager
forward, quant.IntegerGraph, and IntegerGraph on a plan with splitk=True (the host rule as
committed, or --wg / --steps); the three logits are compared bit for bit.

Eager rows (--parent DIR: a checkout of the parent commit with its library built): the flags-off
eager forward of the same six (model, batch) rows at the parent commit and at this one, run as
parent, new, parent, new, parent, new in processes of their own, same machine and session, 7
rounds each.  Per row: the median of the three run medians; parent spread: max - min over all 21
parent rounds.  Rule (profiles/int_infer_planner_rate.txt): the new median may exceed the
parent's by at most the parent's own spread.

Every sample is a device-event time over enough back-to-back calls to fill >= 50 ms, after a
warm-up of every form; forms are alternated round by round in one process; the table holds
medians over the rounds with min-max.  The parent process never opens the GPU: each part runs in
a child under its own time limit, and the first failing child ends the run (the rows measured
until then are still written, marked INCOMPLETE).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from int_infer_stem_rate import measure  # noqa: E402

# (name, Ci, plane, Co, R, stride, pad)
KERNEL_SHAPES = [("r18 layer3 3x3 256 @14", 256, 14, 256, 3, 1, 1),
                 ("r18 layer4 / r50 3x3 512 @7", 512, 7, 512, 3, 1, 1),
                 ("r50 1x1 2048->512 @7", 2048, 7, 512, 1, 1, 0)]
BATCHES = (64, 8)
ZS = (1, 2, 4, 8)
IN_GRAPH = 20
# (name, arch, grouped, seed)
MODELS = [("resnet18", "resnet18", False, 11), ("mobilenetv2", "mobilenetv2", True, 31),
          ("regnetx_3200m", "regnetx_3200m", True, 41)]


def run_kernels(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    name, Ci, H, Co, R, stride, pad = KERNEL_SHAPES[args.kernels]
    N = args.batch
    rng = np.random.default_rng(6105 + args.kernels)
    qw = rng.integers(0, 4, (Co, Ci, R, R))
    zw = rng.integers(0, 4, Co).astype(np.float32)
    d1 = rng.uniform(1e-3, 2e-2, Co).astype(np.float32)
    what = torch.from_numpy((qw - zw.reshape(-1, 1, 1, 1)).astype(np.float32)
                            * d1.reshape(-1, 1, 1, 1)).cuda()
    tz, td = torch.from_numpy(zw).cuda(), torch.from_numpy(d1).cuda()
    packed, bad = K.pack_encode(what, tz, td, False, None, 2, 0, 3)
    prep = K.qweight_prepare(packed, tuple(qw.shape), tz, 2, 0)
    assert bad == 0 and int(prep.bad.item()) == 0
    Cp = (Ci + 15) // 16 * 16
    codes = torch.from_numpy(rng.integers(-128, -112, (N, H, H, Cp)).astype(np.int8)).cuda()
    da, za = 0.05, 3.0
    scale = (torch.full((1,), da, device="cuda") * td).contiguous()
    bias = torch.from_numpy(rng.normal(0, 0.1, Co).astype(np.float32)).cuda()
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(act_zp=za, act_bits=4)
    OH = (H + 2 * pad - R) // stride + 1
    M, nk = N * OH * OH, -(-R * R * Cp // 64)
    y1 = K.qconv(codes, prep, scale, stride, pad, **kw)
    od = float(torch.clamp(y1 + bias.view(1, -1, 1, 1), min=0).max()) / 15.0

    def form(kind, Z):
        z = None if Z == 1 else Z
        if kind == "fp32":
            return lambda: K.qconv(codes, prep, scale, stride, pad, splits=z, **kw)
        return lambda: K.qconv_codes(codes, prep, scale, stride, pad, bias=bias, relu=1, out_delta=od,
                                     out_zp=0.0, out_bits=4, bad=counter, splits=z, **kw)

    zs = [Z for Z in ZS if Z <= nk]
    row = {"shape": name, "N": N, "M": M, "Co": Co, "nk": nk,
           "workgroups": -(-M // 64) * -(-Co // 64), "wrappers": {}, "graph": {}}
    for kind in ("fp32", "codes"):
        want = form(kind, 1)().clone()
        for Z in zs[1:]:
            assert torch.equal(form(kind, Z)().view(torch.uint8), want.view(torch.uint8)), (kind, Z)
        forms = {f"Z={Z}": form(kind, Z) for Z in zs}
        row["wrappers"][kind] = measure(torch, forms, args.rounds)
        replays = {}
        side = torch.cuda.Stream()
        for k, f in forms.items():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                f()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep = [f() for _ in range(IN_GRAPH)]
            replays[k] = (g, keep)
        t = measure(torch, {k: g.replay for k, (g, _) in replays.items()}, args.rounds)
        row["graph"][kind] = {k: {s: v / IN_GRAPH for s, v in d.items()} for k, d in t.items()}
        del replays
    assert int(counter.item()) == 0
    print(json.dumps(row), flush=True)


def run_model(args):
    root = args.parent if args.parent_child else ROOT
    sys.path.insert(0, root)
    import torch
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd import quant as Q
    from shiftedscalequantization_amd.quant.quant_layer import frozen_weight_cache

    name, arch, grouped, seed = MODELS[args.model]
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(seed)
    small = torch.randn(8, 3, 64, 64, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    src = D.build_qnn(arch, 2, 4, device="cuda")
    src.set_quant_state(True, True)
    with torch.no_grad():
        src(small[:2])                                 # initialises every quantizer
    blob = Q.export_quantized(src)
    del src

    def restored(**flags):
        qnn = D.build_qnn(arch, 2, 4, device="cuda")
        Q.load_quantized(qnn, blob)
        qnn.set_quant_state(True, True)
        qnn.eval()
        Q.enable_integer_inference(qnn, small, grouped=grouped, carry_head=True, **flags)
        return qnn

    x = torch.randn(args.batch, 3, 224, 224, generator=torch.Generator().manual_seed(seed + 2)).cuda()
    plain = restored()

    def eager():
        with torch.no_grad(), frozen_weight_cache():
            return plain(x)

    forms, out = {"eager": eager}, {"model": name, "N": args.batch, "parent": bool(args.parent_child)}
    want = eager().clone()
    if not (args.parent_child or args.eager_only):
        if args.wg is not None:
            K.QSPLIT_WORKGROUPS, K.QSPLIT_STEPS = args.wg, args.steps
        split = restored(splitk=True)
        g1, g2 = Q.IntegerGraph(plain), Q.IntegerGraph(split)
        forms["graph"], forms["graph + split"] = (lambda: g1(x)), (lambda: g2(x))
        for k in ("graph", "graph + split"):
            assert torch.equal(forms[k]().view(torch.int32), want.view(torch.int32)), k
        rep = Q.split_report(split)
        out["split"] = {n: z for n, z in rep.items() if z > 1}
        out["thresholds"] = [K.QSPLIT_WORKGROUPS, K.QSPLIT_STEPS]
        out["off_grid"] = Q.integer_report(plain)["off_grid"] + Q.integer_report(split)["off_grid"]
    out["us"] = measure(torch, forms, args.rounds)
    print(json.dumps(out), flush=True)


def child(extra, args):
    cmd = [sys.executable, os.path.abspath(__file__), *extra, "--rounds", str(args.rounds)]
    if args.wg is not None:
        cmd += ["--wg", str(args.wg), "--steps", str(args.steps)]
    if args.parent:
        cmd += ["--parent", args.parent]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"{' '.join(extra)} failed (rc={r.returncode}); stopping")
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out, flush=True)
    return out


def cell(t):
    return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(24)


def keep_lines(rows, splits_of):
    """The keep rule per shape class, from the in-graph medians: the Z that clear in both forms,
    what the host rule (splits_of(M, Co, Kp)) does with the class, and the bounds that follow."""
    lines = ["keep rule (kernels.qconv_splits): a Z clears for a shape class where, in graph, it saves more "
             "than the unsplit spread in BOTH forms (the rule does not know which will run); the rule may "
             "split a class only with a Z that clears",
             f"{'shape':<30}{'N':>3} {'wgs':>5} {'nk':>4}  {'clearing Z (saved fp32 / codes us)':<52}"
             f"{'rule Z':>7} {'split wgs':>10} {'steps':>6}  verdict"]
    kept, bad = [], False
    for r in rows:
        clear = {}
        for k in r["graph"]["fp32"]:
            if k == "Z=1":
                continue
            saved = []
            for kind in ("fp32", "codes"):
                base, t = r["graph"][kind]["Z=1"], r["graph"][kind][k]
                saved.append((base["median"] - t["median"], base["max"] - base["min"]))
            if all(sv > sp for sv, sp in saved):
                clear[int(k[2:])] = saved
        Z = splits_of(r["M"], r["Co"], r["nk"] * 64)
        if Z == 1:
            verdict = "unsplit" + (" (a clearing Z is given up)" if clear else "")
        elif Z in clear:
            verdict = "ok"
            kept.append((r["workgroups"] * Z, r["nk"] // Z))
        else:
            verdict, bad = "VIOLATES the keep rule", True
        txt = ", ".join(f"{z} ({sv[0][0]:.1f} / {sv[1][0]:.1f})" for z, sv in sorted(clear.items())) or "none"
        lines.append(f"{r['shape']:<30}{r['N']:>3} {r['workgroups']:>5} {r['nk']:>4}  {txt:<52}{Z:>7} "
                     f"{r['workgroups'] * Z if Z > 1 else '':>10} {r['nk'] // Z if Z > 1 else '':>6}  {verdict}")
    if kept:
        lines.append(f"the classes the rule splits: split grids of up to {max(k[0] for k in kept)} workgroups, "
                     f"slices of at least {min(k[1] for k in kept)} k steps (QSPLIT_WORKGROUPS, QSPLIT_STEPS)")
    return lines, bad


def eager_lines(rows):
    """Parent and new eager forwards, alternated run by run (the planner rate file's method)."""
    lines = ["flags-off eager forward at the parent commit and at this one: parent, new, parent, new, parent, "
             "new, a process each, 7 rounds each; per row the median of the three run medians; parent spread: "
             "max - min over all 21 parent rounds; rule: the new median may exceed the parent's by at most "
             "the parent's own spread.  us per forward",
             f"{'model':<15}{'N':>3} {'parent medians':>27} {'new medians':>27} {'parent':>9} {'new':>9} "
             f"{'spread':>7}  verdict"]
    import statistics
    for (name, N), runs in rows.items():
        p = [r["us"]["eager"] for r in runs if r["parent"]]
        n = [r["us"]["eager"] for r in runs if not r["parent"]]
        pm, nm = statistics.median(t["median"] for t in p), statistics.median(t["median"] for t in n)
        spread = max(t["max"] for t in p) - min(t["min"] for t in p)
        ps = " ".join("%.1f" % t["median"] for t in p)
        ns = " ".join("%.1f" % t["median"] for t in n)
        lines.append(f"{name:<15}{N:>3} {ps:>27} {ns:>27} {pm:9.1f} {nm:9.1f} {spread:7.1f}  "
                     f"{'ok' if nm - pm <= spread else 'OVER'}")
    return lines


def kernel_lines(rows):
    lines = ["kernels: us per call; 'graph' is a replayed capture of 20 back-to-back calls / 20 and "
             "decides; saved = Z=1 median - this median, spread = the Z=1 form's max - min (both in "
             "graph), clear: saved > spread",
             f"{'shape':<30}{'N':>3} {'wgs':>5} {'nk':>4} {'form':<6}{'Z':>2}{'wrappers us':>24}"
             f"{'graph us':>24} {'saved':>7} {'spread':>7} {'clear':>6}"]
    for r in rows:
        for kind in ("fp32", "codes"):
            base = r["graph"][kind]["Z=1"]
            spread = base["max"] - base["min"]
            for k, t in r["graph"][kind].items():
                saved = base["median"] - t["median"]
                tail = "" if k == "Z=1" else (f" {saved:7.1f} {spread:7.1f} "
                                              f"{'yes' if saved > spread else 'NO':>6}")
                lines.append(f"{r['shape']:<30}{r['N']:>3} {r['workgroups']:>5} {r['nk']:>4} {kind:<6}"
                             f"{k[2:]:>2}{cell(r['wrappers'][kind][k])}{cell(t)}{tail}")
    return lines


def model_lines(rows):
    lines = ["whole models, 224 x 224, W2A4 with the 8-bit head and stem, every carry flag on; us per "
             "forward (images/s at the median); the three logits are bit-identical",
             f"{'model':<15}{'N':>3} {'form':<15}{'us':>24} {'img/s':>9}  split layers (Z)"]
    for r in rows:
        for k, t in r["us"].items():
            note = ""
            if k == "graph + split":
                note = ", ".join(f"{n.replace('model.', '')} x{z}" for n, z in r["split"].items()) or "none"
            lines.append(f"{r['model']:<15}{r['N']:>3} {k:<15}{cell(t)} "
                         f"{r['N'] / t['median'] * 1e6:9.0f}  {note}")
    if rows:
        lines.append("(a replay copies the batch into the graph's static input, 38.5 MB at batch 64, which the "
                     "eager forward does not)")
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--batch", type=int, default=64, help="(child)")
    ap.add_argument("--kernels", type=int, default=None, help="(child) this kernel shape only")
    ap.add_argument("--model", type=int, default=None, help="(child) this model only")
    ap.add_argument("--parent_child", action="store_true", help="(child) the parent's eager forward")
    ap.add_argument("--eager_only", action="store_true", help="(child) this commit's eager forward only")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--wg", type=int, default=None, help="override kernels.QSPLIT_WORKGROUPS")
    ap.add_argument("--steps", type=int, default=8, help="with --wg: kernels.QSPLIT_STEPS")
    ap.add_argument("--only", choices=["kernels", "models", "eager"], default=None)
    ap.add_argument("--json", default=None, help="also dump the raw rows here")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.kernels is not None:
        return run_kernels(args)
    if args.model is not None:
        return run_model(args)
    kern, models, eager, failed = [], [], {}, None
    try:
        for N in BATCHES if args.only in (None, "kernels") else ():
            for i in range(len(KERNEL_SHAPES)):
                kern.append(child(["--kernels", str(i), "--batch", str(N)], args))
        for i in range(len(MODELS)) if args.only in (None, "models") else ():
            for N in BATCHES:
                models.append(child(["--model", str(i), "--batch", str(N)], args))
        for i in range(len(MODELS)) if args.parent and args.only in (None, "eager") else ():
            for N in BATCHES:
                for extra in ("--parent_child", "--eager_only") * 3:
                    r = child(["--model", str(i), "--batch", str(N), extra], args)
                    eager.setdefault((r["model"], r["N"]), []).append(r)
    except (SystemExit, subprocess.TimeoutExpired) as e:   # nothing more is started
        failed = str(e)
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd.build import provenance
    if args.wg is not None:
        K.QSPLIT_WORKGROUPS, K.QSPLIT_STEPS = args.wg, args.steps
    lines = [f"provenance {json.dumps(provenance())}",
             f"small planes: graph replay and split-K int8 conv; median us over {args.rounds} rounds "
             f"(min-max), forms alternated round by round", ""]
    keep, violated = keep_lines(kern, K.qconv_splits) if kern else ([], False)
    lines += kernel_lines(kern) + [""] + keep + [""] + model_lines(models)
    if eager:
        lines += [""] + eager_lines(eager)
    if violated:
        failed = failed or "the host rule splits a class with a Z that does not clear"
    if models:
        lines.append(f"host rule of the 'graph + split' rows: split while workgroups * Z <= "
                     f"{models[0]['thresholds'][0]} and nk / Z >= {models[0]['thresholds'][1]}; "
                     f"off-grid elements over all forwards: {sum(m['off_grid'] for m in models)}")
    if failed:
        lines.append(f"INCOMPLETE: {failed}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"kernels": kern, "models": models,
                       "eager": [r for v in eager.values() for r in v]}, fh)
    if failed:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
