"""What the fused stem (K31, fused_stem) saves over the library conv + K27 (carry_stem), batch 64.

    python tools/int_infer_fused_stem_rate.py [--batch 64] [--wbits 2] [--abits 4] [--rounds 7]
                                              [--out profiles/int_infer_fused_stem_rate.txt]

Kernel rows: the stem conv leaving as int8 codes, K31 (ssq_stem_conv_codes_fwd) against the
route it replaces, F.conv2d (MIOpen, deterministic solvers, the project's default) followed by
K27 (ssq_epilogue_codes_fwd), with both halves of that route and K31's fp32 form timed on their
own.  Bytes are the algorithmic ones (each tensor read or written once, the weight included),
TF is 2 * N * OH * OW * Co * Ci * R * S over the time.  The codes of the two routes are compared
and the share that differs is printed: MIOpen's summation order is not K31's.

Chain rows: the three fronts of tools/int_infer_stem_rate.py (the model's own modules, 224 x 224
inputs) under carry_stem=True and under carry_stem=True, fused_stem=True (SSQ_STEM_FUSED=1, so
the host shape rule does not choose), alternated round by round in one process per chain.

Every sample is a device-event time over enough back-to-back calls to fill >= 50 ms, after a
warm-up of every form; the table holds medians over the rounds with min-max.  The keep rule is
the project's: K31 takes a shape class when the median it saves exceeds the baseline's min-max
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
FORMS = ("conv (MIOpen)", "K27", "MIOpen + K27", "K31 fp32", "K31")


def run_kernels(args):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    torch.backends.cudnn.deterministic = True
    N = args.batch
    g = torch.Generator().manual_seed(5105)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = []
    for name, Co, R, st, pd, H in KERNEL_SHAPES:
        x = torch.randn(N, 3, H, H, generator=g).cuda()
        w = (torch.randn(Co, 3, R, R, generator=g) / (3 * R * R) ** 0.5).cuda()
        bias = (torch.randn(Co, generator=g) * 0.1).cuda()
        blob = K.stem_weight_prepare(w)
        with torch.no_grad():
            y = F.conv2d(x, w, None, st, pd)
            hi = float(torch.clamp(y + bias.view(1, -1, 1, 1), min=0.0).max())
            d, z = hi / 255.0, 0.0                     # the stem's 8-bit quantizer behind a ReLU
            k27 = lambda t: K.epilogue_codes(t, bias, None, None, 1, d, z, 8, False, counter)
            forms = {
                "conv (MIOpen)": lambda: F.conv2d(x, w, None, st, pd),
                "K27": lambda: k27(y),
                "MIOpen + K27": lambda: k27(F.conv2d(x, w, None, st, pd)),
                "K31 fp32": lambda: K.stem_conv(x, blob, st, pd),
                "K31": lambda: K.stem_conv_codes(x, blob, bias, None, None, 1, d, z, 8, False,
                                                 counter, stride=st, padding=pd),
            }
            mine, lib = forms["K31"](), forms["MIOpen + K27"]()
            exact = bool(torch.equal(mine, k27(forms["K31 fp32"]())))
            assert exact and int(counter.item()) == 0, (exact, int(counter.item()))
            differing = float((mine != lib).float().mean())
            us = base.measure(torch, forms, args.rounds)
        OH = y.shape[2]
        Cp = (Co + 15) // 16 * 16
        e_x, e_w, e_y, p_y = N * 3 * H * H, Co * 3 * R * R, N * Co * OH * OH, N * Cp * OH * OH
        nbytes = {"conv (MIOpen)": 4 * (e_x + e_w + e_y), "K27": 4 * e_y + p_y,
                  "MIOpen + K27": 4 * (e_x + e_w + e_y) + 4 * e_y + p_y,
                  "K31 fp32": 4 * (e_x + e_w + e_y), "K31": 4 * (e_x + e_w) + p_y}
        rows.append({"shape": name, "N": N, "k31_equals_k27_of_its_fp32_form": exact,
                     "codes_differing_from_miopen_route": differing, "us": us, "bytes": nbytes,
                     "flop": 2.0 * N * OH * OH * Co * 3 * R * R})
    print(json.dumps({"rows": rows}), flush=True)


def run_chain(i, args):
    import torch
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd import quant as Q

    os.environ["SSQ_STEM_FUSED"] = "1"
    name, arch, grouped, front_of = base.CHAINS[i]
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(5205 + i)
    x = torch.randn(args.batch, 3, 224, 224, generator=torch.Generator().manual_seed(5305 + i)).cuda()
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

    def install(route):
        return Q.enable_integer_inference(qnn, x[:8], grouped=grouped, carry_stem=True,
                                          **({"fused_stem": True} if route == "fused" else {}))

    def run():
        with torch.no_grad():
            return front(x)

    outs, reports, off_grid = {}, {}, 0
    for route in ("stem", "fused"):
        install(route)
        outs[route] = K.materialize_epi(run()).clone()
        reports[route] = Q.stem_carry_report(qnn)
        off_grid += Q.integer_report(qnn)["off_grid"]
    assert off_grid == 0 and list(reports["stem"]["calls"].values()) == [1], (off_grid, reports)
    assert "fused" not in reports["stem"] and list(reports["fused"]["fused"].values()) == [1], reports
    us = base.measure(torch, {r: run for r in ("stem", "fused")}, args.rounds, before=install)
    diff = (outs["fused"] - outs["stem"]).abs()
    print(json.dumps({"chain": name, "N": args.batch, "edge": reports["fused"]["edges"],
                      "max_abs_diff_vs_stem": float(diff.max()),
                      "share_differing": float((diff != 0).float().mean()),
                      "max_abs_output": float(outs["stem"].abs().max()), "us": us}), flush=True)


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
    ap.add_argument("--chain", type=int, default=None, help="(child) run this chain only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.kernels:
        return run_kernels(args)
    if args.chain is not None:
        return run_chain(args.chain, args)
    kern = child(["--kernels"], args)
    chains = [child(["--chain", str(i)], args) for i in range(len(base.CHAINS))]
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(26)

    def verdict(b, s):
        saved, spread = b["median"] - s["median"], b["max"] - b["min"]
        return (f"{saved:8.1f} {spread:8.1f} {b['median'] / s['median']:8.2f} "
                f"{'yes' if saved > spread else 'NO':>6}")

    lines = [f"provenance {json.dumps(provenance())}",
             f"fused stem (fused_stem, K31), batch {args.batch}, W{args.wbits}A{args.abits} with the "
             f"8-bit stem quantizer; median us over {args.rounds} rounds (min-max), forms alternated "
             "round by round; MIOpen on its deterministic solvers",
             "",
             "kernels: the bytes are the algorithmic ones (each tensor read or written once); K31's "
             "codes equal K27's of its own fp32 form byte for byte on every shape",
             f"{'shape':<20}{'form':<15}{'us':>26} {'MB':>8} {'TB/s':>6} {'TF':>7} {'saved':>8} "
             f"{'spread':>8} {'old/new':>8} {'clear':>6}"]
    for r in kern["rows"]:
        for form in FORMS:
            t, nb = r["us"][form], r["bytes"][form]
            tf = r["flop"] / t["median"] / 1e6 if form != "K27" else 0.0
            ref = {"K31": "MIOpen + K27", "K31 fp32": "conv (MIOpen)"}.get(form)
            lines.append(f"{r['shape']:<20}{form:<15}{cell(t)} {nb / 1e6:8.1f} "
                         f"{nb / t['median'] / 1e6:6.2f} {tf:7.1f} "
                         + (verdict(r["us"][ref], t) if ref else ""))
        lines.append(f"    stem codes differing from the MIOpen + K27 route: "
                     f"{100 * r['codes_differing_from_miopen_route']:.4f}%")
    lines += ["",
              "chains: nothing off the grid; the two routes differ where MIOpen's sum and K31's round "
              "a stem value to different codes",
              f"{'chain':<40}{'carry_stem us':>26}{'fused_stem us':>26} {'saved':>8} {'spread':>8} "
              f"{'old/new':>8} {'clear':>6}"]
    for r in chains:
        b, s = r["us"]["stem"], r["us"]["fused"]
        lines.append(f"{r['chain']:<40}{cell(b)}{cell(s)} {verdict(b, s)}")
        lines.append(f"    edge {r['edge']}; max |fused - stem| {r['max_abs_diff_vs_stem']:.3g} on "
                     f"{100 * r['share_differing']:.4f}% of the outputs (max |output| "
                     f"{r['max_abs_output']:.3g})")
    lines.append("saved: baseline - K31 medians; spread: the baseline's max - min; clear: saved > "
                 "spread (the keep rule)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
