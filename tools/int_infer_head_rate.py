"""What putting the pooling head on int8 codes saves (carry_head), batch 64.

    python tools/int_infer_head_rate.py [--batch 64] [--wbits 2] [--abits 4] [--rounds 7]
                                        [--out profiles/int_infer_head_rate.txt]

Kernel rows: K29 (ssq_avgpool_i8_digits_fwd) and K30 (ssq_qlinear_pooled_fwd, with the image
tile 16 and 64) alone at the heads of the supported nets, with the bytes each has to move
(computed from the shapes), beside the forms they replace: K21's inverse + the fp32 mean, and
the decoded fp32 linear.  K30's two tiles are compared bit for bit.

Chain rows: last block -> pool -> fc of a restored model (the model's own modules, fed what the
block receives under the carry_stem plan: the previous block's carried codes, here random codes
of that block's act quantizer on the 7 x 7 plane of a 224 x 224 input; the model is calibrated
and planned on 64 x 64 inputs, where a randomly initialised ResNet-50 stays finite) under two
installed plans, alternated round by round in one process per chain:
    stem   enable_integer_inference(carry_stem=True): the best route without this feature (the
           last block's fp32 tail with a decoded residual, the fp32 pool, the decoded fp32 fc)
    head   carry_head=True: the tail emits codes, K29, K30
The two logits are NOT bit-equal (the head has its own numerics contract); the largest absolute
difference is reported beside the largest logit.  Every sample is a device-event time over
enough back-to-back calls to fill >= 50 ms, after a warm-up of every form; the table holds
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

# (name, channels, plane, classes)
KERNEL_SHAPES = [("r18 512 @7", 512, 7, 1000), ("r50 2048 @7", 2048, 7, 1000),
                 ("mbv2 1280 @7", 1280, 7, 1000), ("rgx3.2 1008 @7", 1008, 7, 1000)]
# (name, arch, grouped, seed, the chain's modules from the model)
CHAINS = [
    ("r18 layer4.1 -> pool -> fc (512 @7)", "resnet18", False, 11,
     lambda m, nn: [m.layer4[-1], m.avgpool, nn.Flatten(1), m.fc]),
    ("mbv2 features.17 -> classifier (1280 @7)", "mobilenetv2", True, 31,
     lambda m, nn: [m.features[17], m.features[18], m.pool, m.classifier]),
    ("rgx3.2 s4.b2 -> pool -> fc (1008 @7)", "regnetx_3200m", True, 41,
     lambda m, nn: [m.s4[-1], m.avgpool, nn.Flatten(1), m.fc]),
    ("r50 layer4.2 -> pool -> fc (2048 @7)", "resnet50", False, 51,
     lambda m, nn: [m.layer4[-1], m.avgpool, nn.Flatten(1), m.fc]),
]
PLANE = 7


def run_kernels(args):
    import numpy as np
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    N = args.batch
    rng = np.random.default_rng(5105)
    rows = []
    for name, Cc, H, Co in KERNEL_SHAPES:
        Cp, HW = (Cc + 15) // 16 * 16, H * H
        q = rng.integers(0, 256, (N, H, H, Cp)).astype(np.int64)
        q[..., Cc:] = 128
        codes = torch.from_numpy((q - 128).astype(np.int8)).cuda()
        d, z = 0.05, 3.0
        qw = rng.integers(0, 256, (Co, Cc))
        zw = rng.integers(0, 256, Co).astype(np.float32)
        d1 = rng.uniform(1e-3, 2e-2, Co).astype(np.float32)
        what = torch.from_numpy((qw - zw.reshape(-1, 1)).astype(np.float32) * d1.reshape(-1, 1)).cuda()
        tz, td = torch.from_numpy(zw).cuda(), torch.from_numpy(d1).cuda()
        packed, bad = K.pack_encode(what, tz, td, False, None, 8, 0, 255)
        prep = K.qweight_prepare(packed, (Co, Cc), tz, 8, 0)
        assert bad == 0 and int(prep.bad.item()) == 0
        sh = K.head_scale(torch.full((1,), d, device="cuda") * td, HW)
        hi, lo, sp = K.avgpool_codes(codes)
        x = K.act_decode(codes, Cc, d, z, 8, False)
        pooled = x.mean([2, 3])

        def k30(tile):
            def f():
                return K.qlinear_pooled(hi, lo, sp, prep, sh, HW, z, 8, False)
            return tile, f

        outs = {}
        for tile, f in (k30(16), k30(64)):
            K.qlinear_pooled_tile(tile)
            outs[tile] = f().clone()
        same = bool(torch.equal(outs[16].view(torch.int32), outs[64].view(torch.int32)))
        ref = F.linear(pooled, what)
        drift = float((outs[16] - ref).abs().max())
        assert same, name
        us = {}
        K.qlinear_pooled_tile(16)
        us.update(measure(torch, {
            "decode + mean": lambda: K.act_decode(codes, Cc, d, z, 8, False).mean([2, 3]),
            "K29": lambda: K.avgpool_codes(codes),
            "fp32 linear": lambda: F.linear(pooled, what),
            "K30 tile 16": k30(16)[1]}, args.rounds))
        K.qlinear_pooled_tile(64)
        us.update(measure(torch, {"K30 tile 64": k30(64)[1]}, args.rounds))
        K.qlinear_pooled_tile(16)
        Cop, Kp = (Co + 63) // 64 * 64, (Cp + 63) // 64 * 64
        nbytes = {"decode + mean": N * HW * Cp + 2 * 4 * N * Cc * HW + 4 * N * Cc,
                  "K29": N * HW * Cp + 2 * N * Cp + 4 * N,
                  "fp32 linear": 4 * (N * Cc + Co * Cc + N * Co),
                  "K30 tile 16": 2 * N * Cp + 4 * N + Cop * Kp + 8 * Cop + 4 * Co + 4 * N * Co}
        nbytes["K30 tile 64"] = nbytes["K30 tile 16"]
        rows.append({"shape": name, "N": N, "tiles_identical": same, "us": us, "bytes": nbytes,
                     "max_abs_diff_vs_fp32": drift, "max_abs_output": float(ref.abs().max())})
    print(json.dumps({"rows": rows}), flush=True)


def run_chain(i, args):
    import torch
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd import quant as Q

    name, arch, grouped, seed, chain_of = CHAINS[i]
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(seed)
    x = torch.randn(8, 3, 64, 64, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    src = D.build_qnn(arch, args.wbits, args.abits, device="cuda")
    src.set_quant_state(True, True)
    with torch.no_grad():
        src(x[:2])                                     # initialises every quantizer
    qnn = D.build_qnn(arch, args.wbits, args.abits, device="cuda")
    Q.load_quantized(qnn, Q.export_quantized(src))
    qnn.set_quant_state(True, True)
    qnn.eval()
    del src
    mods = chain_of(qnn.model, nn)
    chain = nn.Sequential(*mods)

    def install(route):
        mode = {"carry_stem": True} if route == "stem" else {"carry_head": True}
        return Q.enable_integer_inference(qnn, x, grouped=grouped, **mode)

    # the chain's input: the previous block's carried codes, as its first block receives them
    # in a whole forward under the stem plan, redrawn on the 7 x 7 plane at the batch size
    install("stem")
    # (seen through the instance's forward, not a hook: a hooked block is handed fp32)
    seen, first = [], mods[0].forward
    mods[0].forward = lambda t: (seen.append(t), first(t))[1]
    with torch.no_grad():
        qnn(x)
    del mods[0].forward
    cc = getattr(seen[0], "_ssq_codes", None)
    assert cc is not None, "the chain's input is not carried under the stem plan"
    lo, hi = K.qrange(cc.n_bits, cc.sym)
    g = torch.Generator().manual_seed(seed + 2)
    inp = torch.zeros(args.batch, PLANE, PLANE, seen[0].shape[-1], dtype=torch.int8)
    inp[..., :cc.shape[1]] = (torch.randint(lo, hi + 1, (args.batch, PLANE, PLANE, cc.shape[1]),
                                            generator=g) - (lo + 128)).to(torch.int8)
    inp = K.carried(inp.cuda(), (args.batch, cc.shape[1], PLANE, PLANE), *cc.quantizer())
    carried_in = True

    def run():
        with torch.no_grad():
            return chain(inp)

    outs, plans, reports, off_grid = {}, {}, {}, 0
    for route in ("stem", "head"):
        plans[route] = install(route)
        outs[route] = run().clone()
        reports[route] = Q.head_carry_report(qnn)
        off_grid += Q.integer_report(qnn)["off_grid"]
    rep = reports["head"]
    assert off_grid == 0 and reports["stem"]["edges"] == [] and len(rep["edges"]) == 1, reports
    assert list(rep["fc"].values()) == [1] and list(rep["pooled"].values()) == [1], rep
    gained = sorted(n for n, v in plans["head"].items() if v == "int8" and plans["stem"][n] != "int8")
    us = measure(torch, {r: run for r in ("stem", "head")}, args.rounds, before=install)
    print(json.dumps({"chain": name, "N": args.batch, "input_carried": carried_in,
                      "plane": list(inp.shape[1:3]),
                      "max_abs_diff_vs_stem": float((outs["head"] - outs["stem"]).abs().max()),
                      "max_abs_output": float(outs["stem"].abs().max()),
                      "layers_gained": gained, "edge": rep["edges"], "us": us}), flush=True)


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
    chains, failed = [], None
    for i in range(len(CHAINS)):
        try:
            chains.append(child(["--chain", str(i)], args))
        except SystemExit as e:         # nothing more is started; what was measured is kept
            failed = str(e)
            break
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(26)

    lines = [f"provenance {json.dumps(provenance())}",
             f"pooling head on codes (carry_head), batch {args.batch}, W{args.wbits}A{args.abits} with "
             f"the 8-bit head; median us over {args.rounds} rounds (min-max), forms alternated round "
             f"by round",
             "",
             "kernels (8-bit codes and weights, 1000 classes): the bytes are the algorithmic ones "
             "(each tensor read or written once); K30's two image tiles give identical bits",
             f"{'shape':<16}{'form':<15}{'us':>26} {'MB':>8} {'GB/s':>8}"]
    for r in kern["rows"]:
        for form in ("decode + mean", "K29", "fp32 linear", "K30 tile 16", "K30 tile 64"):
            t, nb = r["us"][form], r["bytes"][form]
            lines.append(f"{r['shape']:<16}{form:<15}{cell(t)} {nb / 1e6:8.2f} "
                         f"{nb / t['median'] / 1e3:8.1f}")
        lines.append(f"    max |K30 - fp32 linear of the fp32 mean| {r['max_abs_diff_vs_fp32']:.3g} "
                     f"(max |output| {r['max_abs_output']:.3g})")
    lines += ["",
              "chains: nothing off the grid; the head route's fc ran on K30 once per forward",
              f"{'chain':<44}{'stem us':>26}{'head us':>26} {'saved':>8} {'spread':>8} "
              f"{'stem/head':>9} {'clear':>6}"]
    for r in chains:
        b, s = r["us"]["stem"], r["us"]["head"]
        saved, spread = b["median"] - s["median"], b["max"] - b["min"]
        lines.append(f"{r['chain']:<44}{cell(b)}{cell(s)} {saved:8.1f} {spread:8.1f} "
                     f"{b['median'] / s['median']:9.2f} {'yes' if saved > spread else 'NO':>6}")
        lines.append(f"    edge {r['edge']}; plane {r['plane']}; input carried codes: "
                     f"{r['input_carried']}; layers gained by the plan {r['layers_gained']}; "
                     f"max |head - stem| {r['max_abs_diff_vs_stem']:.3g} "
                     f"(max |logit| {r['max_abs_output']:.3g})")
    lines.append("saved: stem - head medians; spread: the stem route's max - min; clear: saved > "
                 "spread (the keep rule of an edge class)")
    if failed:
        lines.append(f"INCOMPLETE: {failed}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if failed:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
