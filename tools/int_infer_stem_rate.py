"""What carrying int8 codes from the stem through the max-pool saves (carry_stem), batch 64.

    python tools/int_infer_stem_rate.py [--batch 64] [--wbits 2] [--abits 4] [--rounds 7]
                                        [--out profiles/int_infer_stem_rate.txt]

Kernel rows: K27 (ssq_epilogue_codes_fwd) against the pair it replaces, K13 (the fp32 epilogue
with the 8-bit stem quantizer) + K21 (ssq_act_encode), and K28 (ssq_maxpool_i8_fwd) against
ssq_maxpool2d_fwd + K21, with the bytes each form has to move (computed from the shapes) and
the rate they imply against the 8 TB/s peak and this box's float4 copy.

Chain rows: the front of a restored model (the model's own modules, 224 x 224 inputs) under
three installed plans, alternated round by round in one process per chain:
    blocks     enable_integer_inference(carry_blocks=True): the best route without this feature
    stem-plan  carry_stem=True with a no-op forward hook on the stem conv: the carry_stem plan
               (a layer behind the max-pool on K21 + K23 instead of the decoded conv) with the
               stem still on K13, the fp32 pool and K21
    stem       carry_stem=True: K27, K28, the readers and the identity residual on codes
`stem` and `stem-plan` outputs are compared bit for bit (the feature's contract); against
`blocks` the largest absolute difference is reported (0 where the plan is the same; where a
layer moved from the decoded conv to the integer one the two differ by fp32 rounding).  Every
sample is a device-event time over enough back-to-back calls to fill >= 50 ms, after a warm-up
of every form; the table holds medians over the rounds with min-max.  The parent process never
opens the GPU: each part runs in a child under its own time limit, and the first failing child
ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TBS = 8.0

# (name, channels, plane)
KERNEL_SHAPES = [("64 ch @112", 64, 112), ("32 ch @112", 32, 112), ("64 ch @16", 64, 16)]
# (name, arch, grouped, the front's modules from the model)
CHAINS = [
    ("r18 stem -> pool -> layer1 (2 blocks)", "resnet18", False,
     lambda m: [m.conv1, m.bn1, m.relu, m.maxpool, m.layer1]),
    ("mbv2 features.0 -> features.2", "mobilenetv2", True,
     lambda m: [m.features[0], m.features[1], m.features[2]]),
    ("rgx3.2 stem -> s1.b1", "regnetx_3200m", True, lambda m: [m.stem, m.s1.b1]),
]


def sampler(torch):
    def sample(f, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / reps          # us per call
    return sample


def measure(torch, forms, rounds, before=None):
    """{form: {"median", "min", "max"}} in us, the forms alternated round by round; `before`
    (form name) runs untimed ahead of each form's samples (installing its plan)."""
    sample = sampler(torch)
    reps = {}
    for k, f in forms.items():                         # warm-up, then size the window
        if before:
            before(k)
        sample(f, 10)
        reps[k] = max(5, int(50e3 / max(sample(f, 10), 1.0)))
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            if before:
                before(k)
                sample(f, 3)
            times[k].append(sample(f, reps[k]))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)}
            for k, v in times.items()}


def run_kernels(args):
    import torch
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    N = args.batch
    g = torch.Generator().manual_seed(4105)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = []
    n = 64 << 20
    src, dst = torch.zeros(n, device="cuda"), torch.empty(n, device="cuda")
    copy = measure(torch, {"copy": lambda: K.stream_copy(src, dst)}, args.rounds)["copy"]
    copy_tbs = 8.0 * n / copy["median"] / 1e6
    del src, dst
    for name, Cc, H in KERNEL_SHAPES:
        y = (torch.randn(N, Cc, H, H, generator=g) * 2.0).cuda()
        bias = (torch.randn(Cc, generator=g) * 0.1).cuda()
        hi = float(torch.clamp(y + bias.view(1, -1, 1, 1), min=0.0).max())
        d, z = hi / 255.0, 0.0                         # the stem's 8-bit quantizer behind a ReLU
        dt, zt = torch.tensor([d], device="cuda"), torch.tensor([z], device="cuda")
        d = float(dt)
        OH = (H + 2 - 3) // 2 + 1
        Cp = (Cc + 15) // 16 * 16
        with torch.no_grad():
            k13 = lambda: K.bias_act_quant(y, bias, None, 1, dt, zt, 8, False)
            x = k13()
            codes = K.epilogue_codes(y, bias, None, None, 1, d, z, 8, False, counter)
            forms = {
                "K13 + K21": lambda: K.act_encode(k13(), d, z, 8, False, bad=counter)[0],
                "K27": lambda: K.epilogue_codes(y, bias, None, None, 1, d, z, 8, False, counter),
                "pool + K21": lambda: K.act_encode(K.maxpool2d(x, 3, 2, 1), d, z, 8, False,
                                                   bad=counter)[0],
                "K28": lambda: K.maxpool_codes(codes, 3, 2, 1),
            }
            same = bool(torch.equal(forms["K13 + K21"](), forms["K27"]())
                        and torch.equal(forms["pool + K21"](), forms["K28"]()))
            assert same and int(counter.item()) == 0, (same, int(counter.item()))
            us = measure(torch, forms, args.rounds)
        e_in, e_out = N * Cc * H * H, N * Cc * OH * OH
        p_in, p_out = N * Cp * H * H, N * Cp * OH * OH
        nbytes = {"K13 + K21": (4 + 4) * e_in + 4 * e_in + p_in, "K27": 4 * e_in + p_in,
                  "pool + K21": 4 * e_in + 4 * e_out + 4 * e_out + p_out, "K28": p_in + p_out}
        rows.append({"shape": name, "N": N, "outputs_identical": same, "us": us, "bytes": nbytes})
    print(json.dumps({"copy_tbs": copy_tbs, "copy_us": copy, "rows": rows}), flush=True)


def run_chain(i, args):
    import torch
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import drivers as D
    from shiftedscalequantization_amd import kernels as K
    from shiftedscalequantization_amd import quant as Q

    name, arch, grouped, front_of = CHAINS[i]
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(4205 + i)
    x = torch.randn(args.batch, 3, 224, 224, generator=torch.Generator().manual_seed(4305 + i)).cuda()
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
    stem = Q.stem_edges(qnn)[0][0]
    state = {"hook": None}

    def install(route):
        if state["hook"] is not None:
            state["hook"].remove()
            state["hook"] = None
        mode = {"carry_blocks": True} if route == "blocks" else {"carry_stem": True}
        plan = Q.enable_integer_inference(qnn, x[:8], grouped=grouped, **mode)
        if route == "stem-plan":
            state["hook"] = stem.register_forward_hook(lambda m, a, out: None)
        return plan

    def run():
        with torch.no_grad():
            return front(x)

    outs, plans, emitted, off_grid = {}, {}, {}, 0
    for route in ("blocks", "stem-plan", "stem"):
        plans[route] = install(route)
        outs[route] = K.materialize_epi(run()).clone()
        emitted[route] = Q.stem_carry_report(qnn)["calls"]
        off_grid += Q.integer_report(qnn)["off_grid"]
    same = bool(torch.equal(outs["stem"].view(torch.int32), outs["stem-plan"].view(torch.int32)))
    assert same and off_grid == 0 and list(emitted["stem"].values()) == [1], (same, off_grid, emitted)
    assert list(emitted["stem-plan"].values()) == [0] and emitted["blocks"] == {}
    gained = sorted(n for n, v in plans["stem"].items() if v == "int8" and plans["blocks"][n] != "int8")
    us = measure(torch, {r: run for r in ("blocks", "stem-plan", "stem")}, args.rounds, before=install)
    print(json.dumps({"chain": name, "N": args.batch, "stem_equals_stem_plan": same,
                      "max_abs_diff_vs_blocks": float((outs["stem"] - outs["blocks"]).abs().max()),
                      "max_abs_output": float(outs["blocks"].abs().max()),
                      "layers_gained": gained, "edge": Q.stem_carry_report(qnn)["edges"],
                      "us": us}), flush=True)


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
    chains = [child(["--chain", str(i)], args) for i in range(len(CHAINS))]
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(26)

    copy = kern["copy_tbs"]
    lines = [f"provenance {json.dumps(provenance())}",
             f"carried stem (carry_stem), batch {args.batch}, W{args.wbits}A{args.abits} with the "
             f"8-bit stem quantizer; median us over {args.rounds} rounds (min-max), forms alternated "
             f"round by round; float4 copy on this box {copy:.2f} TB/s, peak {PEAK_TBS:.0f} TB/s",
             "",
             "kernels: the bytes are the algorithmic ones (each tensor read or written once); outputs "
             "identical byte for byte on every shape",
             f"{'shape':<14}{'form':<12}{'us':>26} {'MB':>8} {'TB/s':>6} {'of peak':>8} {'of copy':>8} "
             f"{'pair/new':>9}"]
    for r in kern["rows"]:
        for form, ref in (("K13 + K21", None), ("K27", "K13 + K21"), ("pool + K21", None),
                          ("K28", "pool + K21")):
            t, nb = r["us"][form], r["bytes"][form]
            tbs = nb / t["median"] / 1e6
            ratio = f"{r['us'][ref]['median'] / t['median']:9.2f}" if ref else " " * 9
            lines.append(f"{r['shape']:<14}{form:<12}{cell(t)} {nb / 1e6:8.1f} {tbs:6.2f} "
                         f"{100 * tbs / PEAK_TBS:7.1f}% {100 * tbs / copy:7.1f}% {ratio}")
    lines += ["",
              "chains: stem and stem-plan outputs identical bit for bit on every chain, nothing off "
              "the grid",
              f"{'chain':<40}{'blocks us':>26}{'stem-plan us':>26}{'stem us':>26} {'saved':>8} "
              f"{'spread':>8} {'blk/stem':>8} {'clear':>6} {'plan part':>10} {'carry part':>10}"]
    for r in chains:
        b, p, s = r["us"]["blocks"], r["us"]["stem-plan"], r["us"]["stem"]
        saved, spread = b["median"] - s["median"], b["max"] - b["min"]
        lines.append(f"{r['chain']:<40}{cell(b)}{cell(p)}{cell(s)} {saved:8.1f} {spread:8.1f} "
                     f"{b['median'] / s['median']:8.2f} {'yes' if saved > spread else 'NO':>6} "
                     f"{b['median'] - p['median']:10.1f} {p['median'] - s['median']:10.1f}")
        lines.append(f"    edge {r['edge']}; layers gained by the plan {r['layers_gained']}; "
                     f"max |stem - blocks| {r['max_abs_diff_vs_blocks']:.3g} "
                     f"(max |output| {r['max_abs_output']:.3g})")
    lines.append("saved: blocks - stem medians; spread: the blocks route's max - min; clear: saved > "
                 "spread; plan part: blocks - stem-plan (the layers behind the pool moving to the "
                 "integer conv); carry part: stem-plan - stem (K27, K28 and the readers on codes)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
