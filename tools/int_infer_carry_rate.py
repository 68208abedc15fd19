"""What carrying int8 codes between integer layers saves: a chain of layers timed end to end
on the uncarried integer route and on the carried one, batch 64.

    python tools/int_infer_carry_rate.py [--batch 64] [--wbits 2] [--abits 4] [--rounds 7]
                                         [--out profiles/int_infer_carry_rate.txt]

Routes, alternated round by round in one process per chain, both starting from the first
layer's int8 codes and ending in the last layer's fp32 output:
    uncarried    qconv -> K13 (bias + activation + act quantizer, kernels.bias_act_quant) ->
                 K21 (inside the next qconv) -> qconv ...: what QuantModule runs without carry
    carried      qconv_codes -> ... -> qconv: the producers emit the next layer's codes
The two routes' outputs are compared bit for bit before anything is timed.  Chains with a
depthwise layer also time that layer alone from the fp32 activation the previous layer leaves
(`dw decoded`: kernels.conv2d + K13, the decoded path; `dw uncarried`: K21 + K25 + K13) and
from codes (`dw carried`: K25 emitting codes).
Every sample is a device-event time over enough back-to-back calls to fill >= 20 ms, after a
warm-up of every form; the table holds medians over the rounds with min-max.  The parent
process never opens the GPU: each chain runs in a child under its own time limit, and the
first failing child ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, input plane H, [(Ci, Co, R, stride, pad, groups, act), ...]); act 1 ReLU, 2 ReLU6
CHAINS = [
    ("r18 layer1 64 @56 3x3 -> 3x3", 56, [(64, 64, 3, 1, 1, 1, 1), (64, 64, 3, 1, 1, 1, 0)]),
    ("r18 layer2 128 @28 3x3 -> 3x3", 28, [(128, 128, 3, 1, 1, 1, 1), (128, 128, 3, 1, 1, 1, 0)]),
    ("r18 layer3 256 @14 3x3 -> 3x3", 14, [(256, 256, 3, 1, 1, 1, 1), (256, 256, 3, 1, 1, 1, 0)]),
    ("r18 layer4 512 @7 3x3 -> 3x3", 7, [(512, 512, 3, 1, 1, 1, 1), (512, 512, 3, 1, 1, 1, 0)]),
    ("mbv2 24 -> 144 dw -> 24 @56", 56,
     [(24, 144, 1, 1, 0, 1, 2), (144, 144, 3, 1, 1, 144, 2), (144, 24, 1, 1, 0, 1, 0)]),
    ("mbv2 64 -> 384 dw -> 64 @14", 14,
     [(64, 384, 1, 1, 0, 1, 2), (384, 384, 3, 1, 1, 384, 2), (384, 64, 1, 1, 0, 1, 0)]),
    ("mbv2 160 -> 960 dw -> 160 @7", 7,
     [(160, 960, 1, 1, 0, 1, 2), (960, 960, 3, 1, 1, 960, 2), (960, 160, 1, 1, 0, 1, 0)]),
    ("rgx3.2 s3.b1 a -> b -> c", 28,
     [(192, 432, 1, 1, 0, 1, 1), (432, 432, 3, 2, 1, 9, 1), (432, 432, 1, 1, 0, 1, 0)]),
]


def run_chain(i, args):
    import torch
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    name, H, layers = CHAINS[i]
    N = args.batch
    g = torch.Generator().manual_seed(3005 + i)
    alo, ahi = K.qrange(args.abits, False)
    wlo, whi = K.qrange(args.wbits, False)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.backends.cudnn.deterministic = True

    da, za = 0.05, 0.0
    qa = torch.randint(alo, ahi + 1, (N, layers[0][0], H, H), generator=g).float().cuda()
    codes0, _ = K.act_encode((qa - za) * da, da, za, args.abits, False, bad=counter)
    L = []          # per layer: prepared weight, scale, bias, geometry, its input / output quantizer
    x = codes0
    for (Ci, Co, R, stride, pad, G, act) in layers:
        qw = torch.randint(wlo, whi + 1, (Co, Ci // G, R, R), generator=g).float().cuda()
        zw = torch.randint(wlo, whi + 1, (Co,), generator=g).float().cuda()
        d1 = (torch.rand(Co, generator=g) * 0.02 + 1e-3).cuda()
        what = (qw - zw.view(-1, 1, 1, 1)) * d1.view(-1, 1, 1, 1)
        packed, bad = K.pack_encode(what, zw, d1, False, None, args.wbits, wlo, whi)
        assert bad == 0
        prep = K.qweight_prepare(packed, tuple(what.shape), zw, args.wbits, wlo, groups=G)
        scale = (torch.tensor([da], device="cuda") * d1).contiguous()
        bias = (torch.randn(Co, generator=g) * 0.1).cuda()
        kw = dict(groups=G, act_zp=za, act_bits=args.abits, act_sym=False)
        y = K.qconv(x, prep, scale, stride, pad, act_delta=da, bad=counter, **kw)
        lay = dict(prep=prep, scale=scale, bias=bias, stride=stride, pad=pad, G=G, act=act, kw=kw,
                   da=da, what=what)
        L.append(lay)
        if len(L) < len(layers):
            # this layer's act quantizer: a min-max grid over its own activation
            t = torch.clamp(y + bias.view(1, -1, 1, 1), min=0.0)
            t = torch.clamp(t, max=6.0) if act == 2 else t
            d_out = float(t.max()) / (ahi - alo)
            lay["d"], lay["z"] = d_out, 0.0
            lay["dt"] = torch.tensor([d_out], device="cuda")
            lay["zt"] = torch.zeros(1, device="cuda")
            x = K.bias_act_quant(y, bias, None, act, lay["dt"], lay["zt"], args.abits, False)
            da, za = d_out, 0.0

    def k13(lay, y):
        return K.bias_act_quant(y, lay["bias"], None, lay["act"], lay["dt"], lay["zt"],
                                args.abits, False)

    def conv(lay, x):
        return K.qconv(x, lay["prep"], lay["scale"], lay["stride"], lay["pad"],
                       act_delta=lay["da"], bad=counter, **lay["kw"])

    def conv_codes(lay, x):
        return K.qconv_codes(x, lay["prep"], lay["scale"], lay["stride"], lay["pad"],
                             act_delta=lay["da"], bias=lay["bias"], relu=lay["act"],
                             out_delta=lay["d"], out_zp=lay["z"], out_bits=args.abits,
                             bad=counter, **lay["kw"])

    def uncarried():
        with torch.no_grad():
            x = codes0
            for lay in L[:-1]:
                x = k13(lay, conv(lay, x))
            return conv(L[-1], x)

    def carried():
        x = codes0
        for lay in L[:-1]:
            x = conv_codes(lay, x)
        return conv(L[-1], x)

    forms = {"uncarried": uncarried, "carried": carried}
    a, b = uncarried(), carried()
    same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    assert same and int(counter.item()) == 0, (same, int(counter.item()))

    dw = [lay for lay in L[:-1] if lay["G"] > 1 and lay["what"].shape[1] == 1]
    if dw:
        lay = dw[0]
        x_fp = k13(L[0], conv(L[0], codes0))                 # what the expand layer leaves
        x_codes = conv_codes(L[0], codes0)

        def dw_decoded():
            with torch.no_grad():
                return k13(lay, K.conv2d(x_fp, lay["what"], lay["stride"], lay["pad"], 1, lay["G"]))

        def dw_uncarried():
            with torch.no_grad():
                return k13(lay, conv(lay, x_fp))

        forms.update({"dw decoded": dw_decoded, "dw uncarried": dw_uncarried,
                      "dw carried": lambda: conv_codes(lay, x_codes)})

    def sample(f, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / reps          # us per call

    reps = {}
    for k, f in forms.items():                         # warm-up, then size the window
        sample(f, 10)
        reps[k] = max(5, int(20e3 / max(sample(f, 10), 1.0)))
    times = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, f in forms.items():
            times[k].append(sample(f, reps[k]))
    print(json.dumps({"chain": name, "N": N, "outputs_identical": same,
                      "us": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                             for k, v in times.items()}}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--wbits", type=int, default=2)
    ap.add_argument("--abits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=120, help="seconds per chain")
    ap.add_argument("--chain", type=int, default=None, help="(child) run this chain only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.chain is not None:
        return run_chain(args.chain, args)
    rows = []
    for i in range(len(CHAINS)):
        cmd = [sys.executable, os.path.abspath(__file__), "--chain", str(i), "--batch", str(args.batch),
               "--wbits", str(args.wbits), "--abits", str(args.abits), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"chain {CHAINS[i][0]} failed (rc={r.returncode}); stopping")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(22)

    lines = [f"provenance {json.dumps(provenance())}",
             f"integer route with and without carried codes, batch {args.batch}, "
             f"W{args.wbits}A{args.abits}; median us per chain over {args.rounds} rounds (min-max), "
             f"routes alternated round by round; outputs identical bit for bit on every chain",
             f"{'chain':<32}{'uncarried us':>22}{'carried us':>22} {'saved us':>9} {'spread us':>9} "
             f"{'unc/car':>8} {'clear':>6}"]
    for r in rows:
        u, c = r["us"]["uncarried"], r["us"]["carried"]
        saved, spread = u["median"] - c["median"], u["max"] - u["min"]
        lines.append(f"{r['chain']:<32}{cell(u)}{cell(c)} {saved:9.1f} {spread:9.1f} "
                     f"{u['median'] / c['median']:8.2f} {'yes' if saved > spread else 'NO':>6}")
    lines.append("saved: uncarried - carried medians; spread: the uncarried route's max - min; "
                 "clear: saved > spread")
    lines.append(f"{'depthwise layer alone':<32}{'dw decoded us':>22}{'dw uncarried us':>22}"
                 f"{'dw carried us':>22} {'dec/unc':>8} {'dec/car':>8}")
    for r in rows:
        if "dw decoded" in r["us"]:
            d, u, c = (r["us"][k] for k in ("dw decoded", "dw uncarried", "dw carried"))
            lines.append(f"{r['chain']:<32}{cell(d)}{cell(u)}{cell(c)} "
                         f"{d['median'] / u['median']:8.2f} {d['median'] / c['median']:8.2f}")
    lines.append("dw decoded: kernels.conv2d (K18) + K13 from fp32; dw uncarried: K21 + K25 + K13 "
                 "from fp32; dw carried: K25 emitting codes, from codes; dec/unc, dec/car > 1: the "
                 "integer form is faster than the decoded path")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
