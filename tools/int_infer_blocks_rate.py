"""What carrying int8 codes across block tails and block edges saves: a run of consecutive
residual blocks timed end to end with codes carried inside the blocks only (carry=True, the
parent route: its kernels are unchanged) and across the tails and edges too (carry_blocks=True),
batch 64.

    python tools/int_infer_blocks_rate.py [--batch 64] [--wbits 2] [--abits 4] [--rounds 7]
                                          [--out profiles/int_infer_blocks_rate.txt]

Routes, alternated round by round in one process per chain:
    carry        per block: K21 on the fp32 block input (once per reader) -> qconv_codes ... ->
                 qconv (the last conv, fp32) -> K13 with the residual, the block activation and
                 the block act quantizer (kernels.bias_act_quant) -> fp32 block output
    blocks       the block input arrives as codes; the last conv is qconv_codes with the
                 residual (the carried input, or the fp32 output of the proj conv) and emits
                 the next block's codes: the steady state of a carried run
    blocks+ends  `blocks` entered from an fp32 tensor (K21 per reader, fp32 residual) and left
                 through act_decode: what an isolated run of this length pays at its two ends
The fp32 tensor the `blocks` output stands for is compared bit for bit with the `carry` output
before anything is timed.  Every sample is a device-event time over enough back-to-back calls
to fill >= 50 ms, after a warm-up of every form; the table holds medians over the rounds with
min-max.  The parent process never opens the GPU: each chain runs in a child under its own
time limit, and the first failing child ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def basic(c):          # ResNet-18 block, identity residual
    return dict(convs=[(c, c, 3, 1, 1, 1, 1), (c, c, 3, 1, 1, 1, 0)], proj=None, identity=True, act=1)


def inverted(c, h):    # MobileNetV2 block with a residual connection: no activation after the add
    return dict(convs=[(c, h, 1, 1, 0, 1, 2), (h, h, 3, 1, 1, h, 2), (h, c, 1, 1, 0, 1, 0)],
                proj=None, identity=True, act=0)


def regnet(ci, c, stride, gw):
    return dict(convs=[(ci, c, 1, 1, 0, 1, 1), (c, c, 3, stride, 1, c // gw, 1), (c, c, 1, 1, 0, 1, 0)],
                proj=(ci, c, 1, stride, 0, 1, 0) if (ci != c or stride != 1) else None,
                identity=ci == c and stride == 1, act=1)


# (name, class of shapes, input channels, input plane H, blocks)
CHAINS = [
    ("r18 layer1 2 blocks 64 @56", "dense 3x3 tails", 64, 56, [basic(64)] * 2),
    ("r18 layer2 2 blocks 128 @28", "dense 3x3 tails", 128, 28, [basic(128)] * 2),
    ("r18 layer3 2 blocks 256 @14", "dense 3x3 tails", 256, 14, [basic(256)] * 2),
    ("r18 layer4 2 blocks 512 @7", "dense 3x3 tails", 512, 7, [basic(512)] * 2),
    ("mbv2 3 blocks 24/144 @56", "1x1 project tails", 24, 56, [inverted(24, 144)] * 3),
    ("mbv2 3 blocks 64/384 @14", "1x1 project tails", 64, 14, [inverted(64, 384)] * 3),
    ("mbv2 3 blocks 160/960 @7", "1x1 project tails", 160, 7, [inverted(160, 960)] * 3),
    ("rgx3.2 s3.b1 -> s3.b2", "1x1 tails, proj + identity", 192, 28,
     [regnet(192, 432, 2, 48), regnet(432, 432, 1, 48)]),
]


def run_chain(i, args):
    import torch
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    name, _, C0, H, blocks = CHAINS[i]
    N, bits = args.batch, args.abits
    g = torch.Generator().manual_seed(4005 + i)
    alo, ahi = K.qrange(bits, False)
    wlo, whi = K.qrange(args.wbits, False)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.backends.cudnn.deterministic = True

    def make_conv(spec, inq):
        Ci, Co, R, stride, pad, G, act = spec
        qw = torch.randint(wlo, whi + 1, (Co, Ci // G, R, R), generator=g).float().cuda()
        zw = torch.randint(wlo, whi + 1, (Co,), generator=g).float().cuda()
        d1 = (torch.rand(Co, generator=g) * 0.02 + 1e-3).cuda()
        what = (qw - zw.view(-1, 1, 1, 1)) * d1.view(-1, 1, 1, 1)
        packed, bad = K.pack_encode(what, zw, d1, False, None, args.wbits, wlo, whi)
        assert bad == 0
        prep = K.qweight_prepare(packed, tuple(what.shape), zw, args.wbits, wlo, groups=G)
        return dict(prep=prep, scale=(torch.tensor([inq[0]], device="cuda") * d1).contiguous(),
                    bias=(torch.randn(Co, generator=g) * 0.1).cuda(), stride=stride, pad=pad,
                    act=act, Co=Co, da=inq[0],
                    kw=dict(groups=G, act_zp=inq[1], act_bits=bits, act_sym=False))

    def grid(t, act):
        """A min-max act quantizer over t: (delta, zero point); zero point 0 after a ReLU."""
        lo, hi = (0.0, float(t.max())) if act else (float(t.min()), float(t.max()))
        d = max(hi - lo, 1e-6) / (ahi - alo)
        return d, float(min(max(round(-lo / d), alo), ahi))

    def conv(lay, x):
        return K.qconv(x, lay["prep"], lay["scale"], lay["stride"], lay["pad"],
                       act_delta=lay["da"], bad=counter, **lay["kw"])

    def conv_codes(lay, x, q, act, residual=None):
        c = K.qconv_codes(x, lay["prep"], lay["scale"], lay["stride"], lay["pad"],
                          act_delta=lay["da"], bias=lay["bias"], relu=act, out_delta=q[0],
                          out_zp=q[1], out_bits=bits, bad=counter, residual=residual, **lay["kw"])
        n, h, w, _ = c.shape
        return K.carried(c, (n, lay["Co"], h, w), q[0], q[1], bits, False)

    def k13(y, bias, res, act, q):
        return K.bias_act_quant(y, bias, res, act, q["dt"], q["zt"], bits, False)

    def qt(q):
        return dict(dt=torch.tensor([q[0]], device="cuda"), zt=torch.tensor([q[1]], device="cuda"))

    # build the layers and calibrate every act quantizer on the fp32 route
    inq = (0.05, 0.0)
    qa = torch.randint(alo, ahi + 1, (N, C0, H, H), generator=g).float().cuda()
    x0 = ((qa - inq[1]) * inq[0]).contiguous()
    B, x = [], x0
    with torch.no_grad():
        for spec in blocks:
            blk = dict(act=spec["act"], identity=spec["identity"], inq=inq, convs=[], proj=None)
            h, hq = x, inq
            for cs in spec["convs"][:-1]:
                lay = make_conv(cs, hq)
                y = conv(lay, h)
                t = torch.clamp(y + lay["bias"].view(1, -1, 1, 1), min=0.0)
                lay["q"] = grid(torch.clamp(t, max=6.0) if cs[6] == 2 else t, cs[6])
                lay["qt"] = qt(lay["q"])
                h, hq = k13(y, lay["bias"], None, cs[6], lay["qt"]), lay["q"]
                blk["convs"].append(lay)
            last = make_conv(spec["convs"][-1], hq)
            blk["convs"].append(last)
            res = x if spec["identity"] else None
            if spec["proj"] is not None:
                blk["proj"] = make_conv(spec["proj"], inq)
                res = K.bias_act(conv(blk["proj"], x), blk["proj"]["bias"], None, 0)
            raw = conv(last, h)
            t = raw + last["bias"].view(1, -1, 1, 1) + (0 if res is None else res)
            blk["q"] = grid(torch.clamp(t, min=0.0) if spec["act"] else t, spec["act"])
            blk["qt"] = qt(blk["q"])
            x, inq = k13(raw, last["bias"], res, spec["act"], blk["qt"]), blk["q"]
            B.append(blk)
    codes0, _ = K.act_encode(x0, B[0]["inq"][0], B[0]["inq"][1], bits, False, bad=counter)
    codes0 = K.carried(codes0, tuple(x0.shape), B[0]["inq"][0], B[0]["inq"][1], bits, False)

    def block(blk, x, emit):
        h = x
        for lay in blk["convs"][:-1]:
            h = conv_codes(lay, h, lay["q"], lay["act"])
        last = blk["convs"][-1]
        res = x if blk["identity"] else None
        if blk["proj"] is not None:
            res = K.bias_act(conv(blk["proj"], x), blk["proj"]["bias"], None, 0)
        if emit:
            return conv_codes(last, h, blk["q"], blk["act"], residual=res)
        return k13(conv(last, h), last["bias"], res, blk["act"], blk["qt"])

    def route(x, emit):
        with torch.no_grad():
            for blk in B:
                x = block(blk, x, emit)
            return x

    forms = {"carry": lambda: route(x0, False), "blocks": lambda: route(codes0, True),
             "blocks+ends": lambda: K.materialize_epi(route(x0, True))}
    a, b, c = forms["carry"](), K.materialize_epi(forms["blocks"]()), forms["blocks+ends"]()
    same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32))
                and torch.equal(a.view(torch.int32), c.view(torch.int32)))
    assert same and int(counter.item()) == 0, (same, int(counter.item()))

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
        reps[k] = max(5, int(50e3 / max(sample(f, 10), 1.0)))
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
        print(rows[-1], flush=True)
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(24)

    lines = [f"provenance {json.dumps(provenance())}",
             f"runs of residual blocks, codes carried inside the blocks (carry, the parent route) "
             f"and across tails and block edges (blocks), batch {args.batch}, "
             f"W{args.wbits}A{args.abits}; median us per run over {args.rounds} rounds (min-max), "
             f"routes alternated round by round; outputs identical bit for bit on every chain",
             f"{'chain':<30}{'carry us':>24}{'blocks us':>24}{'blocks+ends us':>24} {'saved':>8} "
             f"{'spread':>8} {'car/blk':>8} {'clear':>6} {'ends clear':>10}"]
    for r, ch in zip(rows, CHAINS):
        u, c, e = r["us"]["carry"], r["us"]["blocks"], r["us"]["blocks+ends"]
        saved, spread = u["median"] - c["median"], u["max"] - u["min"]
        lines.append(f"{r['chain']:<30}{cell(u)}{cell(c)}{cell(e)} {saved:8.1f} {spread:8.1f} "
                     f"{u['median'] / c['median']:8.2f} {'yes' if saved > spread else 'NO':>6} "
                     f"{'yes' if u['median'] - e['median'] > spread else 'NO':>10}   [{ch[1]}]")
    lines.append("saved: carry - blocks medians; spread: the carry route's max - min; clear: saved > "
                 "spread; ends clear: the same with blocks+ends in place of blocks")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
