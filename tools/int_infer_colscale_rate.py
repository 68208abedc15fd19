"""What the centred instantiation of the int8 conv (K23 without the window-sum MFMA and the
0/1-row traffic) saves on a column-scaled weight's blob, against the shift-and-correct
instantiation on the SAME blob (cwz = 0 there, so both give the same bits), batch 64.

    python tools/int_infer_colscale_rate.py [--batch 64] [--wbits 2] [--level 32] [--abits 4]
                                            [--rounds 7]
                                            [--out profiles/int_infer_colscale_rate.txt]

Shapes: ResNet-18's four 3x3 body convs and its three 1x1 stride-2 downsample convs.  Forms,
alternated round by round in one process per shape, all from the layer's int8 codes:
    sa fp32 / centred fp32      qconv: ssq_qconv_i8_fwd / ssq_qconv_i8_centred_fwd
    sa codes / centred codes    qconv_codes (bias + ReLU + act quantizer in the kernel):
                                ssq_qconv_i8_codes_fwd / ssq_qconv_i8_centred_codes_fwd
(kernels.QCONV_CENTRED, the SSQ_QCONV_CENTRED knob, switched between calls.)  The outputs of
the two instantiations are compared bit for bit before anything is timed.  Every sample is a
device-event time over enough back-to-back calls to fill >= 20 ms, after a warm-up of every
form; the table holds medians over the rounds with min-max.  The parent process never opens
the GPU: each shape runs in a child under its own time limit, and the first failing child ends
the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, input plane H, Ci, Co, R, stride, pad)
SHAPES = [
    ("r18 layer1 3x3 64 @56", 56, 64, 64, 3, 1, 1),
    ("r18 layer2 3x3 128 @28", 28, 128, 128, 3, 1, 1),
    ("r18 layer3 3x3 256 @14", 14, 256, 256, 3, 1, 1),
    ("r18 layer4 3x3 512 @7", 7, 512, 512, 3, 1, 1),
    ("r18 layer2 ds 1x1 64->128 @56/2", 56, 64, 128, 1, 2, 0),
    ("r18 layer3 ds 1x1 128->256 @28/2", 28, 128, 256, 1, 2, 0),
    ("r18 layer4 ds 1x1 256->512 @14/2", 14, 256, 512, 1, 2, 0),
]


def run_shape(i, args):
    import torch
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    name, H, Ci, Co, R, stride, pad = SHAPES[i]
    N, L = args.batch, args.level
    g = torch.Generator().manual_seed(4005 + i)
    alo, ahi = K.qrange(args.abits, False)
    whi = 2 ** args.wbits - 1
    assert whi * L <= 127, "the scaled weight must fit int8"
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")

    da, za = 0.05, 0.0
    qa = torch.randint(alo, ahi + 1, (N, Ci, H, H), generator=g).float().cuda()
    codes, _ = K.act_encode((qa - za) * da, da, za, args.abits, False, bad=counter)
    qw = torch.randint(0, whi + 1, (Co, Ci, R, R), generator=g).float().cuda()
    zw = torch.randint(0, whi + 1, (Co,), generator=g).float().cuda()
    d1 = (torch.rand(Co, generator=g) * 0.02 + 1e-3).cuda()
    k = torch.randint(1, L + 1, (Ci * R * R,), generator=g, dtype=torch.int32)
    k[0], k[-1] = 1, L
    c = (k.float() / float(L)).cuda()
    what = ((qw - zw.view(-1, 1, 1, 1)) * d1.view(-1, 1, 1, 1)) * c.view(1, Ci, R, R)
    packed, bad = K.pack_encode(what, zw, d1, False, c, args.wbits, 0, whi)
    assert bad == 0
    grid = K.colscale_grid(c)
    assert grid is not None and grid[0] == L and torch.equal(grid[1], k)
    prep = K.qweight_prepare(packed, tuple(what.shape), zw, args.wbits, 0, kcol=k)
    assert prep.centred and int(prep.bad.item()) == 0
    scale = ((torch.tensor([da], device="cuda") * d1) / torch.tensor([float(L)], device="cuda")).contiguous()
    bias = (torch.randn(Co, generator=g) * 0.1).cuda()
    kw = dict(act_zp=za, act_bits=args.abits, act_sym=False)

    def fp32(centred):
        def f():
            K.QCONV_CENTRED = centred
            return K.qconv(codes, prep, scale, stride, pad, **kw)
        return f

    y = fp32(True)()
    d_out = float(torch.clamp(y + bias.view(1, -1, 1, 1), min=0.0).max()) / (ahi - alo)

    def emit(centred):
        def f():
            K.QCONV_CENTRED = centred
            return K.qconv_codes(codes, prep, scale, stride, pad, bias=bias, relu=1, out_delta=d_out,
                                 out_zp=0.0, out_bits=args.abits, bad=counter, **kw)
        return f

    forms = {"sa fp32": fp32(False), "centred fp32": fp32(True),
             "sa codes": emit(False), "centred codes": emit(True)}
    same = (torch.equal(forms["sa fp32"]().view(torch.int32), forms["centred fp32"]().view(torch.int32))
            and torch.equal(forms["sa codes"](), forms["centred codes"]()))
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
    for n, f in forms.items():                         # warm-up, then size the window
        sample(f, 10)
        reps[n] = max(5, int(20e3 / max(sample(f, 10), 1.0)))
    times = {n: [] for n in forms}
    for _ in range(args.rounds):
        for n, f in forms.items():
            times[n].append(sample(f, reps[n]))
    print(json.dumps({"shape": name, "N": N, "outputs_identical": bool(same),
                      "us": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                             for n, v in times.items()}}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--wbits", type=int, default=2)
    ap.add_argument("--level", type=int, default=32)
    ap.add_argument("--abits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=120, help="seconds per shape")
    ap.add_argument("--shape", type=int, default=None, help="(child) run this shape only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.shape is not None:
        return run_shape(args.shape, args)
    rows = []
    for i in range(len(SHAPES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(i), "--batch", str(args.batch),
               "--wbits", str(args.wbits), "--level", str(args.level), "--abits", str(args.abits),
               "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"shape {SHAPES[i][0]} failed (rc={r.returncode}); stopping")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(22)

    lines = [f"provenance {json.dumps(provenance())}",
             f"int8 conv on a column-scaled weight's centred blob, batch {args.batch}, "
             f"W{args.wbits} L{args.level} A{args.abits}; median us per call over {args.rounds} rounds "
             f"(min-max), instantiations alternated round by round; outputs identical bit for bit "
             f"on every shape"]
    for what in ("fp32", "codes"):
        lines.append(f"{what + ' output':<36}{'sa us':>22}{'centred us':>22} {'saved us':>9} "
                     f"{'spread us':>9} {'sa/cen':>7} {'keep':>8}")
        for r in rows:
            s, c = r["us"][f"sa {what}"], r["us"][f"centred {what}"]
            saved, spread = s["median"] - c["median"], s["max"] - s["min"]
            keep = "SA" if c["median"] > s["median"] + spread else "centred"
            lines.append(f"{r['shape']:<36}{cell(s)}{cell(c)} {saved:9.1f} {spread:9.1f} "
                         f"{s['median'] / c['median']:7.3f} {keep:>8}")
    lines.append("sa: the shift-and-correct instantiation (five MFMAs per k step, the parent's kernel) "
                 "on the same blob; saved: sa - centred medians; spread: the sa run's max - min; keep: "
                 "centred unless its median is above the sa median by more than the sa spread")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
