"""What the two-digit weight operand (K23's WIDE instantiations: two int8 weight planes, eight
MFMAs per k step) costs against the centred int8 instantiation on a weight both hold, and
against the decoded fp32 route, at batch 64 and batch 8.

    python tools/int_infer_wide_rate.py [--batches 64,8] [--wbits 2] [--abits 4] [--rounds 7]
                                        [--out profiles/int_infer_wide_rate.txt]

Shapes: ResNet-18's four 3x3 body convs and its three 1x1 stride-2 downsample convs.  The weight
is W2 with a per-(co, ci) scale on the default shift targets (k in {31, 32, 33}, L = 32, |m| <= 99),
prepared twice: the int8 blob (SSQ_QCONV_WIDE=auto) and the wide blob (SSQ_QCONV_WIDE=1).  Forms,
alternated round by round in one process per (shape, batch):
    wide fp32 / int8 fp32 / decoded fp32      qconv on the wide blob / on the int8 blob / the
                                              project's fp32 conv (kernels.conv2d) of the decoded
                                              activation and W_hat
    wide codes / int8 codes / decoded codes   qconv_codes (bias + ReLU + act quantizer in the
                                              kernel) / the fp32 conv and the K13 bias + ReLU +
                                              act-quantizer pass
The two integer outputs are compared bit for bit before anything is timed.  Every sample is a
device-event time over enough back-to-back calls to fill >= 20 ms, after a warm-up of every
form; the table holds medians over the rounds with min-max.  The parent process never opens
the GPU: each (shape, batch) runs in a child under its own time limit, and the first failing
child ends the run.
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
TARGETS = (31 / 32, 33 / 32, 1.0)
KINDS = ("wide", "int8", "decoded")


def run_shape(i, N, args):
    import torch
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    name, H, Ci, Co, R, stride, pad = SHAPES[i]
    g = torch.Generator().manual_seed(5005 + i)
    alo, ahi = K.qrange(args.abits, False)
    whi = 2 ** args.wbits - 1
    assert whi * 33 <= 127, "the scaled weight must fit int8 as well"
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")

    da, za = 0.05, 0.0
    qa = torch.randint(alo, ahi + 1, (N, Ci, H, H), generator=g).float().cuda()
    xhat = (qa - za) * da
    codes, _ = K.act_encode(xhat, da, za, args.abits, False, bad=counter)
    qw = torch.randint(0, whi + 1, (Co, Ci, R, R), generator=g).float().cuda()
    zw = torch.randint(0, whi + 1, (Co,), generator=g).float().cuda()
    delta = (torch.rand(Co, generator=g) * 0.02 + 1e-3).cuda()
    t = torch.tensor(TARGETS, dtype=torch.float32)[torch.randint(0, 3, (Co, Ci), generator=g)].cuda()
    wscale = delta.view(-1, 1) * t
    what = (qw - zw.view(-1, 1, 1, 1)) * wscale.view(Co, Ci, 1, 1)
    packed, bad = K.pack_encode(what, zw, wscale.reshape(-1), True, None, args.wbits, 0, whi)
    assert bad == 0
    L, base, k = K.perci_grid(wscale, Co, Ci, 127)
    assert L == 32
    preps = {}
    for knob in ("auto", "1"):
        K.QCONV_WIDE = knob
        preps[knob] = K.qweight_prepare_scaled(packed, tuple(what.shape), zw, args.wbits, 0, kfac=k,
                                               wide=True)
        assert int(preps[knob].bad.item()) == 0
    K.QCONV_WIDE = "auto"
    assert preps["1"].wide and not preps["auto"].wide and preps["auto"].centred
    prep = {"wide": preps["1"], "int8": preps["auto"]}
    scale = ((torch.tensor([da], device="cuda") * base.cuda())
             / torch.tensor([float(L)], device="cuda")).contiguous()
    bias = (torch.randn(Co, generator=g) * 0.1).cuda()
    kw = dict(act_zp=za, act_bits=args.abits, act_sym=False)

    def fp32(kind):
        if kind == "decoded":
            return lambda: K.conv2d(xhat, what, stride, pad)
        return lambda: K.qconv(codes, prep[kind], scale, stride, pad, **kw)

    y = fp32("int8")()
    d_out = float(torch.clamp(y + bias.view(1, -1, 1, 1), min=0.0).max()) / (ahi - alo)
    dt, zt = torch.tensor([d_out], device="cuda"), torch.zeros(1, device="cuda")

    def emit(kind):
        if kind == "decoded":
            def f():
                with torch.no_grad():
                    return K.bias_act_quant(K.conv2d(xhat, what, stride, pad), bias, None, 1, dt, zt,
                                            args.abits, False)
            return f
        return lambda: K.qconv_codes(codes, prep[kind], scale, stride, pad, bias=bias, relu=1,
                                     out_delta=d_out, out_zp=0.0, out_bits=args.abits, bad=counter, **kw)

    forms = {f"{kind} {what_}": (fp32 if what_ == "fp32" else emit)(kind)
             for what_ in ("fp32", "codes") for kind in KINDS}
    same = (torch.equal(forms["wide fp32"]().view(torch.int32), forms["int8 fp32"]().view(torch.int32))
            and torch.equal(forms["wide codes"](), forms["int8 codes"]()))
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
    ap.add_argument("--batches", default="64,8")
    ap.add_argument("--wbits", type=int, default=2)
    ap.add_argument("--abits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=120, help="seconds per (shape, batch)")
    ap.add_argument("--shape", type=int, default=None, help="(child) run this shape only")
    ap.add_argument("--batch", type=int, default=None, help="(child) at this batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.shape is not None:
        return run_shape(args.shape, args.batch, args)
    rows = []
    for N in (int(b) for b in args.batches.split(",")):
        for i in range(len(SHAPES)):
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(i), "--batch", str(N),
                   "--wbits", str(args.wbits), "--abits", str(args.abits), "--rounds", str(args.rounds)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"shape {SHAPES[i][0]} at batch {N} failed (rc={r.returncode}); stopping")
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(24)

    lines = [f"provenance {json.dumps(provenance())}",
             f"K23 on a W{args.wbits} per-(co, ci) weight (L = 32, |m| <= 99) A{args.abits}: the wide blob "
             f"(two int8 digit planes, eight MFMAs per k step), the int8 blob (centred instantiation) and "
             f"the decoded fp32 route; median us per call over {args.rounds} rounds (min-max), forms "
             f"alternated round by round; wide and int8 outputs identical bit for bit on every shape"]
    for what in ("fp32", "codes"):
        for N in sorted({r["N"] for r in rows}, reverse=True):
            lines.append(f"{what + ' output, batch ' + str(N):<36}{'wide us':>24}{'int8 us':>24}"
                         f"{'decoded us':>24} {'wide/int8':>9} {'wide/dec':>9} {'spread us':>9}")
            for r in rows:
                if r["N"] != N:
                    continue
                w, c, d = (r["us"][f"{kind} {what}"] for kind in KINDS)
                lines.append(f"{r['shape']:<36}{cell(w)}{cell(c)}{cell(d)} "
                             f"{w['median'] / c['median']:9.3f} {w['median'] / d['median']:9.3f} "
                             f"{c['max'] - c['min']:9.1f}")
    lines.append("wide/int8, wide/dec: ratios of medians; spread: the int8 run's max - min.  decoded "
                 "codes: the fp32 conv and the K13 bias + ReLU + act-quantizer pass (two launches, fp32 "
                 "out), against one launch that stores int8 codes")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
