"""Rate of the integer conv path (K21 ssq_act_encode + K23 ssq_qconv_i8_fwd) on the ResNet-18
body shapes at batch 64, beside the fp32 convolution the decoded path runs today (F.conv2d on
the decoded weight, as PackedWeight does).

    python tools/int_infer_rate.py [--batch 64] [--wbits 2] [--abits 4] [--rounds 7]
                                   [--out profiles/int_infer_rate.txt]

Forms, alternated within each round in one process per shape:
    qconv        K23 alone, from int8 codes already encoded
    enc+qconv    K21 + K23 from the fp32 activation: what QuantModule's integer route runs
    fp32 det     F.conv2d(x_hat, W_hat) under cudnn.deterministic (main_imagenet.py's default)
    fp32 fast    the same with MIOpen free to pick its fastest solver
Every sample is a device-event time over enough back-to-back calls to fill >= 20 ms, after a
warm-up of every form; the table holds medians over the rounds.  TOP/s counts 2*M*Co*K integer
operations of the convolution (M = N*OH*OW, K = Ci*R*S) against the dense int8 MFMA peak
(2x the bf16 peak: 5033 TOP/s at 256 CUs x 4 SIMDs x 2048 op/clk x 2.4 GHz).
The parent process never opens the GPU: each shape runs in a child under its own time limit,
and the first failing child ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TOPS = 256 * 4 * 2048 * 2.4e9 / 1e12

# (name, Ci, H, Co, R, stride, pad)
SHAPES = [
    ("layer1 3x3", 64, 56, 64, 3, 1, 1),
    ("layer2 3x3", 128, 28, 128, 3, 1, 1),
    ("layer3 3x3", 256, 14, 256, 3, 1, 1),
    ("layer4 3x3", 512, 7, 512, 3, 1, 1),
    ("layer2 ds 1x1/2", 64, 56, 128, 1, 2, 0),
    ("layer3 ds 1x1/2", 128, 28, 256, 1, 2, 0),
    ("layer4 ds 1x1/2", 256, 14, 512, 1, 2, 0),
]


def run_shape(i, args):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    name, Ci, H, Co, R, stride, pad = SHAPES[i]
    N = args.batch
    g = torch.Generator().manual_seed(1005 + i)
    alo, ahi = K.qrange(args.abits, False)
    wlo, whi = K.qrange(args.wbits, False)
    qa = torch.randint(alo, ahi + 1, (N, Ci, H, H), generator=g).float().cuda()
    qw = torch.randint(wlo, whi + 1, (Co, Ci, R, R), generator=g).float().cuda()
    zw = torch.randint(wlo, whi + 1, (Co,), generator=g).float().cuda()
    d1 = (torch.rand(Co, generator=g) * 0.02 + 1e-3).cuda()
    da, za = 0.05, 0.0
    xhat = (qa - za) * da
    what = (qw - zw.view(-1, 1, 1, 1)) * d1.view(-1, 1, 1, 1)
    packed, bad = K.pack_encode(what, zw, d1, False, None, args.wbits, wlo, whi)
    assert bad == 0
    prep = K.qweight_prepare(packed, tuple(what.shape), zw, args.wbits, wlo)
    scale = (torch.tensor([da], device="cuda") * d1).contiguous()
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    codes, _ = K.act_encode(xhat, da, za, args.abits, False, bad=counter)
    akw = dict(act_zp=za, act_bits=args.abits, act_sym=False)

    def fp32(det):
        def f():
            torch.backends.cudnn.deterministic = det
            return F.conv2d(xhat, what, stride=stride, padding=pad)
        return f

    forms = {
        "qconv": lambda: K.qconv(codes, prep, scale, stride, pad, **akw),
        "enc+qconv": lambda: K.qconv(xhat, prep, scale, stride, pad, act_delta=da, bad=counter, **akw),
        "fp32 det": fp32(True),
        "fp32 fast": fp32(False),
    }
    y = forms["enc+qconv"]()
    ref = forms["fp32 fast"]()
    rel = float((y - ref).abs().max() / ref.abs().max())
    assert int(counter.item()) == 0 and rel < 1e-4, (int(counter.item()), rel)

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
    OH = (H + 2 * pad - R) // stride + 1
    ops = 2.0 * N * OH * OH * Co * Ci * R * R
    print(json.dumps({"shape": name, "N": N, "Ci": Ci, "H": H, "Co": Co, "R": R, "stride": stride,
                      "ops": ops, "max_rel_diff_vs_fp32": rel,
                      "us": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                             for k, v in times.items()}}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--wbits", type=int, default=2)
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
               "--wbits", str(args.wbits), "--abits", str(args.abits), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"shape {SHAPES[i][0]} failed (rc={r.returncode}); stopping")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance
    lines = [f"provenance {json.dumps(provenance())}",
             f"int8 conv path vs fp32 conv, batch {args.batch}, W{args.wbits}A{args.abits}; "
             f"median us per call over {args.rounds} rounds (min-max); int8 MFMA peak "
             f"{PEAK_TOPS:.0f} TOP/s",
             f"{'shape':<18}{'GOP':>7}  {'qconv us':>20} {'TOP/s':>7} {'%peak':>6}  "
             f"{'enc+qconv us':>20} {'TOP/s':>7}  {'fp32 det us':>20}  {'fp32 fast us':>20}  "
             f"{'det/int':>8} {'fast/int':>8}"]

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(20)

    for r in rows:
        u = r["us"]
        q, e = u["qconv"]["median"], u["enc+qconv"]["median"]
        lines.append(f"{r['shape']:<18}{r['ops'] / 1e9:7.2f}  {cell(u['qconv'])} {r['ops'] / q / 1e6:7.1f} "
                     f"{100 * r['ops'] / q / 1e6 / PEAK_TOPS:6.2f}  {cell(u['enc+qconv'])} "
                     f"{r['ops'] / e / 1e6:7.1f}  {cell(u['fp32 det'])}  {cell(u['fp32 fast'])}  "
                     f"{u['fp32 det']['median'] / e:8.2f} {u['fp32 fast']['median'] / e:8.2f}")
    lines.append("det/int, fast/int: fp32 conv time over enc+qconv time (> 1: the integer route is faster)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
