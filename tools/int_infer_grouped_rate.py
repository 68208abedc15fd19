"""Rate of the grouped / depthwise integer conv path (K21 ssq_act_encode + K25 / K26
ssq_qconv_i8_grouped_fwd) on MobileNetV2's depthwise convs and RegNetX-3200M's f.b convs at
batch 64, beside the decoded path of the same commit.

    python tools/int_infer_grouped_rate.py [--batch 64] [--wbits 2] [--abits 4] [--rounds 7]
                                           [--out profiles/int_infer_grouped_rate.txt]

Forms, alternated within each round in one process per shape:
    qconv        K25 / K26 alone, from int8 codes already encoded
    enc+qconv    K21 + K25 / K26 from the fp32 activation: what QuantModule's integer route runs
    decoded      kernels.conv2d(x_hat, W_hat) under no_grad, as QuantModule runs the decoded
                 path (K18 for depthwise, MIOpen for grouped), cudnn.deterministic on
    F.conv2d     plain torch on the same operands, cudnn.deterministic on
Every sample is a device-event time over enough back-to-back calls to fill >= 20 ms, after a
warm-up of every form; the table holds medians over the rounds.  Depthwise rows give the
kernel's algorithmic bytes (N*H*W*Cp codes in, 4*N*OH*OW*C out) over its time as a fraction of
the 8 TB/s HBM peak; grouped rows count 2*M*Co*Cig*R*S integer operations against the dense
int8 MFMA peak (5033 TOP/s), `window` being real k over the k the MFMA runs (the 16-aligned
channel window, the 64-k tail and the 16-row padding of Cog).
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
PEAK_HBM = 8.0e12

# (name, C, H, Co, R, stride, pad, groups)
SHAPES = [
    ("mbv2 dw 96 @112 /2", 96, 112, 96, 3, 2, 1, 96),
    ("mbv2 dw 144 @56", 144, 56, 144, 3, 1, 1, 144),
    ("mbv2 dw 192 @28", 192, 28, 192, 3, 1, 1, 192),
    ("mbv2 dw 384 @14", 384, 14, 384, 3, 1, 1, 384),
    ("mbv2 dw 960 @7", 960, 7, 960, 3, 1, 1, 960),
    ("rgx3.2 b 96 g2 @56", 96, 56, 96, 3, 1, 1, 2),
    ("rgx3.2 b 192 g4 @28", 192, 28, 192, 3, 1, 1, 4),
    ("rgx3.2 b 432 g9 @14", 432, 14, 432, 3, 1, 1, 9),
    ("rgx3.2 b 1008 g21 @7", 1008, 7, 1008, 3, 1, 1, 21),
    # not model layers: the 144 @56 plane at 1 and 25 taps (same fp32 store stream, 1/9 and
    # 25/9 of the loads and integer work) to tell the depthwise kernel's limiter
    ("probe dw 144 @56 1x1", 144, 56, 144, 1, 1, 0, 144),
    ("probe dw 144 @56 5x5", 144, 56, 144, 5, 1, 2, 144),
]


def rup(v, m):
    return (v + m - 1) // m * m


def mfma_k_share(C, Co, R, G):
    """Real multiply-adds over those the grouped kernel's weight MFMAs run."""
    Cig, Cog = C // G, Co // G
    Wc = max(rup((g + 1) * Cig, 16) - g * Cig // 16 * 16 for g in range(G))
    return (Cig * R * R * Cog) / (rup(R * R * Wc, 64) * rup(Cog, 16))


def run_shape(i, args):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    name, C, H, Co, R, stride, pad, G = SHAPES[i]
    N = args.batch
    g = torch.Generator().manual_seed(2005 + i)
    alo, ahi = K.qrange(args.abits, False)
    wlo, whi = K.qrange(args.wbits, False)
    qa = torch.randint(alo, ahi + 1, (N, C, H, H), generator=g).float().cuda()
    qw = torch.randint(wlo, whi + 1, (Co, C // G, R, R), generator=g).float().cuda()
    zw = torch.randint(wlo, whi + 1, (Co,), generator=g).float().cuda()
    d1 = (torch.rand(Co, generator=g) * 0.02 + 1e-3).cuda()
    da, za = 0.05, 0.0
    xhat = (qa - za) * da
    what = (qw - zw.view(-1, 1, 1, 1)) * d1.view(-1, 1, 1, 1)
    packed, bad = K.pack_encode(what, zw, d1, False, None, args.wbits, wlo, whi)
    assert bad == 0
    prep = K.qweight_prepare(packed, tuple(what.shape), zw, args.wbits, wlo, groups=G)
    kind = K.qconv_kind(prep)
    scale = (torch.tensor([da], device="cuda") * d1).contiguous()
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    codes, _ = K.act_encode(xhat, da, za, args.abits, False, bad=counter)
    akw = dict(groups=G, act_zp=za, act_bits=args.abits, act_sym=False)
    torch.backends.cudnn.deterministic = True

    def decoded():
        with torch.no_grad():
            return K.conv2d(xhat, what, stride, pad, 1, G)

    forms = {
        "qconv": lambda: K.qconv(codes, prep, scale, stride, pad, **akw),
        "enc+qconv": lambda: K.qconv(xhat, prep, scale, stride, pad, act_delta=da, bad=counter, **akw),
        "decoded": decoded,
        "F.conv2d": lambda: F.conv2d(xhat, what, None, stride, pad, 1, G),
    }
    y = forms["enc+qconv"]()
    ref = forms["F.conv2d"]()
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
    ops = 2.0 * N * OH * OH * Co * (C // G) * R * R
    nbytes = float(N * H * H * rup(C, 16) + 4 * N * OH * OH * Co)
    print(json.dumps({"shape": name, "kind": kind, "N": N, "C": C, "H": H, "Co": Co, "R": R,
                      "stride": stride, "groups": G, "ops": ops, "bytes": nbytes,
                      "k_share": 1.0 if kind == "depthwise" else mfma_k_share(C, Co, R, G),
                      "max_rel_diff_vs_fp32": rel,
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
             f"grouped / depthwise int8 conv path vs the decoded path, batch {args.batch}, "
             f"W{args.wbits}A{args.abits}; median us per call over {args.rounds} rounds (min-max); "
             f"HBM peak {PEAK_HBM / 1e12:.1f} TB/s, int8 MFMA peak {PEAK_TOPS:.0f} TOP/s",
             f"{'shape':<22}{'kind':<10} {'qconv us':>20} {'TB/s':>6} {'%HBM':>6} {'TOP/s':>7} "
             f"{'%peak':>6} {'window':>7}  {'enc+qconv us':>20}  {'decoded us':>20}  "
             f"{'F.conv2d us':>20}  {'dec/int':>8} {'dec/qconv':>9}"]

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(20)

    for r in rows:
        u = r["us"]
        q, e = u["qconv"]["median"], u["enc+qconv"]["median"]
        tbs = r["bytes"] / q / 1e6
        tops = r["ops"] / q / 1e6
        lines.append(f"{r['shape']:<22}{r['kind']:<10} {cell(u['qconv'])} {tbs:6.2f} "
                     f"{100 * tbs * 1e12 / PEAK_HBM:6.1f} {tops:7.1f} {100 * tops / PEAK_TOPS:6.2f} "
                     f"{r['k_share']:7.2f}  {cell(u['enc+qconv'])}  {cell(u['decoded'])}  "
                     f"{cell(u['F.conv2d'])}  {u['decoded']['median'] / e:8.2f} "
                     f"{u['decoded']['median'] / q:9.2f}")
    lines.append("dec/int, dec/qconv: decoded-path time over enc+qconv / qconv time (> 1: the "
                 "integer route is faster); TB/s: algorithmic bytes of qconv (codes in, fp32 out)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
