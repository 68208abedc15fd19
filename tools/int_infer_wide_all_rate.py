"""What the wide operand costs and saves on the kernels `wide_all` adds it to, batch 64.

    python tools/int_infer_wide_all_rate.py [--batch 64] [--rounds 7]
                                            [--out profiles/int_infer_wide_all_rate.txt]

(a) RegNetX-3200M's grouped 3x3 convs at W4 / L = 32 per-(co, ci) scales (|m| up to 495), A8, from the
    layer's int8 codes to the next layer's int8 codes:
        wide     ssq_qconv_i8_grouped_wide_codes_fwd on the two-plane blob
        int8     ssq_qconv_i8_grouped_codes_fwd on a plain int8 blob of the same shape (K26 as it
                 stands: the difference is the price of the second digit)
        decoded  what such a layer runs without `wide_all`: act_decode, the library's grouped conv on
                 the decoded fp32 weight, the K13 epilogue with the act quantizer, K21
    and the fp32-output forms of the two integer kernels.  wide and decoded are compared (codes that
    differ, of all) before anything is timed; they are not bit-equal (the library conv's summation).
(b) The chain s3.b1 -> s3.b2 of RegNetX-3200M with every weight scaled per (co, ci) at W4:
        wide_all  codes carried through both blocks (1x1 convs on K23's wide form, the grouped 3x3 on
                  K26's, the tails with their residual emitting the next block's codes)
        parent    the grouped 3x3 on the decoded path, hence no carried edge in the block: K21 + the
                  wide 1x1 + K13 per dense conv, library conv + K13 for the grouped one
(c) The head, K29 + K30 on the wide blob (W8 fc, |m| up to 8415; both image tiles), against the
    decoded head (act_decode + mean + the fp32 linear on the decoded weight): ResNet-18 (512 @ 7x7)
    and RegNetX-600M (528 @ 7x7), 1000 classes.

Every sample is a device-event time over enough back-to-back calls to fill >= 50 ms, after a
warm-up of every form, the forms alternated round by round in one process per part; the tables hold
medians over the rounds with min-max.  The parent process never opens the GPU: each part runs in a
child under its own time limit, and the first failing child ends the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from int_infer_stem_rate import measure  # noqa: E402

# (name, C, input plane H, stride, groups): 48 channels per group
GROUPED = [
    ("rgx3.2 s1.b1 96 g2 @112/2", 96, 112, 2, 2), ("rgx3.2 s1 96 g2 @56", 96, 56, 1, 2),
    ("rgx3.2 s2.b1 192 g4 @56/2", 192, 56, 2, 4), ("rgx3.2 s2 192 g4 @28", 192, 28, 1, 4),
    ("rgx3.2 s3.b1 432 g9 @28/2", 432, 28, 2, 9), ("rgx3.2 s3 432 g9 @14", 432, 14, 1, 9),
    ("rgx3.2 s4.b1 1008 g21 @14/2", 1008, 14, 2, 21), ("rgx3.2 s4 1008 g21 @7", 1008, 7, 1, 21),
]
HEADS = [("r18 512 @7", 512, 7, 1000), ("rgx0.6 528 @7", 528, 7, 1000)]
SHIFT = (31, 33, 32)       # the shift targets' k on the L = 32 grid
L = 32
ABITS = 8


def scaled_conv(torch, K, g, Ci, Co, R, G, wb, da, za):
    """A conv weight scaled per (co, ci) on the L = 32 grid: the wide blob (or the int8 one where it
    holds the weight), the decoded fp32 weight, s[co] and a bias."""
    Cig, whi = Ci // G, 2 ** wb - 1
    qw = torch.randint(0, whi + 1, (Co, Cig, R, R), generator=g).float().cuda()
    zw = torch.randint(0, whi + 1, (Co,), generator=g).float().cuda()
    d1 = (torch.rand(Co, generator=g) * 0.02 + 1e-3).cuda()
    k = torch.tensor(SHIFT, dtype=torch.int32)[torch.randint(0, 3, (Co, Cig), generator=g)]
    wscale = d1.view(-1, 1) * (k.float() / float(L)).cuda()
    what = (qw - zw.view(-1, 1, 1, 1)) * wscale.view(Co, Cig, 1, 1)
    packed, bad = K.pack_encode(what, zw, wscale.reshape(-1), True, None, wb, 0, whi)
    assert bad == 0
    prep = K.qweight_prepare_scaled(packed, (Co, Cig, R, R), zw, wb, 0, groups=G, kfac=k.reshape(-1),
                                    wide=True, wide_all=True)
    assert int(prep.bad.item()) == 0
    scale = ((torch.tensor([da], device="cuda") * d1) / torch.tensor([float(L)], device="cuda")).contiguous()
    return dict(prep=prep, what=what, scale=scale, bias=(torch.randn(Co, generator=g) * 0.1).cuda(),
                packed=packed, zw=zw, d1=d1, wb=wb, G=G, Co=Co, da=da,
                kw=dict(groups=G, act_zp=za, act_bits=ABITS, act_sym=False))


def grid_of(t, relu):
    """A min-max 8-bit act quantizer over t: (delta, zero point); zero point 0 behind a ReLU."""
    lo, hi = (0.0, float(t.max())) if relu else (float(t.min()), float(t.max()))
    d = max(hi - lo, 1e-6) / 255
    return d, float(min(max(round(-lo / d), 0), 255))


def run_grouped(i, args):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    name, C, H, stride, G = GROUPED[i]
    N = args.batch
    g = torch.Generator().manual_seed(6105 + i)
    torch.backends.cudnn.deterministic = True
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    da, za = 0.05, 0.0
    qa = torch.randint(0, 256, (N, C, H, H), generator=g).float().cuda()
    codes, _ = K.act_encode((qa - za) * da, da, za, ABITS, False, bad=counter)
    del qa
    lay = scaled_conv(torch, K, g, C, C, 3, G, 4, da, za)
    assert lay["prep"].wide and lay["prep"].wide_all
    # K26 as it stands: a plain W4 weight (per-co scale) of the same shape on the int8 blob
    pw = torch.randint(0, 16, (C, C // G, 3, 3), generator=g).float().cuda()
    pwhat = (pw - lay["zw"].view(-1, 1, 1, 1)) * lay["d1"].view(-1, 1, 1, 1)
    ppacked, bad = K.pack_encode(pwhat, lay["zw"], lay["d1"], False, None, 4, 0, 15)
    assert bad == 0
    narrow = K.qweight_prepare(ppacked, (C, C // G, 3, 3), lay["zw"], 4, 0, groups=G)
    nscale = (torch.tensor([da], device="cuda") * lay["d1"]).contiguous()
    kw = lay["kw"]
    y = K.qconv(codes, lay["prep"], lay["scale"], stride, 1, **kw)
    q = grid_of(torch.clamp(y + lay["bias"].view(1, -1, 1, 1), min=0.0), True)
    dt, zt = torch.tensor([q[0]], device="cuda"), torch.tensor([q[1]], device="cuda")
    del y

    def emit(prep, scale):
        return lambda: K.qconv_codes(codes, prep, scale, stride, 1, bias=lay["bias"], relu=1,
                                     out_delta=q[0], out_zp=q[1], out_bits=ABITS, bad=counter, **kw)

    def decoded():
        x = K.act_decode(codes, C, da, za, ABITS, False)
        yq = K.bias_act_quant(F.conv2d(x, lay["what"], stride=stride, padding=1, groups=G),
                              lay["bias"], None, 1, dt, zt, ABITS, False)
        return K.act_encode(yq, q[0], q[1], ABITS, False, bad=counter)[0]

    forms = {"wide codes": emit(lay["prep"], lay["scale"]), "int8 codes": emit(narrow, nscale),
             "decoded": decoded,
             "wide fp32": lambda: K.qconv(codes, lay["prep"], lay["scale"], stride, 1, **kw),
             "int8 fp32": lambda: K.qconv(codes, narrow, nscale, stride, 1, **kw)}
    with torch.no_grad():
        a, b = forms["wide codes"](), forms["decoded"]()
        differ = int((a != b).sum())
        steps = int((a.int() - b.int()).abs().max())
        assert int(counter.item()) == 0
        us = measure(torch, forms, args.rounds)
    print(json.dumps({"shape": name, "N": N, "codes_differing_from_decoded": differ,
                      "max_steps": steps, "codes": a.numel(), "us": us}), flush=True)


def run_chain(args):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    N, H, gw = args.batch, 28, 48
    g = torch.Generator().manual_seed(6205)
    torch.backends.cudnn.deterministic = True
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    # (Ci, Co, R, stride, pad, groups, activation) per conv; proj where the shape changes
    specs = [dict(ci=192, c=432, stride=2), dict(ci=432, c=432, stride=1)]

    def qt(q):
        return dict(q=q, dt=torch.tensor([q[0]], device="cuda"), zt=torch.tensor([q[1]], device="cuda"))

    def conv(lay, x, stride, pad):
        return K.qconv(x, lay["prep"], lay["scale"], stride, pad, act_delta=lay["da"], bad=counter,
                       **lay["kw"])

    def k13(y, bias, res, relu, t):
        return K.bias_act_quant(y, bias, res, relu, t["dt"], t["zt"], ABITS, False)

    inq = (0.05, 0.0)
    qa = torch.randint(0, 256, (N, 192, H, H), generator=g).float().cuda()
    x0 = ((qa - inq[1]) * inq[0]).contiguous()
    blocks, x = [], x0
    with torch.no_grad():
        for s in specs:                                # build and calibrate on the parent's route
            ci, c, st = s["ci"], s["c"], s["stride"]
            b = dict(stride=st, inq=inq, identity=ci == c and st == 1)
            b["c1"] = scaled_conv(torch, K, g, ci, c, 1, 1, 4, *inq)
            y = conv(b["c1"], x, 1, 0)
            b["q1"] = qt(grid_of(torch.clamp(y + b["c1"]["bias"].view(1, -1, 1, 1), min=0.0), True))
            h = k13(y, b["c1"]["bias"], None, 1, b["q1"])
            b["c2"] = scaled_conv(torch, K, g, c, c, 3, c // gw, 4, *b["q1"]["q"])
            y = F.conv2d(h, b["c2"]["what"], stride=st, padding=1, groups=c // gw)
            b["q2"] = qt(grid_of(torch.clamp(y + b["c2"]["bias"].view(1, -1, 1, 1), min=0.0), True))
            h = k13(y, b["c2"]["bias"], None, 1, b["q2"])
            b["c3"] = scaled_conv(torch, K, g, c, c, 1, 1, 4, *b["q2"]["q"])
            res = x
            if not b["identity"]:
                b["proj"] = scaled_conv(torch, K, g, ci, c, 1, 1, 4, *inq)
                res = K.bias_act(conv(b["proj"], x, st, 0), b["proj"]["bias"], None, 0)
            y = conv(b["c3"], h, 1, 0)
            t = torch.clamp(y + b["c3"]["bias"].view(1, -1, 1, 1) + res, min=0.0)
            b["q"] = qt(grid_of(t, True))
            x, inq = k13(y, b["c3"]["bias"], res, 1, b["q"]), b["q"]["q"]
            blocks.append(b)

    def parent(x):
        for b in blocks:
            st = b["stride"]
            h = k13(conv(b["c1"], x, 1, 0), b["c1"]["bias"], None, 1, b["q1"])
            h = k13(F.conv2d(h, b["c2"]["what"], stride=st, padding=1, groups=b["c2"]["G"]),
                    b["c2"]["bias"], None, 1, b["q2"])
            res = x if b["identity"] else K.bias_act(conv(b["proj"], x, st, 0), b["proj"]["bias"], None, 0)
            x = k13(conv(b["c3"], h, 1, 0), b["c3"]["bias"], res, 1, b["q"])
        return x

    def emit(lay, x, stride, pad, t, residual=None):
        c = K.qconv_codes(x, lay["prep"], lay["scale"], stride, pad, act_delta=lay["da"],
                          bias=lay["bias"], relu=1, out_delta=t["q"][0], out_zp=t["q"][1],
                          out_bits=ABITS, bad=counter, residual=residual, **lay["kw"])
        n, hh, ww, _ = c.shape
        return K.carried(c, (n, lay["Co"], hh, ww), t["q"][0], t["q"][1], ABITS, False)

    def wide_all(x):
        for b in blocks:
            st = b["stride"]
            h = emit(b["c1"], x, 1, 0, b["q1"])
            h = emit(b["c2"], h, st, 1, b["q2"])
            res = x if b["identity"] else K.bias_act(conv(b["proj"], x, st, 0), b["proj"]["bias"], None, 0)
            x = emit(b["c3"], h, 1, 0, b["q"], residual=res)
        return x

    c0, _ = K.act_encode(x0, 0.05, 0.0, ABITS, False, bad=counter)
    xc = K.carried(c0, tuple(x0.shape), 0.05, 0.0, ABITS, False)
    with torch.no_grad():
        ref = parent(x0)
        out = wide_all(xc)
        dec = K.act_decode(out, ref.shape[1], *blocks[-1]["q"]["q"], ABITS, False)
        steps = float(((dec - ref).abs() / blocks[-1]["q"]["q"][0]).max())
        differ = int((dec != ref).sum())
        assert int(counter.item()) == 0
        us = measure(torch, {"parent": lambda: parent(x0), "wide_all": lambda: wide_all(xc)}, args.rounds)
    print(json.dumps({"chain": "rgx3.2 s3.b1 -> s3.b2 (192 @28 -> 432 @14)", "N": N, "us": us,
                      "outputs_differing": differ, "outputs": ref.numel(),
                      "max_difference_in_steps": steps}), flush=True)


def run_heads(args):
    import numpy as np
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd import kernels as K

    N, rows = args.batch, []
    g = torch.Generator().manual_seed(6305)
    rng = np.random.default_rng(6305)
    for name, Cc, H, Co in HEADS:
        Cp, HW = (Cc + 15) // 16 * 16, H * H
        q = rng.integers(0, 256, (N, H, H, Cp)).astype(np.int64)
        q[..., Cc:] = 128
        codes = torch.from_numpy((q - 128).astype(np.int8)).cuda()
        d, z = 0.05, 3.0
        lay = scaled_conv(torch, K, g, Cc, Co, 1, 1, 8, d, z)
        prep = K.QPrepared(lay["prep"].blob, (Co, Cc), lay["prep"].bad, centred=True, wide=True)
        assert lay["prep"].wide
        what = lay["what"].reshape(Co, Cc)
        sh = K.head_scale(torch.tensor([d], device="cuda") * lay["d1"], L * HW)

        def head(tile):
            def f():
                return K.qlinear_pooled(*K.avgpool_codes(codes), prep, sh, HW, z, 8, False, wide_all=True)
            return f

        def decoded():
            return F.linear(K.act_decode(codes, Cc, d, z, 8, False).mean([2, 3]), what)

        with torch.no_grad():
            outs = {}
            for tile in (16, 64):
                K.qlinear_pooled_tile(tile)
                outs[tile] = head(tile)().clone()
            assert torch.equal(outs[16].view(torch.int32), outs[64].view(torch.int32)), name
            ref = decoded()
            drift = float((outs[16] - ref).abs().max())
            K.qlinear_pooled_tile(16)
            us = measure(torch, {"decoded head": decoded, "K29 + K30 wide, tile 16": head(16),
                                 "K29": lambda: K.avgpool_codes(codes)}, args.rounds)
            K.qlinear_pooled_tile(64)
            us.update(measure(torch, {"K29 + K30 wide, tile 64": head(64)}, args.rounds))
            K.qlinear_pooled_tile(16)
        rows.append({"shape": name, "N": N, "us": us, "max_abs_diff_vs_decoded": drift,
                     "max_abs_output": float(ref.abs().max())})
    print(json.dumps({"rows": rows}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=150, help="seconds per part")
    ap.add_argument("--part", default=None, help="(child) grouped:<i> | chain | heads")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.part is not None:
        if args.part.startswith("grouped:"):
            return run_grouped(int(args.part.split(":")[1]), args)
        return {"chain": run_chain, "heads": run_heads}[args.part](args)

    def child(part):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--batch", str(args.batch),
               "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"part {part} failed (rc={r.returncode}); stopping")
        sys.stderr.write(f"[{part}] done\n")
        sys.stderr.flush()
        return json.loads(r.stdout.strip().splitlines()[-1])

    grouped = [child(f"grouped:{i}") for i in range(len(GROUPED))]
    chain = child("chain")
    heads = child("heads")["rows"]
    sys.path.insert(0, ROOT)
    from shiftedscalequantization_amd.build import provenance

    def cell(t):
        return f"{t['median']:8.1f} ({t['min']:.1f}-{t['max']:.1f})".rjust(24)

    def spread(t):
        return t["max"] - t["min"]

    lines = [f"provenance {json.dumps(provenance())}",
             f"the wide operand on grouped convs and the pooled fc, batch {args.batch}; median us per call "
             f"over {args.rounds} rounds (min-max), forms alternated round by round",
             "", "(a) RegNetX-3200M grouped 3x3, W4 / L32 per-(co, ci), A8, codes in -> codes out",
             f"{'shape':<30}{'wide us':>24}{'int8 (K26) us':>24}{'decoded us':>24} {'wide/int8':>9} "
             f"{'dec/wide':>8} {'differ':>12}"]
    for r in grouped:
        u = r["us"]
        w, n, dcd = u["wide codes"], u["int8 codes"], u["decoded"]
        lines.append(f"{r['shape']:<30}{cell(w)}{cell(n)}{cell(dcd)} {w['median'] / n['median']:9.3f} "
                     f"{dcd['median'] / w['median']:8.3f} {r['codes_differing_from_decoded']:>5}/{r['codes']} (<= {r['max_steps']})")
    lines.append(f"{'fp32 output':<30}{'wide us':>24}{'int8 (K26) us':>24} {'wide/int8':>9}")
    for r in grouped:
        w, n = r["us"]["wide fp32"], r["us"]["int8 fp32"]
        lines.append(f"{r['shape']:<30}{cell(w)}{cell(n)} {w['median'] / n['median']:9.3f}")
    lines.append("int8: K26 on a plain int8 blob of the same shape; decoded: act_decode + library grouped "
                 "conv + K13 with the act quantizer + K21; differ: codes of wide that differ from decoded's (and by how "
                 "many steps at most): the library conv's summation order")
    u = chain["us"]
    verdict = ("slower" if u["wide_all"]["median"] > u["parent"]["median"] + spread(u["parent"]) else
               "faster" if u["wide_all"]["median"] < u["parent"]["median"] - spread(u["parent"]) else
               "inside the parent's spread")
    lines += ["", f"(b) {chain['chain']}, every weight W4 / L32 per-(co, ci), A8",
              f"{'route':<30}{'us':>24}",
              f"{'parent (grouped decoded)':<30}{cell(u['parent'])}",
              f"{'wide_all (codes carried)':<30}{cell(u['wide_all'])}",
              f"parent / wide_all = {u['parent']['median'] / u['wide_all']['median']:.3f}: wide_all is "
              f"{verdict}; outputs differing {chain['outputs_differing']}/{chain['outputs']}, at most "
              f"{chain['max_difference_in_steps']:.2f} quantizer steps (the library conv's summation order)"]
    lines += ["", "(c) the head on a W8 / L32 per-(co, ci) fc (|m| up to 8415), A8, 1000 classes",
              f"{'shape':<18}{'decoded head us':>24}{'K29 us':>24}{'K29+K30 wide t16 us':>24}"
              f"{'K29+K30 wide t64 us':>24} {'dec/t16':>8}"]
    for r in heads:
        u = r["us"]
        lines.append(f"{r['shape']:<18}{cell(u['decoded head'])}{cell(u['K29'])}"
                     f"{cell(u['K29 + K30 wide, tile 16'])}{cell(u['K29 + K30 wide, tile 64'])} "
                     f"{u['decoded head']['median'] / u['K29 + K30 wide, tile 16']['median']:8.3f}")
        lines.append(f"{'':<18}max |wide - decoded| = {r['max_abs_diff_vs_decoded']:.3g} of max |logit| = "
                     f"{r['max_abs_output']:.3g}")
    lines.append("decoded head: act_decode + fp32 mean + fp32 linear on the decoded weight; the two tiles' "
                 "outputs are identical bit for bit")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
