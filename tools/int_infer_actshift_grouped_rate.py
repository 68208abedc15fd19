"""Rate of the per-channel-grid emitters of K25 / K26 against their scalar twins of the same build
("Shifted activations on codes"): ssq_qconv_i8_grouped_codes_chq_fwd against
ssq_qconv_i8_grouped_codes_fwd at MobileNetV2's depthwise shapes (3x3 at 112, 56, 28, 14 and 7) and
RegNetX-600MF's grouped f.b shapes (group width 24), batch 64.  The method of
tools/int_infer_actshift_rate.py: HIP-event time per launch (bench.time_events: back-to-back
launches, median of 5 groups), the two forms alternated over 3 rounds; the printed figure is the
median round, with all three and the scalar twin's min-max spread.  Both forms go through the same
Python wrapper (K.qconv_codes).  Inputs are random codes: the rate does not depend on their values.
The scalar kernels are the parent commit's, count for count in the compiler's resource report
(DESIGN 4), so no second library is built here; `--only scalar` times them alone, for a run against
another checkout.

    python tools/int_infer_actshift_grouped_rate.py [--reps 200] [--batch 64] [--only scalar]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from shiftedscalequantization_amd import kernels as K  # noqa: E402

# (name, C, plane, stride, groups): MobileNetV2's depthwise convs by plane (the widest of each
# plane), then RegNetX-600MF's f.b (3x3, group width 24) per stage
SHAPES = [("mbv2_dw", 96, 112, 2, 96), ("mbv2_dw", 144, 56, 1, 144), ("mbv2_dw", 192, 28, 1, 192),
          ("mbv2_dw", 576, 14, 1, 576), ("mbv2_dw", 960, 7, 1, 960),
          ("rgx_fb", 48, 56, 1, 2), ("rgx_fb", 96, 28, 1, 4), ("rgx_fb", 240, 14, 1, 10),
          ("rgx_fb", 528, 7, 1, 22)]
AB, ZA = 4, 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", choices=["scalar"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    print(f"# K25 / K26 _chq emitters against their scalar twins, batch {a.batch}, A{AB}, W2 plain "
          f"weights, {a.reps} back-to-back launches per group, median of 5 groups, 3 alternated rounds")
    for name, C, P, st, G in SHAPES:
        N, Cig = a.batch, C // G
        w = torch.randint(0, 4, (C, Cig, 3, 3), device=dev, generator=g).float()
        zw = torch.full((C,), 2.0, device=dev)
        d1 = torch.full((C,), 0.01, device=dev)
        packed, bad = K.pack_encode((w - 2.0) * 0.01, zw, d1, False, None, 2, 0, 3)
        assert bad == 0
        prep = K.qweight_prepare(packed, (C, Cig, 3, 3), zw, 2, 0, groups=G)
        scale = torch.full((C,), 1e-3, device=dev)
        Cp = -(-C // 16) * 16
        codes = torch.randint(-128, -112, (N, P, P, Cp), device=dev, generator=g, dtype=torch.int8)
        vec = torch.randn(C, device=dev, generator=g) * 0.01
        cs = K.ChannelScale(0.05 * torch.tensor([1.0, 0.5], device=dev)[torch.arange(C, device=dev) % 2])
        word = torch.zeros(1, dtype=torch.int32, device=dev)

        def conv(delta):
            return lambda: K.qconv_codes(codes, prep, scale, st, 1, groups=G, act_zp=ZA, act_bits=AB,
                                         bias=vec, relu=2, out_delta=delta, out_zp=ZA, out_bits=AB,
                                         bad=word)

        forms = {"scalar": conv(0.05)} if a.only else {"scalar": conv(0.05), "chq": conv(cs)}
        t = {k: [] for k in forms}
        for _ in range(3):
            for k, fn in forms.items():
                t[k].append(bench.time_events(fn, a.reps, dev))
        us = {k: [round(v * 1e3, 2) for v in t[k]] for k in t}
        row = {"shape": f"{name} {N}x{C}x{P}x{P} s{st} g{G}", "kind": K.qconv_kind(prep),
               "scalar_us": sorted(us["scalar"])[1],
               "scalar_spread_us": round(max(us["scalar"]) - min(us["scalar"]), 2), "rounds_us": us}
        if "chq" in us:
            row["chq_us"] = sorted(us["chq"])[1]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
