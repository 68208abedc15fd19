"""Rate of the per-channel-grid emitters against their scalar twins ("Shifted activations
on codes"): K23's code-emitting conv (ssq_qconv_i8_codes_chq_fwd against ssq_qconv_i8_*codes*_fwd,
without a residual and with a code residual) and K27 (ssq_epilogue_codes_chq_fwd against
ssq_epilogue_codes_fwd) at ResNet-18's body shapes at batch 64.  HIP-event time per launch
(bench.time_events: back-to-back launches, median of 5 groups), the forms alternated over 3 rounds;
the printed figure is the median round, with all three and the scalar twin's min-max spread.  Both
forms go through the same Python wrapper (K.qconv_codes / K.epilogue_codes), so the host cost per
launch is the same.  Inputs are random codes: the rate does not depend on their values.

    python tools/int_infer_actshift_rate.py [--reps 200] [--batch 64]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from shiftedscalequantization_amd import kernels as K  # noqa: E402

# (C, plane): the 3x3 stride-1 convs of ResNet-18's four stages
SHAPES = [(64, 56), (128, 28), (256, 14), (512, 7)]
AB, ZA = 4, 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    print(f"# _chq emitters against their scalar twins, batch {a.batch}, A{AB}, W2 plain weights, "
          f"{a.reps} back-to-back launches per group, median of 5 groups, 3 alternated rounds")
    for C, P in SHAPES:
        N = a.batch
        w = torch.randint(0, 4, (C, C, 3, 3), device=dev, generator=g).float()
        zw = torch.full((C,), 2.0, device=dev)
        d1 = torch.full((C,), 0.01, device=dev)
        packed, bad = K.pack_encode((w - 2.0) * 0.01, zw, d1, False, None, 2, 0, 3)
        assert bad == 0
        prep = K.qweight_prepare(packed, (C, C, 3, 3), zw, 2, 0)
        scale = torch.full((C,), 1e-3, device=dev)
        codes = torch.randint(-128, -112, (N, P, P, C), device=dev, generator=g, dtype=torch.int8)
        res = torch.randint(-128, -112, (N, P, P, C), device=dev, generator=g, dtype=torch.int8)
        y = torch.randn(N, C, P, P, device=dev, generator=g)
        vec = torch.randn(C, device=dev, generator=g) * 0.01
        dch = 0.05 * torch.tensor([1.0, 0.5], device=dev)[torch.arange(C, device=dev) % 2]
        cs = K.ChannelScale(dch)
        word = torch.zeros(1, dtype=torch.int32, device=dev)

        def conv(delta, rdelta):
            r = None if rdelta is None else K.carried(res, (N, C, P, P), rdelta, ZA, AB, False)
            return lambda: K.qconv_codes(codes, prep, scale, 1, 1, act_zp=ZA, act_bits=AB, bias=vec,
                                         relu=1, out_delta=delta, out_zp=ZA, out_bits=AB, bad=word,
                                         residual=r)

        def k27(delta):
            return lambda: K.epilogue_codes(y, vec, None, None, 1, delta, ZA, AB, False, word)

        pairs = [("k23_codes", conv(0.05, None), conv(cs, None)),
                 ("k23_codes_res_codes", conv(0.05, 0.05), conv(cs, cs)),
                 ("k27", k27(0.05), k27(cs))]
        for name, scalar, chq in pairs:
            t = {"scalar": [], "chq": []}
            for _ in range(3):
                t["scalar"].append(bench.time_events(scalar, a.reps, dev))
                t["chq"].append(bench.time_events(chq, a.reps, dev))
            us = {k: [round(v * 1e3, 2) for v in t[k]] for k in t}
            print(json.dumps({"shape": f"{N}x{C}x{P}x{P}", "form": name,
                              "scalar_us": sorted(us["scalar"])[1], "chq_us": sorted(us["chq"])[1],
                              "scalar_spread_us": round(max(us["scalar"]) - min(us["scalar"]), 2),
                              "rounds_us": us}), flush=True)


if __name__ == "__main__":
    main()
