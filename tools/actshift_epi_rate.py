"""K34 (the shifted-scale act quantizer inside the K13 epilogue pass) against the two-pass
sequences of the same build -- forward ssq_epilogue_fwd then ssq_actshift_fwd, backward
ssq_actshift_bwd_delta then ssq_epilogue_bwd -- and K.stream_copy, at the shapes of a ResNet
block loop, with and without a residual; bias and gamma^z / phi^z present, ReLU, soft form with
ddelta.  Measured as tools/actshift_delta_rate.py measures: HIP-event time per launch sequence
on the launch stream (bench.time_events: back-to-back launches, median of 5 groups), buffers
allocated once, the C ABI called directly, forms alternated over the rounds and every round's
time printed (the spread).  `ratio` is the two-pass median over the fused one.

    python tools/actshift_epi_rate.py [--reps 300] [--S 2] [--rounds 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from shiftedscalequantization_amd import _capi as A  # noqa: E402
from shiftedscalequantization_amd import kernels as K  # noqa: E402

SHAPES = [(32, 64, 56, 56), (32, 512, 7, 7)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--S", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    S = a.S
    sh = A.shifts_arg([1.0, 0.5, 0.75, 0.25][:S])
    print(f"# K34 against K13 + K33, S = {S}, A4 (qmax 15), ReLU, soft with ddelta, {a.reps} "
          f"back-to-back launches per group, median of 5 groups, forms alternated over {a.rounds} "
          f"rounds; us = median round")
    for shape in SHAPES:
        N, C, H, W = shape
        hw, n = H * W, N * C * H * W
        g = torch.Generator(device="cuda").manual_seed(7)
        rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
        conv, res_t, gy = rnd(shape) * 1.2, rnd(shape) * 0.3, rnd(shape)
        bias, gamma, phi = rnd(C) * 0.1, 1.0 + rnd(C) * 0.1, rnd(C) * 0.1
        x, y, dx, dconv, dres = (torch.empty_like(conv) for _ in range(5))
        p = torch.softmax(rnd(C, S), -1).contiguous()
        dp, dd = torch.empty(C, S, device=dev), torch.empty((), device=dev)
        delta, zp = torch.tensor(0.2, device=dev), torch.tensor(0.0, device=dev)
        nbytes = max(A.query("ssq_epilogue_actshift_bwd_workspace_size", N, C, hw, S),
                     A.query("ssq_epilogue_bwd_workspace_size", N * C), 8)
        ws, ws2 = (torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2))
        st, P = A.stream_of(conv), A.ptr
        for res in (None, res_t):
            gres = None if res is None else dres

            def fused_fwd():
                A.call("ssq_epilogue_actshift_fwd", P(conv), P(bias), P(gamma), P(phi), P(res), 1,
                       P(p), P(delta), P(zp), sh, S, N, C, hw, 15, 0, P(y), st)

            def two_fwd():
                A.call("ssq_epilogue_fwd", P(conv), P(bias), P(gamma), P(phi), P(res), P(x), None,
                       n, hw, C, 1, None, None, 0, 1, st)
                A.call("ssq_actshift_fwd", P(x), P(p), P(delta), P(zp), sh, S, N, C, hw, 15, 0,
                       P(y), None, 0, st)

            def fused_bwd():
                A.call("ssq_epilogue_actshift_bwd", P(conv), P(gy), P(bias), P(gamma), P(phi),
                       P(res), 1, P(p), P(delta), P(zp), sh, S, N, C, hw, 15, 0, P(dconv), P(gres),
                       P(dp), P(dd), P(ws), ws.numel(), st)

            def two_bwd():
                A.call("ssq_actshift_bwd_delta", P(x), P(gy), P(p), P(delta), P(zp), sh, S, N, C,
                       hw, 15, 0, P(dx), P(dp), P(dd), P(ws), ws.numel(), st)
                A.call("ssq_epilogue_bwd", P(dx), P(conv), P(bias), P(gamma), P(phi), P(res), N, C,
                       hw, 1, None, None, 0, 1, P(dconv), P(gres), None, None, None, None, P(ws2),
                       ws2.numel(), st)

            two_fwd()      # x for two_bwd
            forms = [("stream_copy", lambda: K.stream_copy(conv, y)), ("fwd_two_pass", two_fwd),
                     ("fwd_fused", fused_fwd), ("bwd_two_pass", two_bwd), ("bwd_fused", fused_bwd)]
            times = {name: [] for name, _ in forms}
            for _ in range(a.rounds):
                for name, fn in forms:
                    times[name].append(bench.time_events(fn, a.reps, dev) * 1e3)
            med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
            for name, _ in forms:
                rec = {"shape": "x".join(map(str, shape)), "residual": res is not None,
                       "form": name, "us": round(med[name], 2),
                       "us_rounds": [round(t, 2) for t in times[name]]}
                if name.endswith("_fused"):
                    rec["ratio"] = round(med[name.replace("fused", "two_pass")] / med[name], 2)
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
