"""K33's backward with the delta gradient (ssq_actshift_bwd_delta) against the backward without
it (ssq_actshift_bwd of the same build) and K.stream_copy, at the shapes of a ResNet block
loop, measured as tools/actshift_rate.py measures: HIP-event time per launch sequence on the
launch stream (bench.time_events: back-to-back launches, median of 5 groups), buffers allocated
once, the C ABI called directly.  Forms are alternated over the rounds and every round's time is
printed (the spread); `extra_us` is the delta form's median over the plain backward's, next to
`second_pass_us`, the time of reading x and g once more (8 B/elem at the copy's rate): what a
separate ddelta pass after ssq_actshift_bwd would cost at the least.

    python tools/actshift_delta_rate.py [--reps 300] [--S 2] [--rounds 5]
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
    sh = A.shifts_arg([1.0, 0.5, 0.75, 0.25][:a.S])
    print(f"# K33 backward with ddelta, S = {a.S}, A4 (qmax 15), {a.reps} back-to-back launches per "
          f"group, median of 5 groups, forms alternated over {a.rounds} rounds; us = median round")
    for shape in SHAPES:
        N, C, H, W = shape
        hw, n = H * W, N * C * H * W
        g = torch.Generator(device="cuda").manual_seed(7)
        x = torch.relu(torch.randn(shape, device=dev, generator=g)) * 1.2
        gy = torch.randn(shape, device=dev, generator=g)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        p = torch.softmax(torch.randn(C, a.S, device=dev, generator=g), -1).contiguous()
        dp, dd = torch.empty(C, a.S, device=dev), torch.empty((), device=dev)
        delta, zp = torch.tensor(0.2, device=dev), torch.tensor(0.0, device=dev)
        ws = torch.empty(max(A.query("ssq_actshift_bwd_delta_workspace_size", N, C, hw, a.S), 8),
                         dtype=torch.uint8, device=dev)
        st, P = A.stream_of(x), A.ptr

        def bwd(hard):
            return lambda: A.call("ssq_actshift_bwd", P(x), P(gy), P(p), P(delta), P(zp), sh, a.S, N,
                                  C, hw, 15, hard, P(dx), P(dp), P(ws), ws.numel(), st)

        def bwd_delta(hard):
            return lambda: A.call("ssq_actshift_bwd_delta", P(x), P(gy), P(p), P(delta), P(zp), sh,
                                  a.S, N, C, hw, 15, hard, P(dx), P(dp), P(dd), P(ws), ws.numel(), st)

        forms = [("stream_copy", lambda: K.stream_copy(x, y)),
                 ("bwd_soft", bwd(0)), ("bwd_delta_soft", bwd_delta(0)),
                 ("bwd_hard", bwd(1)), ("bwd_delta_hard", bwd_delta(1))]
        times = {name: [] for name, _ in forms}
        for _ in range(a.rounds):
            for name, fn in forms:
                times[name].append(bench.time_events(fn, a.reps, dev) * 1e3)
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        second_pass = med["stream_copy"]          # 8 B/elem, as the copy moves
        for name, _ in forms:
            rec = {"shape": "x".join(map(str, shape)), "form": name, "us": round(med[name], 2),
                   "us_rounds": [round(t, 2) for t in times[name]],
                   "gbs_12B": round(12 * n / med[name] / 1e3, 1)}
            if name == "stream_copy":
                rec["gbs_12B"] = None
                rec["gbs_8B"] = round(8 * n / med[name] / 1e3, 1)
            if name.startswith("bwd_delta"):
                rec["extra_us"] = round(med[name] - med[name.replace("_delta", "")], 2)
                rec["second_pass_us"] = round(second_pass, 2)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
