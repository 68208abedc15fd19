"""K33 (ssq_actshift_fwd / ssq_actshift_bwd) rate at the shapes of a ResNet block loop:
HIP-event time per launch on the launch stream (bench.time_events: back-to-back launches,
median of 5 groups), the algorithm's bytes over that time (8 B/elem forward, 12 B/elem
backward) and the fraction of the same run's K.stream_copy rate (8 B/elem) on a tensor of
the same size.  Buffers are allocated once and the C ABI is called directly, so the host
cost per launch is one ctypes call for every form, the copy included.

    python tools/actshift_rate.py [--reps 300] [--S 2]
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
    a = ap.parse_args()
    dev = torch.device("cuda")
    shifts = [1.0, 0.5, 0.75, 0.25][:a.S]
    sh = A.shifts_arg(shifts)
    print(f"# K33 rate, S = {a.S}, A4 (qmax 15), {a.reps} back-to-back launches per group, median of "
          f"5 groups, forms alternated over 3 rounds; GB/s = algorithm bytes / event time")
    for shape in SHAPES:
        N, C, H, W = shape
        hw, n = H * W, N * C * H * W
        g = torch.Generator(device="cuda").manual_seed(7)
        x = torch.relu(torch.randn(shape, device=dev, generator=g)) * 1.2
        gy = torch.randn(shape, device=dev, generator=g)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        p = torch.softmax(torch.randn(C, a.S, device=dev, generator=g), -1).contiguous()
        dp = torch.empty(C, a.S, device=dev)
        delta = torch.tensor(0.2, device=dev)
        zp = torch.tensor(0.0, device=dev)
        wsb = A.query("ssq_actshift_bwd_workspace_size", N, C, hw, a.S)
        ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
        st = A.stream_of(x)
        P = A.ptr

        def fwd(hard):
            return lambda: A.call("ssq_actshift_fwd", P(x), P(p), P(delta), P(zp), sh, a.S, N, C, hw,
                                  15, hard, P(y), None, 0, st)

        def bwd(hard):
            return lambda: A.call("ssq_actshift_bwd", P(x), P(gy), P(p), P(delta), P(zp), sh, a.S, N,
                                  C, hw, 15, hard, P(dx), P(dp), P(ws), ws.numel(), st)

        forms = [("stream_copy", 8, lambda: K.stream_copy(x, y)),
                 ("fwd_soft", 8, fwd(0)), ("fwd_hard", 8, fwd(1)),
                 ("bwd_soft", 12, bwd(0)), ("bwd_hard", 12, bwd(1))]
        best = {}
        for rnd in range(3):
            for name, bpe, fn in forms:
                ms = bench.time_events(fn, a.reps, dev)
                best.setdefault(name, []).append(ms)
        copy_gbs = None
        for name, bpe, _ in forms:
            ms = sorted(best[name])[1]
            gbs = bpe * n / (ms * 1e-3) / 1e9
            if name == "stream_copy":
                copy_gbs = gbs
            print(json.dumps({"shape": "x".join(map(str, shape)), "form": name, "bytes_per_elem": bpe,
                              "us": round(ms * 1e3, 2), "gbs": round(gbs, 1),
                              "of_stream_copy": round(gbs / copy_gbs, 3),
                              "us_rounds": [round(t * 1e3, 2) for t in best[name]]}), flush=True)


if __name__ == "__main__":
    main()
