"""Iteration rate of BRECQ's weight phase under the Fisher-weighted losses, beside the MSE
loop (tools/brecq_bench.py's blocks and method: batch 32, synthetic data, rate =
200 / (T(220 iterations) - T(20)), so caching, the Fisher cache and setup cancel out).

    python tools/fisher_rate.py [--rounds 3] [--forms mse,fast,eager] [--modes fisher_diag,fisher_full]
                                [--root DIR] [--tag NAME]

Forms, alternated within each round in one process:
    mse    opt_mode='mse' (the fused tail, K11t)
    mse_notail  the same with block_recon.FUSE_TAIL off: the block materialises its output and
           K11 is a pass of its own, as the Fisher loops' K20 is
    fast   the device loop with the K20 loss pass (block_recon.FISHER_FAST on)
    eager  the reference's eager loop (SSQ_FISHER_FAST=0: torch autograd + torch.optim.Adam)
--root DIR imports the package from another tree (e.g. a checkout of an earlier commit, whose
Fisher modes have only the eager loop: --forms eager); --tag names the tree in the output.
One JSON line per (round, block, form, mode), then a summary line of medians.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

BLOCKS = (("resnet18", "layer1.0"), ("resnet50", "layer1.0"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--forms", default="mse,fast,eager")
    ap.add_argument("--modes", default="fisher_diag,fisher_full")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="tree")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.root))
    from shiftedscalequantization_amd import nets
    from shiftedscalequantization_amd.quant import QuantModel, block_reconstruction
    BR = importlib.import_module("shiftedscalequantization_amd.quant.block_recon")

    dev = torch.device("cuda")
    cali = torch.randn(128, 3, 224, 224, device=dev)

    def rate(arch, path, opt_mode):
        times = {}
        for iters in (20, 220):
            torch.manual_seed(1005)
            qnn = QuantModel(nets.ARCHS[arch]().eval(),
                             {"n_bits": 2, "channel_wise": True, "scale_method": "max"},
                             {"n_bits": 4, "channel_wise": False, "scale_method": "mse",
                              "leaf_param": True})
            qnn.to(dev).eval()
            qnn.set_first_last_layer_to_8bit()
            qnn.set_quant_state(True, False)
            with torch.no_grad():
                qnn(cali[:64])
            blk = qnn.model
            for part in path.split("."):
                blk = blk[int(part)] if part.isdigit() else getattr(blk, part)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            block_reconstruction(qnn, blk, cali, batch_size=32, iters=iters, weight=0.01, asym=True,
                                 b_range=(20, 2), warmup=0.2, act_quant=False, opt_mode=opt_mode)
            torch.cuda.synchronize()
            times[iters] = time.perf_counter() - t0
        return 200 / (times[220] - times[20])

    forms = args.forms.split(",")
    runs = [(f, "mse") for f in forms if f.startswith("mse")]
    runs += [(f, m) for m in args.modes.split(",") for f in forms if not f.startswith("mse")]
    fuse_tail = BR.FUSE_TAIL
    seen = {}
    for rnd in range(args.rounds + 1):              # round 0: warm-up (MIOpen's solver search)
        for arch, path in BLOCKS:
            for form, mode in runs:
                BR.FISHER_FAST = form != "eager"
                BR.FUSE_TAIL = fuse_tail and form != "mse_notail"
                r = rate(arch, path, mode)
                if rnd:
                    key = f"{arch}.{path}/{form}/{mode}"
                    seen.setdefault(key, []).append(r)
                    print(json.dumps({"tree": args.tag, "round": rnd, "block": f"{arch}.{path}",
                                      "form": form, "opt_mode": mode, "iters_per_s": round(r, 1)}),
                          flush=True)
    print(json.dumps({"tree": args.tag, "summary_iters_per_s": {
        k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
            "max": round(max(v), 1)} for k, v in seen.items()}}), flush=True)


if __name__ == "__main__":
    main()
