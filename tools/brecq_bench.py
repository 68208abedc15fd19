"""BRECQ block_reconstruction iteration rate (ResNet-50 block_recon):
AdaRound weight phase and act-delta (LSQ) phase on one block, batch 32, synthetic data.
Rate = (T(iters_long) - T(iters_short)) / (iters_long - iters_short), so caching and setup
cancel out.

    --opt_mode fisher_diag | fisher_full   the Fisher-weighted loss (its cache's setup cancels
                                           out the same way); SSQ_FISHER_FAST=0 in the
                                           environment times the eager loop instead
    --phases weight[,act]  --blocks resnet18.layer1.0[,...]   a subset of the default runs"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shiftedscalequantization_amd import nets  # noqa: E402
from shiftedscalequantization_amd.quant import QuantModel, block_reconstruction  # noqa: E402


def build(arch, dev):
    torch.manual_seed(1005)
    qnn = QuantModel(nets.ARCHS[arch]().eval(), {"n_bits": 2, "channel_wise": True, "scale_method": "max"},
                     {"n_bits": 4, "channel_wise": False, "scale_method": "mse", "leaf_param": True})
    qnn.to(dev).eval()
    qnn.set_first_last_layer_to_8bit()
    return qnn


def block_of(qnn, path):
    m = qnn.model
    for part in path.split("."):
        m = m[int(part)] if part.isdigit() else getattr(m, part)
    return m


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt_mode", default="mse", choices=["mse", "fisher_diag", "fisher_full"])
    ap.add_argument("--phases", default="weight,act")
    ap.add_argument("--blocks", default="resnet18.layer1.0,resnet50.layer1.0")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    cali = torch.randn(128, 3, 224, 224, device=dev)
    res = {}
    for arch, path in (b.split(".", 1) for b in args.blocks.split(",")):
        for phase in args.phases.split(","):
            times = {}
            for iters in (20, 20, 220):      # the first run pays one-time setup (MIOpen)
                qnn = build(arch, dev)
                qnn.set_quant_state(True, phase == "act")
                with torch.no_grad():
                    qnn(cali[:64])
                blk = block_of(qnn, path)
                kw = dict(batch_size=32, iters=iters, weight=0.01, asym=True, b_range=(20, 2),
                          warmup=0.2, act_quant=phase == "act", opt_mode=args.opt_mode)
                if phase == "act":
                    kw.update(lr=4e-4, p=2.4)
                times[iters] = timed(lambda: block_reconstruction(qnn, blk, cali, **kw))
            rate = 200 / (times[220] - times[20])
            res[f"{arch}.{path}.{phase}"] = round(rate, 1)
            print(json.dumps({"block": f"{arch}.{path}", "phase": phase, "opt_mode": args.opt_mode,
                              "iters_per_s": round(rate, 1)}), flush=True)
    print(json.dumps({"brecq_iters_per_s": res, "opt_mode": args.opt_mode}))


if __name__ == "__main__":
    main()
