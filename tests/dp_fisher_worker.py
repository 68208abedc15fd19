"""One rank of the world-size-2 Fisher reconstruction test (tests/test_fisher_gpu.py), in
tests/dp_worker.py's pattern: two ranks share the one GPU over gloo, each takes its half of
the fixture's calibration data, builds its own Fisher cache (save_grad_data) and runs
block_reconstruction with opt_mode='fisher_diag' for 6 iterations.  Written out: V before and
after, every iteration's (local, all-reduced) gradient bucket, and what the loop used.

    python tests/dp_fisher_worker.py OUT.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ITERS, BS = 6, 4


def host(t):
    return t.detach().float().cpu().numpy().copy()


def main():
    path = sys.argv[1]
    torch.cuda.set_device(0)
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    dist.init_process_group("gloo")
    from conftest import load_golden
    import test_recon_gpu as T
    from shiftedscalequantization_amd import _capi, parallel_dp as P, quant as Q
    from shiftedscalequantization_amd.quant._engine import GRAPH_REPLAYS
    P.RECORD = []
    out = {"rank": np.array([dist.get_rank()])}
    g = load_golden("recon_brecq_fisher_diag")
    qnn = T.build_qnn(Q, g)
    block = qnn.model[3]
    lo, hi = P.shard_rows(len(g["cali"]))
    cali = T.dev(g["cali"][lo:hi])
    convs = ("conv1", "conv2", "downsample")
    calls = {"fisher": 0, "adam": 0}

    def hook(name, args):
        calls["fisher"] += name.startswith("ssq_fisher_diag_loss")

    orig_adam = torch.optim.Adam.__init__

    def adam_init(self, *a, **k):
        calls["adam"] += 1
        return orig_adam(self, *a, **k)

    _capi.CALL_HOOK, torch.optim.Adam.__init__ = hook, adam_init
    import importlib
    BR = importlib.import_module("shiftedscalequantization_amd.quant.block_recon")
    orig_fast = BR._fast_loop

    def fast(*a):
        # V at the loop's start (the AdaRound quantizers exist only from here on)
        for n in convs:
            out[n + "_V0"] = host(getattr(block, n).weight_quantizer.alpha)
        return orig_fast(*a)

    BR._fast_loop = fast
    torch.manual_seed(1005)
    Q.block_reconstruction(qnn, block, cali, batch_size=BS, iters=ITERS, weight=0.01, asym=True,
                           b_range=(20, 2), warmup=0.2, act_quant=False, opt_mode="fisher_diag")
    torch.cuda.synchronize()
    for n in convs:
        out[n + "_V"] = host(getattr(block, n).weight_quantizer.alpha)
    for k, (kind, local, reduced) in enumerate(P.RECORD):
        out[f"rec{k}_local"] = local.cpu().numpy()
        out[f"rec{k}_reduced"] = reduced.cpu().numpy()
    out["n_rec"] = np.array([len(P.RECORD)])
    out["split_replays"] = np.array([GRAPH_REPLAYS["split"]])
    out["fisher_calls"] = np.array([calls["fisher"]])
    out["adam"] = np.array([calls["adam"]])
    np.savez(path, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
