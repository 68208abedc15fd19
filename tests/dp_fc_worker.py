"""One rank of the world-size-2 fc reconstruction tests (tests/test_dp_fc_gpu.py).

Started twice by the test (RANK 0 / 1) on the one GPU of the box over gloo, as
tests/dp_worker.py.  Each rank runs BRECQ's layer loop on the last layer (512 -> 40) of the
recon_layer_brecq_fc fixture's network over its contiguous half of the calibration inputs
(parallel_dp.shard_rows), and writes what the test compares: which fc kernels the loop
called, the split-graph replays, V before and after, every iteration's loss and (local,
all-reduced) gradient bucket (parallel_dp.RECORD), and the hard W^ after the loop.

    python tests/dp_fc_worker.py {fc|fc4} OUT.npz

fc: the fixture's 8-bit scales.  fc4: 4-bit weights, scales initialised from the whole
calibration set (the same on both ranks).  The routing knobs come from the environment
(SSQ_FC_SPLIT), as in production.
"""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ITERS, BS = 12, 8


def host(t):
    return t.detach().float().cpu().numpy().copy()


def build(mode, g):
    import test_recon_gpu as T
    from shiftedscalequantization_amd import quant as Q
    if mode == "fc":
        qnn = T.build_qnn(Q, g, net=T.fc_mlp())
    else:
        qnn = Q.QuantModel(T.fc_mlp(), {"n_bits": 4, "channel_wise": True, "scale_method": "max"},
                           {"n_bits": 8, "channel_wise": False, "scale_method": "max"}).cuda().eval()
        qms = [m for m in qnn.modules() if isinstance(m, Q.QuantModule)]
        for k, m in enumerate(qms):
            w, b = T.dev(g[f"qm{k}_w"]), T.dev(g[f"qm{k}_b"])
            m.org_weight, m.org_bias = w.clone(), b.clone()
            m.weight.data, m.bias.data = w.clone(), b.clone()
        qnn.set_quant_state(True, False)
        with torch.no_grad():
            qnn(T.dev(g["cali"]))
    fc = [m for m in qnn.modules() if isinstance(m, Q.QuantModule)][-1]
    assert tuple(fc.weight.shape) == (40, 512)
    return Q, qnn, fc


def run(mode, out):
    from conftest import load_golden
    from shiftedscalequantization_amd.parallel_dp import shard_rows
    BR = importlib.import_module("shiftedscalequantization_amd.quant.block_recon")
    E = importlib.import_module("shiftedscalequantization_amd.quant._engine")
    g = load_golden("recon_layer_brecq_fc")
    Q, qnn, fc = build(mode, g)
    lo, hi = shard_rows(len(g["cali"]))
    cali = torch.as_tensor(g["cali"][lo:hi]).cuda()
    calls = {"fc_recon_iter": 0, "fc_recon_grad": 0, "fc_recon_apply": 0}
    losses = []

    def counted(name):
        fn = getattr(BR.K, name)

        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        setattr(BR.K, name, f)

    for name in calls:
        counted(name)
    adam_init, record = E.SsqAdam.__init__, BR.LossFunction.record

    def init(self, params, *a, **k):
        adam_init(self, params, *a, **k)
        out["V0"] = host(self.params[0])

    def spy(self, rec, rnd, b, count=None):
        losses.append(float(rec))
        return record(self, rec, rnd, b, count=count)

    E.SsqAdam.__init__, BR.LossFunction.record = init, spy
    torch.manual_seed(1005)
    Q.layer_reconstruction(qnn, fc, cali, batch_size=BS, iters=ITERS, weight=0.01, asym=True,
                           b_range=(20, 2), warmup=0.2, act_quant=False, opt_mode="mse")
    q = fc.weight_quantizer
    out["V"] = host(q.alpha)
    out["losses"] = np.array(losses, np.float64)
    for name, n in calls.items():
        out["calls_" + name] = np.array([n])
    assert not q.soft_targets
    with torch.no_grad():
        out["what_hard"] = host(q(fc.weight))


def main():
    mode, path = sys.argv[1], sys.argv[2]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    from shiftedscalequantization_amd import parallel_dp as P
    P.RECORD = []
    out = {"rank": np.array([dist.get_rank()])}
    run(mode, out)
    torch.cuda.synchronize()
    for k, (kind, local, reduced) in enumerate(P.RECORD):
        out[f"rec{k}_local"] = local.cpu().numpy()
        out[f"rec{k}_reduced"] = reduced.cpu().numpy()
    out["n_rec"] = np.array([len(P.RECORD)])
    from shiftedscalequantization_amd.quant._engine import GRAPH_REPLAYS
    out["split_replays"] = np.array([GRAPH_REPLAYS["split"]])
    np.savez(path, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
