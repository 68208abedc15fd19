"""Iteration rate of the fc's AdaRound weight phase (main_imagenet.py:114-118:
layer_reconstruction on ResNet-18's last QuantModule, batch 32, synthetic data): the
end-to-end flow's 20000-iteration loop on a tiny layer, where the host's per-iteration work
can outlast the GPU's.  Rate = 2000 / (T(2200) - T(200)); then a cProfile of one
2200-iteration run (top host functions by own time).  Usage: python tools/fc_recon_rate.py

--split-ab [--rounds R] [--out FILE]: the iteration's three forms at world 1, us per iteration
of back-to-back chunk-graph replays (block_recon.CHUNK_PROBE; GPU work and launch boundaries,
no host work or collective), alternated R times in one process: the unfused launches
(FUSE_FC off: the world > 1 body without the split), the split pair (FC_SPLIT on:
ssq_fc_recon_grad + ssq_fc_recon_apply) and K19 (ssq_fc_recon_iter)."""
import cProfile
import io
import json
import os
import pstats
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shiftedscalequantization_amd import nets  # noqa: E402
from shiftedscalequantization_amd.quant import QuantModel, QuantModule, layer_reconstruction  # noqa: E402


def build(dev):
    torch.manual_seed(1005)
    qnn = QuantModel(nets.ARCHS["resnet18"]().eval(), {"n_bits": 2, "channel_wise": True, "scale_method": "max"},
                     {"n_bits": 4, "channel_wise": False, "scale_method": "mse", "leaf_param": True})
    qnn.to(dev).eval()
    qnn.set_first_last_layer_to_8bit()
    return qnn


def run(dev, cali, iters):
    qnn = build(dev)
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:64])
    fc = [m for m in qnn.modules() if isinstance(m, QuantModule)][-1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    layer_reconstruction(qnn, fc, cali, batch_size=32, iters=iters, weight=0.01, asym=True,
                         b_range=(20, 2), warmup=0.2, act_quant=False, opt_mode="mse")
    torch.cuda.synchronize()
    return time.perf_counter() - t0


FORMS = (("unfused", False, "off"), ("split", True, "on"), ("k19", True, "off"))


def split_ab(rounds, out_path):
    from shiftedscalequantization_amd.build import provenance
    from shiftedscalequantization_amd.quant import block_recon as BR
    dev = torch.device("cuda")
    cali = torch.randn(256, 3, 224, 224, device=dev)
    probe = BR.ChunkGraph.probe
    BR.ChunkGraph.probe = lambda self: probe(self, reps=200)      # 5000 iterations a window
    prev = (BR.FUSE_FC, BR.FC_SPLIT)
    lines = []
    try:
        for r in range(rounds + 1):                               # round 0 warms every form up
            for name, fuse, split in FORMS:
                BR.FUSE_FC, BR.FC_SPLIT = fuse, split
                BR.CHUNK_PROBE[0] = False
                run(dev, cali, 300)
                us, BR.CHUNK_PROBE[0] = BR.CHUNK_PROBE[0], None
                if r:
                    lines.append(json.dumps({"round": r, "form": name,
                                             "chunk_replay_us_per_iter": round(us, 2)}))
                    print(lines[-1], flush=True)
    finally:
        BR.ChunkGraph.probe = probe
        BR.FUSE_FC, BR.FC_SPLIT = prev
    med = {}
    for name, _, _ in FORMS:
        v = sorted(json.loads(ln)["chunk_replay_us_per_iter"] for ln in lines
                   if json.loads(ln)["form"] == name)
        med[name] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
    lines.append(json.dumps({"summary_us_per_iter": med, "iters_per_chunk": BR.CHUNK_ITERS,
                             "shape": "512 -> 1000, batch 32, 8-bit", **provenance()}))
    print(lines[-1])
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    if "--split-ab" in sys.argv:
        arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d  # noqa: E731
        return split_ab(int(arg("--rounds", 3)), arg("--out", None))
    dev = torch.device("cuda")
    cali = torch.randn(256, 3, 224, 224, device=dev)
    run(dev, cali, 20)
    t = {n: run(dev, cali, n) for n in (200, 2200)}
    us = (t[2200] - t[200]) / 2000 * 1e6
    out = {"fc_adaround_us_per_iter": round(us, 2), "it_per_s": round(1e6 / us, 1)}
    print(json.dumps(out))
    # the chunk graph's own replay time (GPU work + launch boundaries, no host work between
    # iterations): 20 back-to-back replays of the loop's last chunk graph, HIP events
    from shiftedscalequantization_amd.quant import block_recon as BR
    BR.CHUNK_PROBE[0] = False
    run(dev, cali, 300)
    us_chunk = BR.CHUNK_PROBE[0]
    BR.CHUNK_PROBE[0] = None
    if us_chunk:
        print(json.dumps({"chunk_replay_us_per_iter": round(us_chunk, 2),
                          "iters_per_chunk": BR.CHUNK_ITERS}))
    pr = cProfile.Profile()
    pr.enable()
    run(dev, cali, 2200)
    pr.disable()
    s = io.StringIO()
    pstats.Stats(pr, stream=s).sort_stats("tottime").print_stats(25)
    print(s.getvalue())


if __name__ == "__main__":
    main()
