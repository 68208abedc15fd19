"""The fc AdaRound loop under data parallel at world size 2 (block_recon.FC_SPLIT): K19 split
around the bucket's all-reduce -- ssq_fc_recon_grad writing V's gradient into its bucket
slice, the collective, ssq_fc_recon_apply -- as two graphs around the collective after the
eager warm-up (quant._engine.IterationGraph).

Two ranks share the box's one GPU over gloo, as tests/test_dp_gpu.py: the bucket / collective
logic is backend-independent.  Each rank reconstructs on its half of the calibration inputs
(tests/dp_fc_worker.py)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ITERS = 12


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_world2(mode, tmp_path, tag="", **extra_env):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    port = _free_port()
    procs, outs = [], []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **extra_env)
        out = str(tmp_path / f"{mode}{tag}_r{r}.npz")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dp_fc_worker.py"), mode, out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=100)[0].decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    return [dict(np.load(o)) for o in outs]


def _calls(r):
    return {k: int(r["calls_fc_recon_" + k][0]) for k in ("iter", "grad", "apply")}


def test_fc_world2_fused_replicated(tmp_path):
    """Default knobs (FC_SPLIT auto: a bucket exists, so the split pair), batch 8, 12
    iterations: the loop runs on fc_recon_grad / fc_recon_apply and never fc_recon_iter, the
    iterations after the warm-up replay the two graphs around the collective; every reduced
    bucket is the same on both ranks and the sum of the two locals, which differ; V is
    replicated and equal to a one-process Adam (lr 1e-3) replay fed the reduced buckets from
    the recorded start; the hard W^ is replicated."""
    from shiftedscalequantization_amd.quant._engine import SsqAdam
    r0, r1 = _run_world2("fc", tmp_path)
    for r in (r0, r1):
        c = _calls(r)
        assert c["grad"] >= 2 and c["apply"] == c["grad"] and c["iter"] == 0, c
        assert int(r["split_replays"][0]) > 0
    n = int(r0["n_rec"][0])
    assert n == int(r1["n_rec"][0]) == ITERS
    reduced = []
    for k in range(n):
        red0, red1 = r0[f"rec{k}_reduced"], r1[f"rec{k}_reduced"]
        assert red0.size == 40 * 512
        np.testing.assert_array_equal(red0.view(np.int32), red1.view(np.int32), err_msg=f"bucket {k}")
        np.testing.assert_array_equal(red0.view(np.int32),
                                      (r0[f"rec{k}_local"] + r1[f"rec{k}_local"]).view(np.int32),
                                      err_msg=f"bucket {k} is not the sum of the locals")
        assert not np.array_equal(r0[f"rec{k}_local"], r1[f"rec{k}_local"])      # different shards
        reduced.append(red0)
    np.testing.assert_array_equal(r0["V0"], r1["V0"])
    np.testing.assert_array_equal(r0["V"].view(np.int32), r1["V"].view(np.int32))
    assert not np.array_equal(r0["V"], r0["V0"])
    p = torch.nn.Parameter(torch.as_tensor(r0["V0"]).cuda())
    opt = SsqAdam([p], lr=1e-3)
    for flat in reduced:
        p.grad = torch.as_tensor(flat).view_as(p).cuda()
        opt.step()
    np.testing.assert_array_equal(p.detach().cpu().numpy().view(np.int32), r0["V"].view(np.int32))
    np.testing.assert_array_equal(r0["what_hard"].view(np.int32), r1["what_hard"].view(np.int32))
    assert not np.array_equal(r0["losses"], r1["losses"])        # each rank's own shard


def test_fc_world2_fused_vs_unfused(tmp_path):
    """The same world-2 loop at 4-bit weights with the split pair (default) and with
    SSQ_FC_SPLIT=0 (the unfused iteration: hipBLASLt's GEMMs, another fp32 summation order --
    no bit check).  The first iteration starts from the same state in both runs: its loss
    within rtol 1e-5 (test_fc_fused_iteration_matches_unfused's 4-bit bound) and its reduced
    bucket within 1e-4 x max|bucket| (the bound test_fc_recon_iter_vs_reference holds V's
    gradient to against float64).  Later iterations: V inside Adam's walk budget,
    iterations x 2e-3, as the world-1 comparison."""
    split = _run_world2("fc4", tmp_path)
    unfused = _run_world2("fc4", tmp_path, tag="_unfused", SSQ_FC_SPLIT="0")
    for r in split:
        c = _calls(r)
        assert c["grad"] >= 2 and c["iter"] == 0, c
    for r in unfused:
        assert _calls(r) == {"iter": 0, "grad": 0, "apply": 0}, _calls(r)
    stats = {}
    for k, (a, b) in enumerate(zip(split, unfused)):
        assert int(a["n_rec"][0]) == int(b["n_rec"][0]) == ITERS
        np.testing.assert_array_equal(a["V0"], b["V0"])
        la, lb = a["losses"], b["losses"]
        assert len(la) == len(lb) == ITERS
        red_a, red_b = a["rec0_reduced"], b["rec0_reduced"]
        scale = float(np.abs(red_b).max())
        stats[f"r{k}_loss0_rel"] = abs(la[0] - lb[0]) / abs(lb[0])
        stats[f"r{k}_loss_rel_max"] = float(np.max(np.abs(la - lb) / np.abs(lb)))
        stats[f"r{k}_bucket0_err"] = float(np.abs(red_a - red_b).max())
        stats[f"r{k}_bucket0_max"] = scale
        stats[f"r{k}_V_dev"] = float(np.abs(a["V"] - b["V"]).max())
    print("PARITY", json.dumps({"test": "fc_world2_split_vs_unfused[w4]", **stats}))
    for k in range(2):
        assert stats[f"r{k}_loss0_rel"] <= 1e-5, stats
        assert stats[f"r{k}_bucket0_err"] <= 1e-4 * stats[f"r{k}_bucket0_max"], stats
        assert stats[f"r{k}_V_dev"] <= ITERS * 2e-3, stats
