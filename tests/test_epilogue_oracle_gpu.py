"""The K13 epilogue family on the device against the fp64 oracle (oracle/ssq_ref.py
epilogue_fwd / epilogue_bwd / epilogue_loss_bwd), at the edges of its forms: the cases of
tests/epilogue_cases.py through the public wrappers (tests/epilogue_worker.py check_case).

  * Forward output, pre-quant activation where the pass keeps it, gy and gres: bit-identical
    to the oracle, which states the same individually rounded fp32 operations (so the masks
    are the same bits too).  A NaN that propagates from a NaN input is compared bit for bit
    as well; a NaN an invalid operation makes (inf - inf) only by position.  At p = 2 the
    tail's gradients are bit-exact and the loss is within rtol 1e-6 (row partials).
  * ggamma, gphi, gdelta, gzp and the residual epilogue's gamma / phi sums: inside the derived
    bound |got - S| <= ulp32(S) + (n - 1) * 2^-53 * A (epilogue_cases.sum_bound), at every p.
  * The fused tail at p = 2.4 goes through the hardware log2 / exp2, so its loss gradient is
    only within K11's tolerance (rtol 1e-5, atol 1e-9) of the oracle's, and so are gy, gres
    and the loss: asserted.  To keep the sums' bound and the bit identity there too, K11's
    own kernel (the same lp_elem) gives the loss gradient of the oracle's output, that
    gradient is checked against the oracle's at K11's tolerance, and the oracle's backward is
    restated from it: against that reference gy and gres are bit-identical and every sum is
    inside the same derived bound, with no looser term.
  * Every call repeated once: bit-identical (the delta ticket resets); on the 1025-row and
    16500-row cases the deferred finalize gives the standalone bits.
  * The compiled A/B forms (SSQ_EPI_G16=0 with SSQ_EPI_MULTI_ROW unset / 2 / 0,
    SSQ_K13_PLANE4=0) are read once per process: one fresh child process each, one after
    another, running the worker's reduced case list with the same assertions.

Each case reports its form and, per sum, error / bound through $SSQ_PARITY_LOG
(profiles/epilogue_parity.jsonl)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import epilogue_cases as EC
import epilogue_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


def parity_report(rec):
    """Print the reached parity and append it to $SSQ_PARITY_LOG (jsonl) when set."""
    print(json.dumps(rec))
    path = os.environ.get("SSQ_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


@pytest.mark.parametrize("c", EC.BWD, ids=EC.case_id)
def test_epilogue_forward_and_backward_match_the_oracle(K, c):
    parity_report(W.check_case(K, c))


@pytest.mark.parametrize("c", EC.TAIL, ids=EC.case_id)
def test_fused_tail_matches_the_oracle(K, c):
    parity_report(W.check_case(K, c))


@pytest.mark.parametrize("c", EC.FWD, ids=EC.case_id)
def test_forward_forms_match_the_oracle(K, c):
    parity_report(W.check_case(K, c))


def test_special_values_bit_for_bit(K):
    """-0.0, NaN, +-inf, 6.0 and its neighbours, denormals through ReLU6 and the 4-bit
    quantizer: forward, gy, gres bit for bit with a NaN wherever the oracle has one, each sum
    NaN exactly where the oracle's is."""
    parity_report(W.check_case(K, EC.SPECIAL))


def test_non_default_forms_in_fresh_processes(K):
    """SSQ_EPI_G16=0 (the 4-rows register form), with SSQ_EPI_MULTI_ROW=2 and =0, and
    SSQ_K13_PLANE4=0: one child per environment, none started after a failed one."""
    clean = {k: v for k, v in os.environ.items()
             if k not in ("SSQ_EPI_G16", "SSQ_EPI_MULTI_ROW", "SSQ_K13_PLANE4")}
    for name, (env, _) in EC.WORKER_ENVS.items():
        r = subprocess.run([sys.executable, os.path.join(HERE, "epilogue_worker.py"), name],
                           env=dict(clean, **env), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
        assert f"worker OK {name}" in r.stdout, (name, r.stdout[-2000:])
        for line in r.stdout.splitlines():
            if line.startswith("PARITY "):
                parity_report(json.loads(line[len("PARITY "):]))
