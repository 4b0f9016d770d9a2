"""GPU (-m gpu): q = J A J^T g and E = g^T J A J^T g per frame and net on every instance of the metric kernels, through the C ABI,
against the fp64 oracle - the table of tests/metric_cases.py (its docstring: reference, error measure, bars).

Each case calls ``cvf_align_feature_fwd`` with aux and scratch, ``cvf_metric_dense_tensors`` and ``cvf_metric_apply``; it first asserts
the instance ``cvf_metric_route`` names - the function the launch decides by.  Every output starts as NaN: a valid lane left unwritten
fails.  A repeated call must give the same bits, and so must a call whose padded lanes of ``g_tiled``, ``aux`` and ``slot_xyz`` hold
garbage instead of zeros.  ``cvf_metric_apply_stats``: q and E are those of ``cvf_metric_apply`` bit for bit, and ``stats`` is held to
exact summation (``math.fsum``) of the fp64 terms built from the kernel's own E, within (B + 3) 2^-53 sum |t|.
The instances behind the process-wide switches run in one child process per switch (tests/metric_switch_child.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import metric_cases as M
from tests.stats_tail_cases import tiled

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_q_and_e_per_frame_vs_fp64(dev, case):
    M.run_and_check(case, dev)


@pytest.mark.parametrize("cid,B,k", M.STATS_CASES, ids=[f"{cid}-B{B}" for cid, B, _ in M.STATS_CASES])
def test_apply_stats_vs_exact_sums(dev, cid, B, k):
    case = M.BY_ID[cid]
    p = M.abi_prepare(case, dev, B)
    plan = M.abi_route(p.desc, B, k, True, case.npb)
    assert plan == M.expected_plan(case, True, B=B, k=k), (cid, B, plan)
    g = M.cotangent(case, p.layer.d_r, B, k).numpy()
    rs = np.random.RandomState(B + k)
    w = rs.uniform(0.5, 1.5, B).astype(np.float32)
    y = rs.standard_normal((B, k)).astype(np.float32)
    w_dev = torch.tensor(w, device=dev)
    gt, aux, slot = M.padded(p, g, None)
    q0, E0 = M.abi_apply(p, gt, k, aux, slot, case.npb)
    q1, E1, st = M.abi_apply(p, gt, k, aux, slot, case.npb, stats=(w_dev, torch.tensor(tiled(y, B), device=dev)))
    assert np.isfinite(q1).all() and np.isfinite(E1).all() and np.isfinite(st).all()
    assert M.same_bits(q0, q1) and M.same_bits(E0, E1), "the fused call computes another q or E"
    want, abs_sums = M.exact_sums(M.stats_terms(w, y, E1))
    bound = (B + 3) * 2.0 ** -53 * abs_sums
    worst = float((np.abs(st - want) / bound).max())
    print(f"[metric stats] {cid} B {B}: family {plan['family']} F {plan['F']} fused {plan['fused']} rows {plan['fused_rows']}: "
          f"max |stats - exact| / bound = {worst:.3f}", flush=True)
    assert (np.abs(st - want) <= bound).all(), worst
    if B % M.TILE:
        # Garbage in the padded lanes of g and y: the padded frames carry weight 0.  (aux and slot_xyz stay as the forward call left
        # them: both stages multiply a padded lane's E by the weight 0, so E must be finite there - it is for the copies of the last
        # frame the forward call leaves, and for any finite g; garbage geometry can make it NaN, and 0 x NaN is NaN.)
        gt, aux, slot = M.padded(p, g, "garbage", seed=B, g_only=True)
        q2, E2, st2 = M.abi_apply(p, gt, k, aux, slot, case.npb, stats=(w_dev, torch.tensor(tiled(y, B, garbage=B), device=dev)))
        assert M.same_bits(q1, q2) and M.same_bits(E1, E2) and M.same_bits(st, st2), "the padded lanes reach the sums"


def test_switch_instances_in_a_child_process(dev):
    """CVF_METRIC_WAVES and CVF_METRIC_PRE are read once per process: one fresh child per switch, each under a time limit of its
    own; the first non-zero status ends the test."""
    env = {n: v for n, v in os.environ.items() if n not in ("CVF_METRIC_NPB", "CVF_METRIC_WAVES", "CVF_METRIC_PRE")}
    for which, switch in (("waves16", {"CVF_METRIC_WAVES": "16"}), ("pre5", {"CVF_METRIC_PRE": "5"})):
        r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-m", "tests.metric_switch_child", which], cwd=ROOT,
                           env={**env, **switch}, capture_output=True, text=True)
        print(r.stdout, flush=True)
        assert r.returncode == 0, (which, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
