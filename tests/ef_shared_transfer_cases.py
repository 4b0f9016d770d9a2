"""Case table, inputs and fp64 oracle of the transfer-mode shared-trunk step (csrc/ef_general.hip: cvf_ef_general_shared_transfer_*,
DESIGN.md section 4.12), shared by tests/test_ef_shared_transfer_host.py (CPU) and tests/test_ef_shared_transfer_gpu.py.

Reference: oracle.losses.ef_loss in fp64 with ``X_lag, w_lag, lag_idx, dt`` and the shared layers passed as the SAME leaf tensors
for every net, so autograd sums their gradient (the rule of tests/test_ef_general_shared_gpu.py::_oracle).  Bars, one per quantity:
8 x the worst distance of the same oracle evaluated in fp32 on the CPU from its fp64 evaluation, over all cases and both batch
sizes - the loss vector and the eigenvalues relative, the gradient relative to its largest entry.

Frames: an AR(1) sequence with one correlation per input feature (0.2 .. 0.95), so that the nets' time-lagged eigenvalues differ
by far more than the bar (checked on the CPU: test_ef_shared_transfer_host.py::test_eigenvalues_are_separated).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.ef_general_cases import HALF_B

ACTS = {"tanh": (1, torch.tanh), "relu": (3, torch.relu), "softplus": (6, F.softplus)}   # (code of include/cvf.h, oracle function)
# id, dims, k, n_shared, activation
CASES = [("d2-k3", [7, 65, 33, 1], 3, 1, "tanh"),              # width 65 crosses a 64-row block, the head has a hidden layer
         ("top-k2", [9, 130, 1], 2, 1, "tanh"),                # n_shared = NH: the summed top step
         ("top-d2-k3", [7, 65, 33, 1], 3, 2, "tanh"),          # the same below a two-layer trunk
         ("d3-k8", [5, 5, 70, 6, 1], 8, 2, "tanh"),
         ("softplus", [7, 65, 33, 1], 3, 1, "softplus"),       # sigma(0) != 0
         ("relu", [9, 130, 1], 2, 1, "relu")]
BATCHES = [70, HALF_B]    # two ragged tiles (four with the lagged ones); 258 step tiles on 256 slab rows
ALPHA, LAG, DT = 12.0, 2, 0.5
# seed of a case's parameters and frames (+ B % 89): chosen so that the fp64 eigenvalues of both batches are well apart - among 60
# seeds the eight eigenvalues of d3-k8 are at least 1.9 % of the largest apart only at this one
SEEDS = {c[0]: 4000 + 11 * i for i, c in enumerate(CASES)}
SEEDS["d3-k8"] = 4023


def eig_w(k):
    return [1.0 - 0.1 * i for i in range(k)]


def case_of(cid):
    return next(c for c in CASES if c[0] == cid)


@functools.lru_cache(maxsize=None)
def inputs(cid, B):
    """Parameters (net 0's first n_shared layers stand for every net's), frames [B + LAG, d0] and weights of a case: CPU, fp32."""
    from oracle import nnref
    case = case_of(cid)
    _, dims, k, ns, act = case
    g = torch.Generator().manual_seed(SEEDS[cid] + B % 89)
    sd = nnref.init_eigenfunctions(dims, k, g)
    rho = torch.linspace(0.2, 0.95, dims[0])
    noise = torch.randn(B + LAG, dims[0], generator=g, dtype=torch.float64)
    X = torch.empty(B + LAG, dims[0], dtype=torch.float64)
    X[0] = noise[0]
    for t in range(1, B + LAG):
        X[t] = rho * X[t - 1] + torch.sqrt(1 - rho * rho) * noise[t]
    w = torch.rand(B + LAG, generator=g) + 0.5
    return sd, X.float(), w


def flat(sd, dims, k, ns):
    """Flat vector in the layout of core._SharedTrunkFlat: the shared layers once (net 0's), then net by net the rest."""
    L = len(dims) - 1
    out = [sd[f"eigen_funcs.0.{l + 1}.{n}"].reshape(-1) for l in range(ns) for n in ("weight", "bias")]
    for i in range(k):
        out += [sd[f"eigen_funcs.{i}.{l + 1}.{n}"].reshape(-1) for l in range(ns, L) for n in ("weight", "bias")]
    return torch.cat(out)


def tied(sd, k, ns):
    """``sd`` with net 0's first ns layers standing in every net (the same tensor objects)."""
    sd = dict(sd)
    for i in range(1, k):
        for l in range(ns):
            for n in ("weight", "bias"):
                sd[f"eigen_funcs.{i}.{l + 1}.{n}"] = sd[f"eigen_funcs.0.{l + 1}.{n}"]
    return sd


def oracle(cid, B, dtype):
    """(loss vector [loss, npl, pen], eigenvalues, cvec, flat gradient) of oracle.losses.ef_loss in ``dtype``."""
    from oracle import losses
    _, dims, k, ns, act = case_of(cid)
    sd0, X, w = inputs(cid, B)
    torch.set_default_dtype(dtype)
    try:
        sd = tied({n: p.to(dtype).requires_grad_(True) for n, p in sd0.items()}, k, ns)
        Xd, wd = X.to(dtype), w.to(dtype)
        lo, eo, no, po, co = losses.ef_loss(sd, k, lambda x: x, Xd[:B], wd[:B], Xd[LAG:LAG + B], wd[LAG:LAG + B], alpha=ALPHA,
                                            eig_w=eig_w(k), lag_idx=LAG, dt=DT, activation=ACTS[act][1])
        lo.backward()
        grad = flat({n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in sd.items()}, dims, k, ns)
    finally:
        torch.set_default_dtype(torch.float32)
    return (np.asarray([float(lo.detach()), float(no.detach()), float(po.detach())]), eo.double().numpy(), [int(c) for c in co], grad.double().numpy())


def errors(got, want):
    """(loss vector, eigenvalues, gradient / its largest entry) distances of a result from the fp64 one."""
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)))   # noqa: E731
    return rel(got[0], want[0]), rel(got[1], want[1]), float(np.abs(got[3] - want[3]).max() / np.abs(want[3]).max())


@functools.lru_cache(maxsize=None)
def reference():
    """({(case id, B): fp64 oracle}, bars) - computed once per process, never modified."""
    ref, worst = {}, [0.0, 0.0, 0.0]
    for case in CASES:
        for B in BATCHES:
            ref[case[0], B] = want = oracle(case[0], B, torch.float64)
            worst = [max(a, b) for a, b in zip(worst, errors(oracle(case[0], B, torch.float32), want))]
    bars = dict(zip(("loss", "eig", "grad"), (8.0 * e for e in worst)))
    print(f"[shared-tr] bars (8 x fp32 CPU oracle vs fp64): loss {bars['loss']:.2e} eig {bars['eig']:.2e} grad {bars['grad']:.2e}")
    return ref, bars


def sum_copies(grad, dims, k, ns):
    """Gradient of the copies layout folded into the shared layout: the nets' copies of the shared layers summed."""
    L = len(dims) - 1
    size = [dims[l + 1] * (dims[l] + 1) for l in range(L)]
    per, n_sh = sum(size), sum(size[:ns])
    g = grad.reshape(k, per)
    return np.concatenate([g[:, :n_sh].sum(0)] + [g[i, n_sh:] for i in range(k)])
