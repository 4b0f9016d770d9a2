#!/usr/bin/env python3
"""Timing of the general eigenfunction route (EigenFunctionTask(general_nets=True), csrc/ef_general.hip): a few generator-mode
steps (loss_func + backward) of one shape on Identity features, meant to run under
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_ef_general.py --dims 384,256,256,256,1 --k 6 --batch 16000
The kernel statistics file then gives the time per kernel; this script prints the step's matrix FLOP count (the model of DESIGN.md
section 4.8) and the wall time per step measured with HIP events, as one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd")):
    sys.path.insert(0, p)


def step_flops(dims, k, B, gen=True):
    """Matrix FLOPs of one step: forward (every layer), g sweep (every layer), tangent (hidden layers), adjoint sweep (hidden
    layers but the first), weight gradients (every layer, two parts in generator mode)."""
    prods = [dims[l] * dims[l + 1] for l in range(len(dims) - 1)]
    hidden = prods[:-1]
    n = sum(prods)                         # forward
    if gen:
        n += sum(prods[:-1]) + sum(hidden)  # g sweep (the top layer's product is a broadcast), tangent
        n += sum(prods[1:-1])               # adjoint sweep
        n += 2 * sum(prods)                 # weight gradients: [zbar | d] x [h | tdot]
    else:
        n += sum(prods[1:-1]) + sum(prods)
    return 2 * n * k * B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="384,256,256,256,1")
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--batch", type=int, default=16000)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    from colvarsfinder import core, nn
    from tests.synth import Traj
    dims = [int(v) for v in a.dims.split(",")]
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(3)
    X = rs.normal(size=(a.batch, dims[0])).astype(np.float32)
    w = rs.uniform(0.5, 1.5, size=a.batch)
    torch.manual_seed(0)
    model = nn.EigenFunctions(dims, a.k)
    task = core.EigenFunctionTask(Traj(X[:64], w[:64], 1.0), torch.nn.Identity(), model, "/tmp/cvf_bench_general", 10.0,
                                  [1.0] * a.k, k=a.k, device=dev, verbose=False, save_model_every_step=0, general_nets=True)
    Xd, wd = torch.tensor(X, device=dev), torch.tensor(w, dtype=torch.float32, device=dev)
    for _ in range(2):
        task.loss_func(Xd, wd, None, None)
        task.backward()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.steps):
        task.loss_func(Xd, wd, None, None)
        task.backward()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.steps
    f = step_flops(dims, a.k, a.batch)
    print(json.dumps(dict(dims=dims, k=a.k, batch=a.batch, ms_per_step=ms, step_gflop=f / 1e9, tflops=f / ms / 1e9,
                          n_params=task._flat.n, slab_rows=task._workspace(a.batch).slab_rows)))


if __name__ == "__main__":
    main()
