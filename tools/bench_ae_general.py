#!/usr/bin/env python3
"""Timing of the per-layer autoencoder route (csrc/ae_general.hip, reached through AutoEncoderTask._step on chains cvf_ae_step
refuses): training steps (gradient + fused Adam) of one chain on resident feature rows, meant to run under
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_ae_general.py --e-dims 384,256,64,2 --d-dims 2,64,256,384 --batch 16000
The kernel statistics file then gives the time per kernel (aeg_*, slab_reduce_kernel).  Beside it, on the same device and in the
same process, the reference's own step written with torch in fp32: oracle.nnref.autoencoder_forward + ae_loss + backward +
torch.optim.Adam.  Prints one JSON line: wall time per step of both, measured with device events around `--steps` steps after
`--warmup`, alternating the two in `--rounds` rounds, and the step's matrix FLOP count."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd")):
    sys.path.insert(0, p)


def step_flops(dims, B):
    """Matrix FLOPs of one training step: forward and weight gradient of every layer, the adjoint product of all but the first."""
    prods = [dims[l] * dims[l + 1] for l in range(len(dims) - 1)]
    return 2 * (2 * sum(prods) + sum(prods[1:])) * B


def timed(fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--e-dims", default="66,128,128,2")
    ap.add_argument("--d-dims", default="2,128,128,66")
    ap.add_argument("--batch", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from colvarsfinder import core, nn
    from oracle import losses
    from tests.synth import Traj
    e_dims, d_dims = ([int(v) for v in s.split(",")] for s in (a.e_dims, a.d_dims))
    dims = e_dims + d_dims[1:]
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(3)
    X = rs.normal(size=(a.batch, dims[0])).astype(np.float32)
    w = rs.uniform(0.5, 1.5, size=a.batch)
    torch.manual_seed(0)
    model = nn.AutoEncoder(e_dims, d_dims)
    sd = {n: p.detach().clone().to(dev).requires_grad_(True) for n, p in model.state_dict().items()}
    task = core.AutoEncoderTask(Traj(X[:64], w[:64], 1.0), torch.nn.Identity(), model, "/tmp/cvf_bench_ae_general", learning_rate=1e-3,
                                device=dev, verbose=False, save_model_every_step=0)
    assert task._general[True], "cvf_ae_step takes this chain: the per-layer route is not reached"
    Xd, wd = torch.tensor(X, device=dev), torch.tensor(w, dtype=torch.float32, device=dev)
    inv_wsum = 1.0 / float(wd.sum(dtype=torch.float64))
    opt = torch.optim.Adam(list(sd.values()), lr=1e-3)

    def hip_step():
        task._step(Xd, None, wd, True, inv_wsum, advance=True, fuse_adam=True)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        losses.ae_loss(sd, Xd, wd).backward()
        opt.step()

    for fn in (hip_step, torch_step):
        timed(fn, a.warmup)
    hip_ms, torch_ms = [], []
    for _ in range(a.rounds):
        hip_ms.append(timed(hip_step, a.steps))
        torch_ms.append(timed(torch_step, a.steps))
    f = step_flops(dims, a.batch)
    print(json.dumps(dict(dims=dims, batch=a.batch, n_params=task._flat.n, hip_ms_per_step=min(hip_ms), hip_ms_rounds=hip_ms,
                          torch_ms_per_step=min(torch_ms), torch_ms_rounds=torch_ms, step_gflop=f / 1e9,
                          hip_tflops=f / min(hip_ms) / 1e9, loss=float(task._out2[2]))))


if __name__ == "__main__":
    main()
