"""EigenFunctionTask (generator mode) with a foreign preprocessing module: the dipeptide-sized shape with all pairwise distances
of 10 atoms (d_r = 45, tot_dim = 30, rho = 30), k = 2, nets [45, 20, 20, 20, 1], 150 000 frames, batches of 20 000.

Prints one JSON line: record build time at construction, step time through train()'s graph path, the factored-metric kernel's
time by HIP events (its record bytes per second), and the same batch through oracle.losses.ef_loss + autograd on the GPU.
For the kernel's time from the profiler, run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_foreign_pp.py`
(a run of its own).  Usage: python tools/bench_foreign_pp.py [--frames N] [--batch B] [--epochs E]"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd")):
    sys.path.insert(0, p)

from tests.foreign_modules import PairDistances  # noqa: E402
from tests.synth import Traj, diag_coeff_for, make_molecule_traj  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150000)
    ap.add_argument("--batch", type=int, default=20000)
    ap.add_argument("--epochs", type=int, default=3)
    args = ap.parse_args()
    from colvarsfinder import _hip, core, nn
    dev = torch.device("cuda")
    traj, w, _ = make_molecule_traj(10, args.frames, seed=1)
    a = torch.tensor(diag_coeff_for(10, 1), dtype=torch.float32)
    module = PairDistances(10)
    torch.manual_seed(0)
    model = nn.EigenFunctions([45, 20, 20, 20, 1], 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), module, model, "/tmp/cvf_bench_foreign", 20.0, [1.0, 0.8], diag_coeff=a,
                                  k=2, batch_size=args.batch, num_epochs=args.epochs, device=dev, verbose=False,
                                  save_model_every_step=0, test_ratio=0.2)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    n_train = int(args.frames * 0.8) // args.batch
    n_test = int(args.frames * 0.2) // args.batch
    task.train()   # epoch 1: eager warm-up + graph capture; later epochs replay
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    task.num_epochs = args.epochs
    task.train()   # (train() re-captures: time the replays of a second call's later epochs)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    # replay-only timing: one more epoch through the captured graphs
    g = task._graphs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        for key in sorted(g):
            g[key].replay()
    torch.cuda.synchronize()
    step_us = (time.perf_counter() - t0) / (reps * (n_train + n_test)) * 1e6
    # the kernel alone, HIP events
    B = args.batch
    ws = task._workspace(B)
    X = task._traj[:B]
    lib, P = _hip.lib(), _hip.ptr
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(3):
        lib.cvf_metric_apply(task._pp, P(X), B, None, None, 2, P(ws.g), P(ws.q), P(ws.e), None, None, _hip.stream())
    ev[0].record()
    n_k = 50
    for i in range(n_k):   # (rotate through the resident records: every launch reads from HBM, not the Infinity Cache)
        s = (i * B) % (task._traj.shape[0] - B + 1)
        lib.cvf_metric_apply(task._pp, P(task._traj[s:s + B]), B, None, None, 2, P(ws.g), P(ws.q), P(ws.e), None, None, _hip.stream())
    ev[1].record()
    torch.cuda.synchronize()
    k_us = ev[0].elapsed_time(ev[1]) / n_k * 1e3
    rec_bytes = B * 45 * 30 * 4
    # the reference's step on the same GPU: ef_loss + autograd through the module
    from oracle import losses
    sd = {n: p.detach().clone().to(dev).requires_grad_(True) for n, p in model.state_dict().items()}
    Xc = torch.as_tensor(traj[:B], device=dev)
    wc = torch.as_tensor(w[:B], device=dev, dtype=torch.float32)
    mod = copy.deepcopy(module).to(dev)

    def ref_step():
        Xr = Xc.clone().requires_grad_(True)
        loss = losses.ef_loss(sd, 2, mod, Xr, wc, alpha=20.0, eig_w=[1.0, 0.8], diag_coeff=a.to(dev))[0]
        torch.autograd.grad(loss, list(sd.values()))

    for _ in range(2):
        ref_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        ref_step()
    torch.cuda.synchronize()
    ref_us = (time.perf_counter() - t0) / 5 * 1e6
    print(json.dumps(dict(shape="pairs10 d_r=45 rho=30 k=2 nets[45,20,20,20,1]", frames=args.frames, batch=B,
                          record_build_s=round(build_s, 3), resident_bytes=task.resident_bytes,
                          step_us_graph=round(step_us, 1), train_call_s=round(total, 3),
                          metric_factor_us_events=round(k_us, 2), record_TBps=round(rec_bytes / k_us * 1e-6, 3),
                          ref_autograd_step_us=round(ref_us, 1), speedup=round(ref_us / step_us, 1))), flush=True)


if __name__ == "__main__":
    main()
