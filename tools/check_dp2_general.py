#!/usr/bin/env python3
"""Data-parallel check of the general eigenfunction route (EigenFunctionTask(general_nets=True), csrc/ef_general.hip) on ONE
GPU: the same training run once in a single process and once as two ranks (both on cuda:0, `gloo` process group, eager
launches).  The nets have more than 262 144 parameters, past the peer-to-peer window of cvf_slab_reduce_dp: the gradient is
summed by cvf_slab_reduce + the all-reduce.  Prints one JSON line; exit status 1 when the runs disagree.
    python tools/check_dp2_general.py            (parent: runs the single-process run, spawns the two ranks, compares)
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd")):
    sys.path.insert(0, p)

DIMS = [66, 384, 384, 1]
K = 2


def run(kind, out_path):
    import torch
    from colvarsfinder import _dist, core, nn, pp
    from tests.synth import Traj, diag_coeff_for, make_molecule_traj
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        _dist.init_from_env("gloo")
    n_atoms = 22
    traj, w, ref = make_molecule_traj(n_atoms, 3000, seed=321)
    layer = pp.AlignFeatureLayer(n_atoms, list(range(n_atoms)), ref, [("position", tuple(range(n_atoms)))])
    torch.manual_seed(9)
    np.random.seed(13)
    model = nn.EigenFunctions(DIMS, K)
    a = torch.tensor(diag_coeff_for(n_atoms, 5), dtype=torch.float32) if kind == "gen" else None
    task = core.EigenFunctionTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_dp2_general", 20.0, [1.0, 0.7], diag_coeff=a, beta=1.0,
                                  lag_tau=0 if kind == "gen" else 1.0, learning_rate=1e-3, k=K, batch_size=1000, num_epochs=2,
                                  device=dev, verbose=False, save_model_every_step=0, general_nets=True)
    assert task._general and task._flat.n > 262144
    task.train()
    torch.cuda.synchronize()
    if _dist.rank() == 0:
        losses = np.concatenate([np.asarray(e[0]).reshape(len(e[0]), -1) for e in task.loss_list])
        # (each net's output bias - its last parameter - has exact gradient 0 and random-walks on roundoff under Adam in any run)
        last = set({n.split(".")[1]: n for n, _ in model.named_parameters()}.values())
        params = np.concatenate([p.detach().cpu().numpy().reshape(-1) for n, p in model.named_parameters() if n not in last])
        np.savez(out_path, losses=losses, params=params, n_params=task._flat.n)
    if _dist.world() > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        return run(sys.argv[2], sys.argv[3])
    report, ok = {}, True
    for kind in ("gen", "tr"):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
        env["CVF_GRAPH"] = "0"
        one, two = f"/tmp/dp2g_{kind}_{os.getpid()}_w1.npz", f"/tmp/dp2g_{kind}_{os.getpid()}_w2.npz"
        subprocess.run([sys.executable, __file__, "worker", kind, one], check=True, env=env, timeout=300)
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = str(sk.getsockname()[1])
        procs = [subprocess.Popen([sys.executable, __file__, "worker", kind, two],
                                  env=dict(env, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port))
                 for r in range(2)]
        if any(p.wait(timeout=300) != 0 for p in procs):
            raise SystemExit(f"a rank failed ({kind})")
        a, b = np.load(one), np.load(two)
        dl = float(np.max(np.abs(a["losses"] - b["losses"]) / np.maximum(np.abs(a["losses"]), 1e-3)))
        dp = float(np.max(np.abs(a["params"] - b["params"])))
        report[kind] = dict(steps=int(a["losses"].shape[0]), n_params=int(a["n_params"]), max_rel_loss_diff=dl, max_abs_param_diff=dp)
        ok = ok and dl < 2e-4 and dp < 2e-3
        for f in (one, two):
            os.remove(f)
    print(json.dumps(dict(ok=ok, **report)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
