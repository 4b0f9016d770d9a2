#!/usr/bin/env python3
"""Data-parallel check of RegAutoEncoderTask(general_nets=True) on ONE GPU: the dipeptide chain [66,128,128,2 | 2,128,128,66] with
two regularisers [2,128,128,1] in generator mode (the shared-trunk launches of csrc/ef_general.hip), the same training run once
in a single process and once as two ranks (both on cuda:0, `gloo` process group).  Prints one JSON line; exit status 1 when the
runs disagree.
    python tools/check_dp2_regae_shared.py       (parent: runs the single-process run, spawns the two ranks, compares)
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


def run(out_path):
    import torch
    from colvarsfinder import _dist, core, nn, pp
    from tests.synth import Traj, make_molecule_traj
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        _dist.init_from_env("gloo")
    n_atoms = 22
    traj, w, ref = make_molecule_traj(n_atoms, 1300, seed=321)
    layer = pp.AlignFeatureLayer(n_atoms, list(range(n_atoms)), ref, [("position", tuple(range(n_atoms)))])
    torch.manual_seed(9)
    np.random.seed(13)
    model = nn.RegAutoEncoder([66, 128, 128, 2], [2, 128, 128, 66], [2, 128, 128, 1], 2)
    task = core.RegAutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_dp2_regae_shared", eig_weights=[1.0, 0.7],
                                   learning_rate=1e-3, batch_size=500, num_epochs=2, gamma=[1.0, 1.0], device=dev, verbose=False,
                                   save_model_every_step=0, general_nets=True)
    assert task._gen is not None and task._gen.shared and task._gen.inner._route.shared == 2
    task.train()
    torch.cuda.synchronize()
    if _dist.rank() == 0:
        losses = np.concatenate([np.asarray(e[0]).reshape(len(e[0]), -1) for e in task.loss_list])
        # (each regulariser net's last bias has exact gradient 0 and random-walks on roundoff under Adam in any run)
        params = np.concatenate([p.detach().cpu().numpy().reshape(-1) for n, p in model.named_parameters()
                                 if not (n.startswith("reg.") and n.endswith(".3.bias"))])
        np.savez(out_path, losses=losses, params=params)
    if _dist.world() > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        return run(sys.argv[2])
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    one, two = f"/tmp/dp2rs_{os.getpid()}_w1.npz", f"/tmp/dp2rs_{os.getpid()}_w2.npz"
    subprocess.run([sys.executable, __file__, "worker", one], check=True, env=env, timeout=200)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    procs = [subprocess.Popen([sys.executable, __file__, "worker", two],
                              env=dict(env, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port))
             for r in range(2)]
    if any(p.wait(timeout=200) != 0 for p in procs):
        raise SystemExit("a rank failed")
    a, b = np.load(one), np.load(two)
    dl = float(np.max(np.abs(a["losses"] - b["losses"]) / np.maximum(np.abs(a["losses"]), 1e-3)))
    dp = float(np.max(np.abs(a["params"] - b["params"])))
    ok = dl < 2e-4 and dp < 2e-3
    for f in (one, two):
        os.remove(f)
    print(json.dumps(dict(ok=ok, shared=True, steps=int(a["losses"].shape[0]), max_rel_loss_diff=dl, max_abs_param_diff=dp)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
