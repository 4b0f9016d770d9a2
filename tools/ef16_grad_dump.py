"""Developer tool (GPU): the flat gradient of ONE 16-frame train step at B = 87 (n_rec = 22, D = 66, k = 3) for several hidden
shapes in both modes, as OUT/grad_<mode>_h<H>x<NH>.npy - run it in two trees (it imports the tree it lies in) and compare the
files' bytes:   python tools/ef16_grad_dump.py OUT            (in each tree)
                python tools/ef16_grad_dump.py --compare A B  (anywhere)
The batches are those of tests/test_ef16_back_tail4_gpu.py (tests.synth, seed 7300 + the shape's position)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd")):
    sys.path.insert(0, p)

SHAPES = ((16,), (20, 20, 20), (24, 24), (32, 32))
B, N_REC, K, LAG = 87, 22, 3, 2


def dump(out):
    import torch
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    from tests.synth import Traj, diag_coeff_for, make_molecule_traj
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda:0")
    for s, hidden in enumerate(SHAPES):
        for mode in ("gen", "tr"):
            lag = 0 if mode == "gen" else LAG
            traj, w, ref = make_molecule_traj(N_REC, B + lag, seed=7300 + s, scale=2.0, sigma=0.3)
            layer = pp.AlignFeatureLayer(N_REC, list(range(N_REC)), ref, [("position", tuple(range(N_REC)))], False).to(dev)
            dims = [layer.d_r] + list(hidden) + [1]
            model = nn.EigenFunctions(dims, K)
            model.load_state_dict(nnref.init_eigenfunctions(dims, K, torch.Generator().manual_seed(17 + K)))
            a = torch.tensor(diag_coeff_for(N_REC, 3), dtype=torch.float32) if mode == "gen" else None
            task = core.EigenFunctionTask(Traj(traj[:64 + lag], w[:64 + lag], 0.5), layer, model, "/tmp/cvf_test", 12.0,
                                          [1.0 - 0.1 * i for i in range(K)], diag_coeff=a, beta=1.2, lag_tau=lag * 0.5, k=K, device=dev,
                                          verbose=False, save_model_every_step=0)
            X, wt = torch.tensor(traj[:B]), torch.tensor(w[:B])
            Xl, wl = (None, None) if lag == 0 else (torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B]))
            task.loss_func(X, wt, Xl, wl)
            task.backward()
            torch.cuda.synchronize()
            assert task._route.kind == "ef16", task._route
            g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
            assert np.isfinite(g).all()
            np.save(os.path.join(out, f"grad_{mode}_h{hidden[0]}x{len(hidden)}.npy"), g)


def compare(a, b):
    bad = 0
    for name in sorted(os.listdir(a)):
        if not name.endswith(".npy"):
            continue
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        if x.shape == y.shape and x.tobytes() == y.tobytes():
            print(f"{name} identical bytes ({x.size} values)")
        else:
            bad += 1
            n = int((x != y).sum()) if x.shape == y.shape else -1
            print(f"{name} DIFFER in {n} of {x.size}")
    return bad


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    dump(sys.argv[1])
