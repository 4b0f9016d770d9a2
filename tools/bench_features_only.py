#!/usr/bin/env python3
"""A feature layer WITHOUT alignment (pp.AlignFeatureLayer(n, None, None, features), CVF_PP_FEATURES, csrc/k1_features.hip) beside
the aligned layer built on the SAME feature list: HIP-event times of cvf_align_feature_fwd (tiled output, as the training step
calls it) and of one generator-mode EigenFunctionTask.train_step (hipGraph replay of a resident batch), at

  config-5 shape   5000 atoms, 128 dihedrals + 128 bonds (d_r = 384), 16 000 frames, k = 6 nets [384, 20, 20, 20, 1]
                   - "local": every feature on atoms that are neighbours in the index, as bonded atoms of a topology are;
                   - "spread": every feature's atoms drawn over the whole frame, as bench.c5_features draws them;
  22 atoms         10 dihedrals + 12 bonds along the chain (d_r = 32), 20 000 frames, k = 3 nets [32, 20, 20, 20, 1].

The two layers alternate inside every round (the machine is shared: a difference counts only beyond the rounds' spread); a row
reports the median over the rounds and their min .. max.  Algorithmic bytes per frame of the forward: the feature atoms' 12 B
each plus 4 d_r out (new), the whole frame's 12 N plus 4 d_r and the 72 B of alignment rows (aligned).
    python tools/bench_features_only.py [--rounds 7] [--summary FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import bench  # noqa: E402
from colvarsfinder import _hip, core, nn, pp  # noqa: E402
from tests.synth import Traj, diag_coeff_for  # noqa: E402

dev = torch.device("cuda:0")
lib, P = _hip.lib(), _hip.ptr


def chain_features(n_atoms, n_dih, n_bond, seed, local):
    rs = np.random.RandomState(seed)

    def pick(m):
        if local:
            a0 = int(rs.randint(0, n_atoms - m + 1))
            return tuple(range(a0, a0 + m))
        return tuple(int(i) for i in rs.choice(n_atoms, m, replace=False))

    return [("dihedral", pick(4)) for _ in range(n_dih)] + [("bond", pick(2)) for _ in range(n_bond)]


def once(fn, reps):
    """Median of `reps` event-timed calls, us."""
    evs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
    return t[len(t) // 2]


def interleaved(fns, rounds, reps):
    """{name: (median, min, max)} over `rounds` rounds in which the functions alternate."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            got[name].append(once(fn, reps))
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in got.items()}


def forward_fn(layer, x, B):
    desc = layer.pp_desc()
    feat = torch.empty(_hip.ntiles(B) * layer.d_r * _hip.TILE, device=dev)
    aux = torch.empty(_hip.ntiles(B) * _hip.AUX_ROWS * _hip.TILE, device=dev)
    scratch = _hip.align_scratch(desc, B, dev)
    s = _hip.stream()
    keep = (desc, feat, aux, scratch)

    def fn():
        _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, P(feat), None, P(aux), P(scratch), s), "cvf_align_feature_fwd")

    fn.keep = keep
    return fn, feat


def step_fn(layer, x, w, B, k, hidden, n_atoms):
    dims = [layer.d_r] + hidden + [1]
    torch.manual_seed(3)
    model = nn.EigenFunctions(dims, k)
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    tok = x[:64].cpu().numpy()
    task = core.EigenFunctionTask(Traj(tok, np.ones(64), 0.5), layer, model, "/tmp/cvf_bench_features_only", 12.0,
                                  [1.0 - 0.1 * i for i in range(k)], diag_coeff=a, beta=1.0, lag_tau=0, learning_rate=1e-3, k=k,
                                  device=dev, verbose=False, save_model_every_step=0)
    log = torch.zeros(3 + 2 * k, device=dev, dtype=torch.float64)
    X = x.reshape(B, -1)

    def fn():
        task._graph_call(("bench", 0), lambda: task.train_step(X, w, out=log))

    fn.task = task
    return fn


def shape(label, n_atoms, feats, B, k, hidden, rounds):
    ref = np.random.RandomState(bench.SEED).normal(scale=2.0, size=(n_atoms, 3))
    x, w = bench.device_frames(B, ref, 0.3, bench.SEED + 21, dev, chunk=4000)
    new = pp.AlignFeatureLayer(n_atoms, None, None, feats).to(dev)
    old = pp.AlignFeatureLayer(n_atoms, list(range(n_atoms)), ref, feats).to(dev)
    f_new, feat_new = forward_fn(new, x, B)
    f_old, feat_old = forward_fn(old, x, B)
    fwd = interleaved({"features_only": f_new, "aligned": f_old}, rounds, 10)
    diff = float((feat_new - feat_old).abs().max() / feat_old.abs().max())   # invariant features: the same numbers
    s_new, s_old = step_fn(new, x, w, B, k, hidden, n_atoms), step_fn(old, x, w, B, k, hidden, n_atoms)
    step = interleaved({"features_only": s_new, "aligned": s_old}, rounds, 10)
    row = dict(shape=label, n_atoms=n_atoms, d_r=new.d_r, frames=B, feature_atoms=new._n_slot, contribution_rows=new._n_ref, k=k,
               bytes_per_frame=dict(features_only=12 * new._n_slot + 4 * new.d_r, aligned=12 * n_atoms + 4 * new.d_r + 4 * _hip.AUX_ROWS),
               routes=dict(features_only=s_new.task._route.kind, aligned=s_old.task._route.kind),
               max_rel_diff_of_the_two_forwards=float(f"{diff:.2e}"))
    for what, res in (("fwd_us", fwd), ("train_step_us", step)):
        row[what] = {name: dict(median=round(m, 1), min=round(lo, 1), max=round(hi, 1)) for name, (m, lo, hi) in res.items()}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--summary", default=None, help="also write the table as text to this file")
    args = ap.parse_args()
    na5 = bench.C5["n_atoms"]
    rows = [shape("config-5 local", na5, chain_features(na5, 128, 128, bench.SEED + 5, True), 16000, 6, [20, 20, 20], args.rounds),
            shape("config-5 spread", na5, chain_features(na5, 128, 128, bench.SEED + 5, False), 16000, 6, [20, 20, 20], args.rounds),
            shape("22 atoms", 22, [("dihedral", (i, i + 1, i + 2, i + 3)) for i in range(0, 20, 2)] +
                  [("bond", (i, i + 1)) for i in range(0, 12)], 20000, 3, [20, 20, 20], args.rounds)]
    print(json.dumps(dict(tool="bench_features_only", rounds=args.rounds, measured=rows)))
    if args.summary:
        with open(args.summary, "w") as f:
            f.write(f"tools/bench_features_only.py --rounds {args.rounds}: median [min .. max] over the rounds, us; the two layers alternate\n")
            for r in rows:
                f.write(f"\n{r['shape']}: {r['n_atoms']} atoms, d_r = {r['d_r']}, {r['frames']} frames, {r['feature_atoms']} feature atoms, "
                        f"k = {r['k']}; algorithmic bytes per frame of the forward: features only {r['bytes_per_frame']['features_only']}, "
                        f"aligned {r['bytes_per_frame']['aligned']}; step routes {r['routes']}; "
                        f"max rel. difference of the two forwards {r['max_rel_diff_of_the_two_forwards']}\n")
                for what in ("fwd_us", "train_step_us"):
                    for name, v in r[what].items():
                        f.write(f"  {what:14s} {name:14s} {v['median']:9.1f}  [{v['min']:.1f} .. {v['max']:.1f}]\n")


if __name__ == "__main__":
    main()
