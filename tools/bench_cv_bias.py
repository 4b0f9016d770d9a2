#!/usr/bin/env python3
"""Bias energy and forces along a CV per MD step: the one launch cvf_cv_frame_bias_eval / cvf_cv_frame_large_bias_eval
(csrc/cv_bias.hip) against what an engine does without it, every variant replayed from a captured graph, B = 1.

  shapes    c3         config 3: 22 atoms, all positions, d_r 66, nets [66,20,20,20,1] x 3      (the wave kernel)
            mixed1000  1000 atoms, 600 of them aligned, 80 mixed features, nets [132,20,20,1] x 3 (the workgroup kernel)
  bias      one harmonic restraint per CV and one 64-node table on CV 0
  variants  plain        ONE cvf_cv_frame[_large]_eval with a coef that is already there: the launch without the bias - what the
                         added bias arithmetic and the indexed addressing are measured against
            plain2       the same a second time: the tool's own run-to-run spread
            biased       cvf_cv_frame[_large]_bias_eval on the dense layout (layout = NULL)
            biased_md    the same through cvf_md_layout: the CV's atoms scattered over an engine of --engine-atoms atoms of 4 floats
            two_launch   the alternative: cvf_cv_frame[_large]_eval for xi, torch operators for coef = -dU/dxi (harmonic terms
                         only: three elementwise kernels), cvf_cv_frame[_large]_eval with coef; the engine's own gather and
                         scatter launches, which the MD layout also saves, are NOT counted

Method (tools/bench_cv_frame.py's): HIP events around a window of --replays (200) back-to-back graph replays, time per evaluation
= window / replays; per round and variant the median of --windows (3) windows; --rounds (5) rounds that alternate the variants;
reported per variant: the median of the rounds' medians and their spread (min, max), in microseconds.  One JSON line; --summary
PATH also writes a table."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench_cv_frame import SHAPES, captured, window_us  # noqa: E402

from colvarsfinder import _hip, core, export, nn, pp  # noqa: E402
from tests.synth import make_molecule_traj  # noqa: E402

VARIANTS = ("plain", "plain2", "biased", "biased_md", "two_launch")


def build(shape, dev, engine_atoms):
    lib, P = _hip.lib(), _hip.ptr
    n, hidden, k, feature_case = SHAPES[shape]
    large = shape != "c3"
    traj, _, ref = make_molecule_traj(n, 1, seed=17)
    if feature_case is None:
        layer = pp.AlignFeatureLayer(n, list(range(n)), ref, [("position", tuple(range(n)))]).to(dev)
    else:
        from tests.test_align_vjp_gpu import case
        _, align, feats, _ = case(feature_case)
        layer = pp.AlignFeatureLayer(n, align, ref[align], feats).to(dev)
    torch.manual_seed(11)
    nets = nn.EigenFunctions([layer.d_r] + hidden, k).to(dev)
    mdesc, upto, k, params = core._CVModel._nets_plan(nets)
    theta = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
    pdesc = layer.pp_desc()
    plain_eval = lib.cvf_cv_frame_large_eval if large else lib.cvf_cv_frame_eval
    bias_eval = lib.cvf_cv_frame_large_bias_eval if large else lib.cvf_cv_frame_bias_eval
    ok = (lib.cvf_cv_frame_large_bias_supported if large else lib.cvf_cv_frame_bias_supported)(mdesc, upto, pdesc)
    assert ok == 1, lib.cvf_last_error().decode()
    nc = 3 * n
    x = torch.tensor(traj, device=dev).reshape(1, nc).contiguous()
    kappa = torch.tensor([1.0 + 0.1 * i for i in range(k)], device=dev)
    center = torch.tensor([0.3 - 0.2 * i for i in range(k)], device=dev)
    harmonic = [("harmonic", i, float(kappa[i]), float(center[i])) for i in range(k)]
    grid = np.linspace(-2.0, 2.0, 64)
    table = {"kind": "table", "cv": 0, "lo": -2.0, "h": float(grid[1] - grid[0]), "u": 0.1 * np.cos(3 * grid), "du": -0.3 * np.sin(3 * grid)}
    desc, tab = export.bias_desc(harmonic + [table], k, dev)
    desc_h, _ = export.bias_desc(harmonic, k, dev)      # what two_launch computes with torch operators
    # the engine's arrays
    g = torch.Generator().manual_seed(5)
    index = torch.randperm(engine_atoms, generator=g)[:n].sort().values.to(torch.int32).to(dev)
    a = torch.arange(nc, device=dev)
    cols = index.long()[a // 3] * 4 + a % 3
    X_all = torch.zeros(1, engine_atoms * 4, device=dev)
    X_all[:, cols] = x
    F_all, F_dense = torch.zeros(1, engine_atoms * 4, device=dev), torch.zeros(1, nc, device=dev)
    layout = _hip.MDLayout(index.data_ptr(), 4, 0, engine_atoms * 4, engine_atoms * 4)
    xi, U, dU = torch.empty(1, k, device=dev), torch.empty(1, device=dev), torch.empty(1, k, device=dev)
    coef, coef0 = torch.empty(1, k, device=dev), torch.randn(1, k, generator=g).to(dev)
    J, Fx = torch.empty(1, k, nc, device=dev), torch.empty(1, nc, device=dev)
    keep = (layer, nets, theta, tab, index, desc, desc_h, layout)
    th = P(theta)

    def plain():
        _hip.check(plain_eval(mdesc, th, upto, pdesc, P(x), 1, P(coef0), P(xi), P(Fx), _hip.stream()), "plain")

    def biased():
        _hip.check(bias_eval(mdesc, th, upto, pdesc, desc, None, P(x), 1, P(xi), P(U), P(dU), P(F_dense), _hip.stream()), "biased")

    def biased_md():
        _hip.check(bias_eval(mdesc, th, upto, pdesc, desc, layout, P(X_all), 1, P(xi), P(U), P(dU), P(F_all), _hip.stream()), "biased_md")

    def two_launch():
        s = _hip.stream()
        _hip.check(plain_eval(mdesc, th, upto, pdesc, P(x), 1, None, P(xi), P(J), s), "two_launch 1")
        torch.sub(center, xi, out=coef)          # coef = -kappa (xi - c)
        coef.mul_(kappa)
        _hip.check(plain_eval(mdesc, th, upto, pdesc, P(x), 1, P(coef), P(xi), P(Fx), s), "two_launch 2")

    # the variants agree before anything is timed: harmonic terms only, dense against indexed against two launches
    F_dense.zero_()
    _hip.check(bias_eval(mdesc, th, upto, pdesc, desc_h, None, P(x), 1, P(xi), P(U), P(dU), P(F_dense), _hip.stream()), "check")
    two_launch()
    torch.cuda.synchronize()
    diff = float((F_dense - Fx).abs().max() / Fx.abs().max())
    F_dense.zero_()
    biased()
    biased_md()
    torch.cuda.synchronize()
    assert torch.equal(F_all[:, cols], F_dense), "the indexed layout and the dense one differ"
    return {"plain": plain, "plain2": plain, "biased": biased, "biased_md": biased_md, "two_launch": two_launch}, diff, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="c3,mixed1000")
    ap.add_argument("--engine-atoms", type=int, default=100000)
    ap.add_argument("--summary", default=None)
    a = ap.parse_args()
    assert a.replays >= 200 and a.rounds >= 3, "at least 200 replays per window and three rounds"
    assert torch.cuda.is_available(), "bench_cv_bias.py measures on the GPU"
    dev = torch.device("cuda:0")
    out = {"tool": "bench_cv_bias", "gpu": torch.cuda.get_device_name(0), "replays": a.replays, "windows": a.windows, "rounds": a.rounds,
           "engine_atoms": a.engine_atoms, "unit": "us per evaluation, B = 1, graph replays", "results": {}}
    lines = [f"{'shape':10s} " + " ".join(f"{v:>24s}" for v in VARIANTS) + "   biased/plain  biased_md/plain  two_launch/biased  plain2/plain"]
    for shape in [s for s in a.shapes.split(",") if s]:
        fns, diff, keep = build(shape, dev, a.engine_atoms)
        replays, graphs = {}, []
        for v, fn in fns.items():
            replays[v], g = captured(fn)
            graphs.append(g)
        for fn in replays.values():
            window_us(fn, 20)
        rounds = {v: [] for v in replays}
        for _ in range(a.rounds):
            for v in replays:            # the variants alternate inside a round
                rounds[v].append(statistics.median(window_us(replays[v], a.replays) for _ in range(a.windows)))
        res = {v: {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)} for v, t in rounds.items()}
        res["rel_diff_two_launch"] = diff
        out["results"][shape] = res
        m = lambda v: res[v]["median"]
        lines.append(f"{shape:10s} " + " ".join(f"{m(v):9.2f} [{res[v]['min']:6.2f},{res[v]['max']:6.2f}]" for v in VARIANTS)
                     + f"   {m('biased') / m('plain'):.3f}  {m('biased_md') / m('plain'):.3f}  {m('two_launch') / m('biased'):.3f}  {m('plain2') / m('plain'):.3f}"
                     + f"   (force rel diff one launch vs two {diff:.1e})")
        del graphs, replays, fns, keep
    print("\n".join(lines), file=sys.stderr)
    if a.summary:
        with open(a.summary, "w") as f:
            f.write(f"bench_cv_bias on {out['gpu']}: us per evaluation at B = 1, graph replays, median of the rounds' medians [min, max over rounds]; "
                    f"{a.replays} replays per window, {a.windows} windows per round, {a.rounds} rounds, variants alternating\n")
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
