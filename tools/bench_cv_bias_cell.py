#!/usr/bin/env python3
"""Periodic cells inside the one-launch bias kernels: whole molecules and the virial (csrc/cv_bias.hip, csrc/cvf_cell.hpp;
DESIGN.md 4.20), every variant replayed from its own captured graph, B = 1 frame, in an engine's layout (4 floats per atom, a
shuffled atom_index with 5 more engine atoms).

  shapes    c3, mixed1000 of tools/bench_cv_bias.py (one harmonic term per CV)
  variants  layout       (a) cvf_cv_frame[_large]_bias_eval through cvf_md_layout: the launch as it was
            layout2      (a) a second time: the tool's own run-to-run spread
            layout_old   with --parent-lib PATH, a libcvf_hip.so built from the commit before the cell: (a) on that library in the same
                         process - did the existing path move?
            cell         (b) cvf_cv_frame[_large]_bias_cell_eval on the torn frame (every atom wrapped and shifted)
            cell_virial  (c) (b) with virial_rows
            whole_then   (d) cvf_md_make_whole into a dense frame, then (a) on it with a NULL layout: what an engine does without the
                         cell launch (its scatter of the dense force back into the engine's array is NOT counted)

Method (tools/bench_cv_bias2.py's): HIP events around a window of --replays (200) back-to-back graph replays, time per evaluation
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
from tests import cv_cell_cases as Cc  # noqa: E402
from tests.synth import make_molecule_traj  # noqa: E402


def build(shape, dev, parent):
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
    name = "cvf_cv_frame_large" if large else "cvf_cv_frame"
    bias_eval, cell_eval = getattr(lib, name + "_bias_eval"), getattr(lib, name + "_bias_cell_eval")
    assert getattr(lib, name + "_bias_cell_supported")(mdesc, upto, pdesc) == 1, lib.cvf_last_error().decode()
    nc = 3 * n
    # the cell (dyadic triclinic, scaled to the molecule) and the torn frame in the engine's layout
    d = float(np.abs(np.diff(traj[0].astype(np.float64), axis=0)).max())
    cell = (Cc.DYADIC * 2.0 ** np.ceil(np.log2(2.5 * d / 2.0))).astype(np.float32)
    torn = Cc.tear(cell, traj[0], np.random.RandomState(3), shifts=2, keep_first=True, centred=True)
    n_total, stride = n + 5, 4
    index = torch.randperm(n_total, generator=torch.Generator().manual_seed(1))[:n].to(torch.int32)
    a = torch.arange(nc)
    cols = (index.long()[a // 3] * stride + a % 3).to(dev)
    X_whole, X_torn = torch.zeros(1, n_total * stride, device=dev), torch.zeros(1, n_total * stride, device=dev)
    X_whole[:, cols] = torch.tensor(traj, device=dev).reshape(1, nc)
    X_torn[:, cols] = torch.tensor(torn, device=dev).reshape(1, nc)
    F_all, F_dense, x_dense = torch.zeros(1, n_total * stride, device=dev), torch.zeros(1, nc, device=dev), torch.zeros(1, nc, device=dev)
    index = index.to(dev)
    layout = _hip.MDLayout(index.data_ptr(), stride, 0, n_total * stride, n_total * stride)
    cell_t, vir = torch.tensor(cell, device=dev), torch.zeros(1, 9, device=dev)
    mc, mcv = _hip.MDCell(cell_t.data_ptr(), 0, None), _hip.MDCell(cell_t.data_ptr(), 0, vir.data_ptr())
    xi, U, dU = torch.empty(1, k, device=dev), torch.empty(1, device=dev), torch.empty(1, k, device=dev)
    desc, tab = export.bias_desc([{"kind": "harmonic", "cv": i, "kappa": 1.0 + 0.1 * i, "center": 0.5} for i in range(k)], k, dev)
    th = P(theta)
    keep = [layer, nets, theta, desc, tab, index, cell_t]

    def layout_run(fn, what):
        def run():
            _hip.check(fn(mdesc, th, upto, pdesc, desc, layout, P(X_whole), 1, P(xi), P(U), P(dU), P(F_all), _hip.stream()), what)
        return run

    def cell_run(m, what):
        def run():
            _hip.check(cell_eval(mdesc, th, upto, pdesc, desc, layout, P(X_torn), 1, P(xi), P(U), P(dU), P(F_all), _hip.stream(), m), what)
        return run

    def whole_then():
        _hip.check(lib.cvf_md_make_whole(layout, mc, P(X_torn), n, 1, P(x_dense), _hip.stream()), "make_whole")
        _hip.check(bias_eval(mdesc, th, upto, pdesc, desc, None, P(x_dense), 1, P(xi), P(U), P(dU), P(F_dense), _hip.stream()), "whole_then")

    fns = {"layout": layout_run(bias_eval, "layout"), "layout2": layout_run(bias_eval, "layout2")}
    if parent is not None:
        fn_old = getattr(parent, name + "_bias_eval")
        fn_old.restype, fn_old.argtypes = C.c_int, _hip._SIGNATURES[name + "_bias_eval"][1]
        fns["layout_old"] = layout_run(fn_old, "layout_old")
        got = []
        for v in ("layout", "layout_old"):       # the two libraries give the same bits
            F_all.zero_()
            fns[v]()
            torch.cuda.synchronize()
            got.append((U.clone(), dU.clone(), F_all.clone()))
        assert all(torch.equal(p, q) for p, q in zip(*got)), "the parent library and this one differ on the layout launch"
    fns["cell"], fns["cell_virial"], fns["whole_then"] = cell_run(mc, "cell"), cell_run(mcv, "cell_virial"), whole_then
    return fns, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="c3,mixed1000")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--summary", default=None)
    a = ap.parse_args()
    assert a.replays >= 200 and a.rounds >= 3, "at least 200 replays per window and three rounds"
    assert torch.cuda.is_available(), "bench_cv_bias_cell.py measures on the GPU"
    dev = torch.device("cuda:0")
    parent = C.CDLL(a.parent_lib) if a.parent_lib else None
    out = {"tool": "bench_cv_bias_cell", "gpu": torch.cuda.get_device_name(0), "replays": a.replays, "windows": a.windows, "rounds": a.rounds,
           "unit": "us per evaluation, B = 1, graph replays", "results": {}}
    lines = []
    for shape in [s for s in a.shapes.split(",") if s]:
        fns, keep = build(shape, dev, parent)
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
        m = {v: r["median"] for v, r in res.items()}
        res["differences"] = {"cell - layout": round(m["cell"] - m["layout"], 3), "cell_virial - cell": round(m["cell_virial"] - m["cell"], 3),
                              "whole_then - cell": round(m["whole_then"] - m["cell"], 3)}
        out["results"][shape] = res
        cols = [v for v in res if v != "differences"]
        if not lines:
            lines.append(f"{'shape':10s} " + " ".join(f"{v:>24s}" for v in cols))
        lines.append(f"{shape:10s} " + " ".join(f"{res[v]['median']:9.2f} [{res[v]['min']:6.2f},{res[v]['max']:6.2f}]" for v in cols))
        lines.append(f"{'':10s} " + "   ".join(f"{key} = {val:+.2f}" for key, val in res["differences"].items()))
        del graphs, replays, fns, keep
    print("\n".join(lines), file=sys.stderr)
    if a.summary:
        with open(a.summary, "w") as f:
            f.write(f"bench_cv_bias_cell on {out['gpu']}: us per evaluation at B = 1, graph replays, median of the rounds' medians [min, max over rounds]; "
                    f"{a.replays} replays per window, {a.windows} windows per round, {a.rounds} rounds, variants alternating\n")
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
