#!/usr/bin/env python3
"""A joint 2-D grid term inside the one-launch bias kernels, and hill deposition on the device (csrc/cv_bias.hip,
csrc/cv_bias_hills.hip), every variant replayed from a captured graph, B = 1 frame.

  shapes    c3, mixed1000 of tools/bench_cv_bias.py (k = 3: the grid lies on CV 0 and CV 1)
  variants  plain          ONE cvf_cv_frame[_large]_eval with a coef that is already there: the launch without a bias
            grid2d         (a) cvf_cv_frame[_large]_bias_eval with one 64 x 64 joint grid on (CV 0, CV 1)
            tables1d       (b) the same launch with two 64-node 1-D tables, on CV 0 and on CV 1: what a description could say before
                           the joint grid - the baseline of (a)
            tables1d2      (b) a second time: the tool's own run-to-run spread
            tables1d_old   (c) with --parent-lib PATH, a libcvf_hip.so built from the commit before the 2-D fields (a cvf_bias_term of
                           32 bytes): (b) on that library in the same process - did the 1-D path move?
            deposit1/8     (d) cvf_cv_bias_deposit alone (two launches) on the 64 x 64 grid, B = 1 and B = 8 hills

Method (tools/bench_cv_bias.py's): HIP events around a window of --replays (200) back-to-back graph replays, time per evaluation
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


class OldTerm(C.Structure):
    """cvf_bias_term before the 2-D fields."""
    _fields_ = _hip.BiasTerm._fields_[:8]


class OldDesc(C.Structure):
    _fields_ = [("n_terms", C.c_int32), ("n_table", C.c_int32), ("term", OldTerm * _hip.BIAS_MAX_TERMS), ("table", C.c_void_p)]


def old_desc(d):
    o = OldDesc()
    o.n_terms, o.n_table, o.table = d.n_terms, d.n_table, d.table
    for t in range(d.n_terms):
        assert d.term[t].n_nodes2 == 0
        for name, _ in OldTerm._fields_:
            setattr(o.term[t], name, getattr(d.term[t], name))
    return o


def build(shape, dev, parent):
    lib, P = _hip.lib(), _hip.ptr
    n, hidden, k, feature_case = SHAPES[shape]
    assert k >= 2
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
    plain_eval, bias_eval = getattr(lib, name + "_eval"), getattr(lib, name + "_bias_eval")
    assert getattr(lib, name + "_bias_supported")(mdesc, upto, pdesc) == 1, lib.cvf_last_error().decode()
    nc = 3 * n
    x = torch.tensor(traj, device=dev).reshape(1, nc).contiguous()
    xi, U, dU = torch.empty(1, k, device=dev), torch.empty(1, device=dev), torch.empty(1, k, device=dev)
    th = P(theta)
    _hip.check(plain_eval(mdesc, th, upto, pdesc, P(x), 1, None, P(xi), P(torch.empty(1, k, nc, device=dev)), _hip.stream()), "xi")
    c = [round(float(v), 2) for v in xi[0].cpu()]       # the grids are centred on the frame's xi: the interpolation is what is timed
    g = np.linspace(-2.0, 2.0, 64)
    h = float(g[1] - g[0])
    X, Y = np.meshgrid(g, g, indexing="ij")
    grid = {"kind": "table2d", "cv": 0, "cv2": 1, "lo": (c[0] - 2.0, c[1] - 2.0), "h": (h, h), "u": 0.1 * np.cos(3 * X) * np.cos(2 * Y),
            "d1": -0.3 * np.sin(3 * X) * np.cos(2 * Y), "d2": -0.2 * np.cos(3 * X) * np.sin(2 * Y), "d12": 0.6 * np.sin(3 * X) * np.sin(2 * Y)}
    tables = [{"kind": "table", "cv": i, "lo": c[i] - 2.0, "h": h, "u": 0.1 * np.cos(3 * g), "du": -0.3 * np.sin(3 * g)} for i in (0, 1)]
    desc2, tab2 = export.bias_desc([grid], k, dev)
    desc1, tab1 = export.bias_desc(tables, k, dev)
    descd, tabd = export.bias_desc([dict(grid, n=(64, 64))], k, dev)       # the grid the deposits go into
    coef0 = torch.randn(1, k, generator=torch.Generator().manual_seed(5)).to(dev)
    F = torch.zeros(1, nc, device=dev)
    centres = torch.tensor(np.array(c) + np.random.RandomState(2).uniform(-1.5, 1.5, size=(8, k)), dtype=torch.float32, device=dev)
    hills = torch.empty(8, 4, device=dev)
    hill = _hip.HillDesc(0, 0, 1e-4, 0.2, 0.2, 0.0)
    keep = [layer, nets, theta, tab1, tab2, tabd, desc1, desc2, descd, hill]

    def bias(fn, d, what):
        def run():
            _hip.check(fn(mdesc, th, upto, pdesc, d, None, P(x), 1, P(xi), P(U), P(dU), P(F), _hip.stream()), what)
        return run

    def plain():
        _hip.check(plain_eval(mdesc, th, upto, pdesc, P(x), 1, P(coef0), P(xi), P(F), _hip.stream()), "plain")

    def dep(B):
        def run():
            _hip.check(lib.cvf_cv_bias_deposit(descd, k, hill, P(centres), B, P(tabd), P(hills), _hip.stream()), "deposit")
        return run

    fns = {"plain": plain, "grid2d": bias(bias_eval, desc2, "grid2d"), "tables1d": bias(bias_eval, desc1, "tables1d"),
           "tables1d2": bias(bias_eval, desc1, "tables1d")}
    if parent is not None:
        fn_old = getattr(parent, name + "_bias_eval")
        fn_old.restype = C.c_int
        fn_old.argtypes = [C.POINTER(_hip.MLPDesc), C.c_void_p, C.c_int, C.POINTER(_hip.PPDesc), C.POINTER(OldDesc), C.c_void_p, C.c_void_p,
                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        od = old_desc(desc1)
        keep.append(od)
        fns["tables1d_old"] = bias(fn_old, od, "tables1d_old")
        # the two libraries give the same bits on the 1-D description
        got = []
        for v in ("tables1d", "tables1d_old"):
            F.zero_()
            fns[v]()
            torch.cuda.synchronize()
            got.append((U.clone(), dU.clone(), F.clone()))
        assert all(torch.equal(a, b) for a, b in zip(*got)), "the parent library and this one differ on the 1-D tables"
    fns["deposit1"], fns["deposit8"] = dep(1), dep(8)
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
    assert torch.cuda.is_available(), "bench_cv_bias2.py measures on the GPU"
    dev = torch.device("cuda:0")
    parent = C.CDLL(a.parent_lib) if a.parent_lib else None
    out = {"tool": "bench_cv_bias2", "gpu": torch.cuda.get_device_name(0), "replays": a.replays, "windows": a.windows, "rounds": a.rounds,
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
        out["results"][shape] = res
        if not lines:
            lines.append(f"{'shape':10s} " + " ".join(f"{v:>24s}" for v in res))
        lines.append(f"{shape:10s} " + " ".join(f"{r['median']:9.2f} [{r['min']:6.2f},{r['max']:6.2f}]" for r in res.values()))
        del graphs, replays, fns, keep
    print("\n".join(lines), file=sys.stderr)
    if a.summary:
        with open(a.summary, "w") as f:
            f.write(f"bench_cv_bias2 on {out['gpu']}: us per evaluation at B = 1, graph replays, median of the rounds' medians [min, max over rounds]; "
                    f"{a.replays} replays per window, {a.windows} windows per round, {a.rounds} rounds, variants alternating\n")
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
