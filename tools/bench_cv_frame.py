#!/usr/bin/env python3
"""xi(x) and d xi / d x for small batches: the one-launch entries cvf_cv_frame_eval (csrc/cv_frame.hip; one wave
per frame, at most 64 atoms) and cvf_cv_frame_large_eval (csrc/cv_frame_large.hip; one workgroup per frame, any
size) against the three-call recipe cvf_align_feature_fwd -> cvf_cv_nets_eval -> cvf_align_feature_vjp_rows, in one process.

  shapes    c3         config 3: 22 atoms, all positions, d_r 66, nets [66,20,20,20,1] x 3
            dipeptide  the dipeptide notebook: 10 atoms, all positions, d_r 30, nets [30,20,20,20,1] x 2
            mixed1000  1000 atoms, 600 of them aligned, 80 mixed features (d_r 132), nets [132,20,20,1] x 3
            c5         the config-5 layer: 5000 atoms, d_r 384, nets [384,20,20,1] x 6
  batches   B = 1, 8, 64, 1024
  variants  three_eager   the three calls issued from the host each time
            three_graph   the same launches replayed from one captured hipGraph (single stream) - the yardstick
            frame_eager   cvf_cv_frame_eval issued from the host each time
            frame_graph   the same launch replayed from a graph
            frame_large_eager, frame_large_graph   the same for cvf_cv_frame_large_eval
            (a variant whose predicate declines the shape - the wave kernel past 64 atoms - is left out of that shape's row)

Method: HIP events around a window of --replays (200) back-to-back evaluations, time per evaluation = window / replays; per
round and variant the median of --windows (3) windows; --rounds (3) rounds that alternate the variants; reported per variant: the
median of the rounds' medians and their spread (min, max), in microseconds.  Before timing, the two routes' J are compared.
Buffers are allocated once; nothing is allocated inside a window.  One JSON line; --summary PATH also writes a table.

--shared measures form C (k scalar chains on one trunk: cvf_cv_frame_shared_eval, cvf_cv_frame_large_shared_eval,
cvf_cv_nets_shared_eval) against form A - the entries above on the SAME aliased description and theta - on config
3's layer, every route replayed from a captured graph, with and without coef:

  models    narrow     trunk [66, 20, 20], head [20, 1], k = 3
            wide       trunk [66, 64, 64], head [64, 1], k = 8
  variants  per route (frame, frame_large, three): A, A2 (form A a second time: the tool's own run-to-run spread) and C, alternating
            inside a round; with coef the three-call recipe contracts d xi / d r with coef (one bmm) before cvf_align_feature_vjp"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from colvarsfinder import _hip, core, nn, pp  # noqa: E402
from tests.synth import make_molecule_traj  # noqa: E402

# (atoms, the nets' hidden dims behind d_r, k, named feature case of tests/test_align_vjp_gpu.case or None = all positions)
SHAPES = {"c3": (22, [20, 20, 20, 1], 3, None), "dipeptide": (10, [20, 20, 20, 1], 2, None),
          "mixed1000": (1000, [20, 20, 1], 3, "mixed1000"), "c5": (5000, [20, 20, 1], 6, "c5")}
BATCHES = (1, 8, 64, 1024)
VARIANTS = ("three_eager", "three_graph", "frame_eager", "frame_graph", "frame_large_eager", "frame_large_graph")


def build(shape, B, dev):
    """The routes as closures over preallocated buffers: (three(), frame() or None, large() or None, J of each, buffers)."""
    lib, P = _hip.lib(), _hip.ptr
    n, hidden, k, feature_case = SHAPES[shape]
    traj, _, ref = make_molecule_traj(n, B, seed=17)
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
    has_frame = lib.cvf_cv_frame_supported(mdesc, upto, pdesc) == 1
    has_large = lib.cvf_cv_frame_large_supported(mdesc, upto, pdesc) == 1
    assert has_frame or has_large, lib.cvf_last_error().decode()
    x = torch.tensor(traj, device=dev).reshape(B, -1).contiguous()
    T, d_r, nc = _hip.ntiles(B), layer.d_r, 3 * n
    r_t = torch.empty(T, d_r, _hip.TILE, device=dev)
    aux = torch.empty(T, _hip.AUX_ROWS, _hip.TILE, device=dev)
    G = torch.empty(B, k, d_r, device=dev)
    ws = torch.empty(lib.cvf_cv_nets_scratch_floats(mdesc, upto, B, 1), device=dev)
    xi3, J3 = torch.empty(B, k, device=dev), torch.empty(B, k, nc, device=dev)
    xi1, J1 = torch.empty(B, k, device=dev), torch.empty(B, k, nc, device=dev)
    xi2, J2 = torch.empty(B, k, device=dev), torch.empty(B, k, nc, device=dev)
    scratch = _hip.align_scratch(pdesc, B, dev)   # (None for small molecules)
    keep = (layer, nets, theta, x, r_t, aux, G, ws, scratch)

    def three():
        s = _hip.stream()
        _hip.check(lib.cvf_align_feature_fwd(pdesc, P(x), B, P(r_t), None, P(aux), P(scratch), s), "cvf_align_feature_fwd")
        _hip.check(lib.cvf_cv_nets_eval(mdesc, P(theta), upto, None, P(r_t), B, P(xi3), P(G), None, P(ws), s), "cvf_cv_nets_eval")
        _hip.check(lib.cvf_align_feature_vjp_rows(pdesc, P(x), B, P(aux), k, P(G), P(J3), s), "cvf_align_feature_vjp_rows")

    def frame():
        _hip.check(lib.cvf_cv_frame_eval(mdesc, P(theta), upto, pdesc, P(x), B, None, P(xi1), P(J1), _hip.stream()), "cvf_cv_frame_eval")

    def large():
        _hip.check(lib.cvf_cv_frame_large_eval(mdesc, P(theta), upto, pdesc, P(x), B, None, P(xi2), P(J2), _hip.stream()),
                   "cvf_cv_frame_large_eval")

    return three, (frame if has_frame else None), (large if has_large else None), J3, J1, J2, keep


def captured(fn):
    """fn's launches as one graph on a single stream; returns the replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay, g


def window_us(fn, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / replays


SHARED_MODELS = {"narrow": ([20, 20], [20, 1], 3), "wide": ([64, 64], [64, 1], 8)}


def build_shared(model, B, dev, with_coef):
    """{(route, form): closure} over preallocated buffers for a SharedEigenFunctions on config 3's layer; form "A" is the existing
    entry on the form-C description (aliased offsets, the same theta), form "C" the _shared one.  Also the outputs per closure."""
    lib, P = _hip.lib(), _hip.ptr
    n = 22
    traj, _, ref = make_molecule_traj(n, B, seed=17)
    layer = pp.AlignFeatureLayer(n, list(range(n)), ref, [("position", tuple(range(n)))]).to(dev)
    trunk, head, k = SHARED_MODELS[model]
    torch.manual_seed(11)
    nets = nn.SharedEigenFunctions([layer.d_r] + trunk, head, k).to(dev)
    mdesc, L, k, params, ns = core._CVModel._nets_plan_shared(nets)
    theta = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
    pdesc = layer.pp_desc()
    for ok in (lib.cvf_cv_frame_supported(mdesc, L, pdesc), lib.cvf_cv_frame_shared_supported(mdesc, ns, pdesc),
               lib.cvf_cv_frame_large_supported(mdesc, L, pdesc), lib.cvf_cv_frame_large_shared_supported(mdesc, ns, pdesc)):
        assert ok == 1, lib.cvf_last_error().decode()
    x = torch.tensor(traj, device=dev).reshape(B, -1).contiguous()
    T, d_r, nc = _hip.ntiles(B), layer.d_r, 3 * n
    cf = torch.randn(B, k, generator=torch.Generator().manual_seed(3)).to(dev) if with_coef else None
    r_t = torch.empty(T, d_r, _hip.TILE, device=dev)
    aux = torch.empty(T, _hip.AUX_ROWS, _hip.TILE, device=dev)
    G, g = torch.empty(B, k, d_r, device=dev), torch.empty(B, 1, d_r, device=dev)
    ws = torch.empty(max(lib.cvf_cv_nets_scratch_floats(mdesc, L, B, 1), lib.cvf_cv_nets_shared_scratch_floats(mdesc, ns, B, 1)), device=dev)
    keep = [layer, nets, theta, x, r_t, aux, G, g, ws, cf]
    fns, outs = {}, {}
    for route in ("frame", "frame_large", "three"):
        for form in ("A", "A2", "C"):
            xi, D = torch.empty(B, k, device=dev), torch.empty((B, nc) if with_coef else (B, k, nc), device=dev)
            cut = ns if form == "C" else L
            if route == "three":
                nets_eval, label = (lib.cvf_cv_nets_shared_eval, "cvf_cv_nets_shared_eval") if form == "C" else (lib.cvf_cv_nets_eval, "cvf_cv_nets_eval")

                def fn(xi=xi, D=D, cut=cut, nets_eval=nets_eval, label=label):
                    s = _hip.stream()
                    _hip.check(lib.cvf_align_feature_fwd(pdesc, P(x), B, P(r_t), None, P(aux), None, s), "cvf_align_feature_fwd")
                    _hip.check(nets_eval(mdesc, P(theta), cut, None, P(r_t), B, P(xi), P(G), None, P(ws), s), label)
                    if cf is None:
                        _hip.check(lib.cvf_align_feature_vjp_rows(pdesc, P(x), B, P(aux), k, P(G), P(D), s), "cvf_align_feature_vjp_rows")
                    else:
                        torch.bmm(cf.unsqueeze(1), G, out=g)
                        _hip.check(lib.cvf_align_feature_vjp(pdesc, P(x), B, P(aux), P(g), P(D), s), "cvf_align_feature_vjp")
            else:
                label = "cvf_cv_" + route + ("_shared" if form == "C" else "") + "_eval"
                entry = getattr(lib, label)

                def fn(xi=xi, D=D, cut=cut, entry=entry, label=label):
                    _hip.check(entry(mdesc, P(theta), cut, pdesc, P(x), B, P(cf), P(xi), P(D), _hip.stream()), label)
            fns[(route, form)], outs[(route, form)] = fn, (xi, D)
    return fns, outs, keep


def main_shared(a, dev):
    out = {"tool": "bench_cv_frame --shared", "replays": a.replays, "windows": a.windows, "rounds": a.rounds, "unit": "us per evaluation",
           "results": {}}
    lines = [f"{'model':7s} {'B':>5s} {'coef':>4s} {'route':12s} {'form A':>24s} {'form A again':>24s} {'form C':>24s}   C/A   A2/A   max rel diff C vs A"]
    for model in SHARED_MODELS:
        for B in [int(b) for b in a.batches.split(",")]:
            for with_coef in (False, True):
                fns, outs, keep = build_shared(model, B, dev, with_coef)
                for fn in fns.values():      # one eager call of every variant before any capture
                    fn()
                torch.cuda.synchronize()
                diffs = {r: float((outs[(r, "C")][1] - outs[(r, "A")][1]).abs().max() / outs[(r, "A")][1].abs().max()) for r in ("frame", "frame_large", "three")}
                replays, graphs = {}, []
                for key, fn in fns.items():
                    replays[key], g = captured(fn)
                    graphs.append(g)
                for fn in replays.values():
                    window_us(fn, 20)
                rounds = {v: [] for v in replays}
                for _ in range(a.rounds):
                    for v in replays:        # the variants alternate inside a round
                        rounds[v].append(statistics.median(window_us(replays[v], a.replays) for _ in range(a.windows)))
                res = {v: {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)} for v, t in rounds.items()}
                cell = lambda r: f"{r['median']:9.2f} [{r['min']:6.2f},{r['max']:6.2f}]"
                for route in ("frame", "frame_large", "three"):
                    A, A2, Cc = res[(route, "A")], res[(route, "A2")], res[(route, "C")]
                    out["results"][f"{model}/B{B}/{'coef' if with_coef else 'rows'}/{route}"] = {"A": A, "A2": A2, "C": Cc, "rel_diff": diffs[route]}
                    lines.append(f"{model:7s} {B:5d} {'yes' if with_coef else 'no':>4s} {route:12s} {cell(A):>24s} {cell(A2):>24s} {cell(Cc):>24s}"
                                 f"   {Cc['median'] / A['median']:.3f}  {A2['median'] / A['median']:.3f}   {diffs[route]:.1e}")
                del graphs, replays, fns, keep
    print("\n".join(lines), file=sys.stderr)
    if a.summary:
        with open(a.summary, "w") as f:
            f.write("bench_cv_frame --shared: us per evaluation of (xi, J) or (xi, F), graph replays, median of the rounds' medians [min, max over "
                    f"rounds]; {a.replays} replays per window, {a.windows} windows per round, {a.rounds} rounds, variants alternating\n")
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)), help="comma-separated batch sizes (larger ones locate the crossover)")
    ap.add_argument("--shapes", default=",".join(SHAPES), help="comma-separated shapes of SHAPES")
    ap.add_argument("--summary", default=None)
    ap.add_argument("--shared", action="store_true", help="form C against form A on config 3's layer (DESIGN.md 4.17)")
    a = ap.parse_args()
    assert a.replays >= 200 and a.rounds >= 3, "at least 200 replays per window and three rounds"
    assert torch.cuda.is_available(), "bench_cv_frame.py measures on the GPU"
    dev = torch.device("cuda:0")
    if a.shared:
        return main_shared(a, dev)
    out = {"tool": "bench_cv_frame", "replays": a.replays, "windows": a.windows, "rounds": a.rounds, "unit": "us per evaluation",
           "results": {}}
    lines = [f"{'shape':10s} {'B':>5s} " + " ".join(f"{v:>24s}" for v in VARIANTS) + "   frame_graph, frame_large_graph / three_graph"]
    for shape in [s for s in a.shapes.split(",") if s]:
        for B in [int(b) for b in a.batches.split(",")]:
            three, frame, large, J3, J1, J2, keep = build(shape, B, dev)
            three()
            diffs = []
            for fn, J in ((frame, J1), (large, J2)):   # one eager call of every route before any capture
                if fn is not None:
                    fn()
                    torch.cuda.synchronize()
                    diffs.append(float((J - J3).abs().max() / J3.abs().max()))
            diff = max(diffs)
            fns, graphs = {}, []
            for name, fn in (("three", three), ("frame", frame), ("frame_large", large)):
                if fn is not None:
                    replay, g = captured(fn)
                    graphs.append(g)
                    fns[name + "_eager"], fns[name + "_graph"] = fn, replay
            for fn in fns.values():          # warm every variant once more behind the captures
                window_us(fn, 20)
            rounds = {v: [] for v in fns}
            for _ in range(a.rounds):
                for v in fns:                # the variants alternate inside a round
                    rounds[v].append(statistics.median(window_us(fns[v], a.replays) for _ in range(a.windows)))
            res = {v: {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)} for v, t in rounds.items()}
            res["rel_diff_J"] = diff
            out["results"][f"{shape}/B{B}"] = res
            ratios = " ".join(f"{res[v]['median'] / res['three_graph']['median']:.3f}" if v in res else "    -" for v in ("frame_graph", "frame_large_graph"))
            lines.append(f"{shape:10s} {B:5d} " + " ".join(
                (f"{res[v]['median']:9.2f} [{res[v]['min']:6.2f},{res[v]['max']:6.2f}]" if v in res else f"{'-':>24s}") for v in VARIANTS)
                + f"   {ratios}   (J rel diff {diff:.1e})")
            del graphs, fns, keep
    print("\n".join(lines), file=sys.stderr)
    if a.summary:
        with open(a.summary, "w") as f:
            f.write("bench_cv_frame: us per evaluation of (xi, J), median of the rounds' medians [min, max over rounds]; "
                    f"{a.replays} replays per window, {a.windows} windows per round, {a.rounds} rounds, variants alternating\n")
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
