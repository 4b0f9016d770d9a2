#!/usr/bin/env python3
"""Per-frame CV Jacobians and CV metric tensors of a CV model (_CVModel.jacobian / metric_tensor): HIP-event
times (median after warm-up) of

  metric_tensor      M = J A J^T per frame [B, k, k]   (nets' d xi / d r by cvf_cv_nets_eval, cvf_metric_apply, cvf_metric_gram)
  jacobian           J per frame [B, k, 3N]           (nets' d xi / d r by cvf_cv_nets_eval, cvf_align_feature_vjp_rows)
  nets_torch_func    the nets' part alone, xi and d xi / d r from the feature rows by torch.func.vmap(jacrev(nets)) - the route
                     both calls took before and models outside cvf_cv_nets_supported still take
  nets_hip           the same from the feature tiles by cvf_cv_nets_eval (g_rows); the two alternate in one process over three
                     rounds: the median of each round, their median and their spread (min, max) are reported
  torch_route        what users had before: colvar_model() on a grad-requiring input (the torch twin), one autograd.grad per
                     CV, M by einsum - the comparison for both
  vjp_rows           one cvf_align_feature_vjp_rows launch for k cotangents
  vjp_single_x_k     k cvf_align_feature_vjp launches on the same cotangents

at config 3 (22 atoms, positions, d_r 66, k 3, nets [66,20,20,20,1], 20 000 frames), config 5 (bench.c5_features(5000),
d_r 384, k 6, 2 000 frames) and one encoder (config 3's layer, chain [66,128,128,2], 20 000 frames).  Inputs live on the device.
One JSON line.   python tools/bench_cv_jacobian.py [--shape c3|c5|enc]"""
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

dev = torch.device("cuda:0")
lib, P = _hip.lib(), _hip.ptr


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
    return t[len(t) // 2]   # median, us


def nets_part(cv, layer, model, x, B, k, rounds=3, reps=10):
    """The nets' part both ways on the same features, alternating: {route: [median of each round, us]}."""
    desc, T, s = layer.pp_desc(), _hip.ntiles(B), _hip.stream()
    rows, tiles = torch.empty(B, layer.d_r, device=dev), torch.empty(T, layer.d_r, _hip.TILE, device=dev)
    _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, P(tiles), P(rows), None, P(_hip.align_scratch(desc, B, dev)), s), "fwd")
    mdesc, upto, _, params = cv._nets_plan(model)
    theta = torch.cat([p_.detach().reshape(-1) for p_ in params])
    xi, G = torch.empty(B, k, device=dev), torch.empty(B, k, layer.d_r, device=dev)
    ws = torch.empty(lib.cvf_cv_nets_scratch_floats(mdesc, upto, B, 1), device=dev)

    def f(v):
        y = model(v.unsqueeze(0)).reshape(-1)
        return y, y

    def by_torch_func():
        Gt, xt = torch.func.vmap(torch.func.jacrev(f, has_aux=True))(rows)
        return xt, Gt.detach().contiguous()

    def by_hip():
        _hip.check(lib.cvf_cv_nets_eval(mdesc, P(theta), upto, None, P(tiles), B, P(xi), P(G), None, P(ws), s), "cvf_cv_nets_eval")

    out = dict(nets_torch_func=[], nets_hip=[])
    for _ in range(rounds):
        out["nets_torch_func"].append(timed(by_torch_func, reps))
        out["nets_hip"].append(timed(by_hip, reps))
    xt, Gt = by_torch_func()
    by_hip()
    torch.cuda.synchronize()
    out["max_rel_diff_g"] = float((G - Gt).abs().max() / Gt.abs().max())
    return out


def shape(label, n_atoms, feats, dims, k, B, torch_reps, encoder=False):
    ref = np.random.RandomState(bench.SEED).normal(scale=2.0, size=(n_atoms, 3))
    layer = pp.AlignFeatureLayer(n_atoms, list(range(n_atoms)), ref, feats).to(dev)
    torch.manual_seed(bench.SEED)
    model = (nn.create_sequential_nn([layer.d_r] + dims[1:]) if encoder else nn.EigenFunctions([layer.d_r] + dims[1:], k)).to(dev)
    cv = core._CVModel(layer, model, device=dev)
    assert cv.nets_route() == ("hip", None), cv.nets_route()
    x, _ = bench.device_frames(B, ref, 0.3, bench.SEED + 11, dev, chunk=4000)
    a = torch.rand(3 * n_atoms, generator=torch.Generator().manual_seed(3), dtype=torch.float64) + 0.1
    t_m = timed(lambda: cv.metric_tensor(x, diag_coeff=a), 10)
    t_j = timed(lambda: cv.jacobian(x), 10)
    a_dev = a.to(device=dev, dtype=torch.float32)

    def torch_route():
        xr = x.clone().requires_grad_(True)
        y = cv(xr)
        J = torch.stack([torch.autograd.grad(y[:, i].sum(), xr, retain_graph=i + 1 < k)[0].reshape(B, -1) for i in range(k)], 1)
        return y.detach(), J, torch.einsum("bin,n,bjn->bij", J, a_dev, J)

    t_torch = timed(torch_route, torch_reps, warmup=1)
    _, Jt, Mt = torch_route()
    _, M = cv.metric_tensor(x, diag_coeff=a)
    _, J = cv.jacobian(x)
    dm = float((M - Mt).abs().max() / Mt.abs().max())
    dj = float((J.reshape(B, k, -1) - Jt).abs().max() / Jt.abs().max())
    del Jt, J
    # the VJP entry alone: one launch for k rows against k single-cotangent launches
    desc = layer.pp_desc()
    aux = torch.empty(_hip.ntiles(B), _hip.AUX_ROWS, _hip.TILE, device=dev)
    feat = torch.empty(B, layer.d_r, device=dev)
    s = _hip.stream()
    _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, None, P(feat), P(aux), P(_hip.align_scratch(desc, B, dev)), s), "fwd")
    G = torch.randn(B, k, layer.d_r, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    Gs = [G[:, i].contiguous() for i in range(k)]
    rows = torch.empty(B, k, 3 * n_atoms, device=dev)
    gx = [torch.empty(B, 3 * n_atoms, device=dev) for _ in range(k)]

    def vjp_rows():
        _hip.check(lib.cvf_align_feature_vjp_rows(desc, P(x), B, P(aux), k, P(G), P(rows), s), "cvf_align_feature_vjp_rows")

    def vjp_single():
        for i in range(k):
            _hip.check(lib.cvf_align_feature_vjp(desc, P(x), B, P(aux), P(Gs[i]), P(gx[i]), s), "cvf_align_feature_vjp")

    t_rows, t_single = timed(vjp_rows, 20), timed(vjp_single, 20)
    del G, Gs, rows, gx
    part = nets_part(cv, layer, model, x, B, k)
    med = lambda v: sorted(v)[len(v) // 2]
    nets = {}
    for route in ("nets_torch_func", "nets_hip"):
        nets[route + "_us"] = round(med(part[route]), 1)
        nets[route + "_rounds_us"] = [round(v, 1) for v in part[route]]
    nets["torch_func_over_hip"] = round(med(part["nets_torch_func"]) / med(part["nets_hip"]), 1)
    nets["max_rel_diff_g_vs_torch_func"] = float(f"{part['max_rel_diff_g']:.2e}")
    return dict(shape=label, n_atoms=n_atoms, d_r=layer.d_r, k=k, frames=B, nets=list(dims), **nets,
                metric_tensor_us=round(t_m, 1), jacobian_us=round(t_j, 1), torch_route_us=round(t_torch, 1),
                torch_over_metric_tensor=round(t_torch / t_m, 1), torch_over_jacobian=round(t_torch / t_j, 1),
                vjp_rows_us=round(t_rows, 1), vjp_single_x_k_us=round(t_single, 1),
                rows_over_single_x_k=round(t_rows / t_single, 3),
                max_rel_diff_m_vs_torch=float(f"{dm:.2e}"), max_rel_diff_j_vs_torch=float(f"{dj:.2e}"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["c3", "c5", "enc", "all"], default="all")
    args = ap.parse_args()
    out = []
    if args.shape in ("c3", "all"):
        out.append(shape("config-3", 22, [("position", tuple(range(22)))], [66, 20, 20, 20, 1], 3, 20000, 5))
    if args.shape in ("c5", "all"):
        na5 = bench.C5["n_atoms"]
        out.append(shape("config-5", na5, bench.c5_features(na5), [384, 20, 20, 20, 1], 6, 2000, 3))
    if args.shape in ("enc", "all"):
        out.append(shape("encoder", 22, [("position", tuple(range(22)))], [66, 128, 128, 2], 2, 20000, 5, encoder=True))
    print(json.dumps(dict(tool="bench_cv_jacobian", measured=out)))
