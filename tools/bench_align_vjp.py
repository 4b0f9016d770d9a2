#!/usr/bin/env python3
"""The alignment + feature layer differentiated in the coordinates: HIP-event times of the VJP launch alone
(cvf_align_feature_vjp) and of one layer forward + backward through autograd (AlignFeatureLayer -> _AlignFeatureFn), against
the same gradient through the pure-torch twin (export.ScriptableAlignFeature + autograd) on the GPU, at the config-3 shape
(22 atoms, positions, 20 000 frames) and the config-5 shape (bench.c5_features(5000), 2 000 and 16 000 frames).

The bytes the VJP must move per frame are computed from the shapes: it writes the dense row of 3N floats (12 N bytes) and reads
x only where a feature looks (12 n_slot), the upstream row (4 d_r) and the aux rows (72); small frames read the whole x row
(12 N) instead of 12 n_slot.  Fraction of 6.3 TB/s (MI355X_MICROARCH: measured float4 copy).   python tools/bench_align_vjp.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import bench  # noqa: E402
from colvarsfinder import _hip, pp  # noqa: E402
from colvarsfinder.export import ScriptableAlignFeature  # noqa: E402

HBM_BPS = 6.3e12
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


def shape(label, n_atoms, feats, B, twin_reps):
    ref = np.random.RandomState(bench.SEED).normal(scale=2.0, size=(n_atoms, 3))
    layer = pp.AlignFeatureLayer(n_atoms, list(range(n_atoms)), ref, feats).to(dev)
    x, _ = bench.device_frames(B, ref, 0.3, bench.SEED + 11, dev, chunk=4000)
    g = torch.randn(B, layer.d_r, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    desc = layer.pp_desc()
    aux = torch.empty(_hip.ntiles(B), _hip.AUX_ROWS, _hip.TILE, device=dev)
    feat = torch.empty(B, layer.d_r, device=dev)
    scratch = _hip.align_scratch(desc, B, dev)
    s = _hip.stream()
    _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, None, P(feat), P(aux), P(scratch), s), "cvf_align_feature_fwd")
    gx = torch.empty(B, 3 * n_atoms, device=dev)

    def vjp():
        _hip.check(lib.cvf_align_feature_vjp(desc, P(x), B, P(aux), P(g), P(gx), s), "cvf_align_feature_vjp")

    t_vjp = timed(vjp, 20)
    xr = x.clone().requires_grad_(True)

    def fwd_bwd():
        return torch.autograd.grad(layer(xr), xr, g)[0]

    t_fb = timed(fwd_bwd, 10)
    (ours,) = torch.autograd.grad(layer(xr), xr, g)
    twin = ScriptableAlignFeature(layer).to(dev)

    def twin_fb():
        return torch.autograd.grad(twin(xr), xr, g)[0]

    t_twin = timed(twin_fb, twin_reps, warmup=1)
    diff = float((twin_fb() - ours).abs().max() / ours.abs().max())
    large = 3 * n_atoms > 192
    read = (12 * layer._n_slot if large else 12 * n_atoms) + 4 * layer.d_r + 4 * _hip.AUX_ROWS
    vjp_bytes = B * (12 * n_atoms + read)
    return dict(shape=label, n_atoms=n_atoms, d_r=layer.d_r, frames=B, kernel="vjp_large_kernel" if large else "vjp_align_kernel",
                vjp_us=round(t_vjp, 1), vjp_bytes=vjp_bytes, vjp_frac_of_6p3TBps=round(vjp_bytes / (t_vjp * 1e-6) / HBM_BPS, 3),
                fwd_bwd_us=round(t_fb, 1), twin_fwd_bwd_us=round(t_twin, 1), twin_over_ours=round(t_twin / t_fb, 1),
                max_rel_diff_vs_twin=float(f"{diff:.2e}"))


na5 = bench.C5["n_atoms"]
rows = [shape("config-3", 22, [("position", tuple(range(22)))], 20000, 10),
        shape("config-5", na5, bench.c5_features(na5), 2000, 5),
        shape("config-5", na5, bench.c5_features(na5), 16000, 3)]
print(json.dumps(dict(tool="bench_align_vjp", measured=rows)))
