#!/usr/bin/env python3
"""Time one generator-mode regulariser step of the dipeptide chain on the shared-trunk launches of csrc/ef_general.hip (DESIGN.md
section 4.12): [66,128,128,2 | 2,128,128,66] with two regularisers [2,128,128,1] - the chains reg_i o encoder are two nets
[66,128,128,128,128,1] whose first two layers are the encoder's - at B = 20 000, in two forms:
    shared   the trunk stored and run once (cvf_ef_general_shared_*, n_shared = 2)
    copies   the same kernels on K explicit copies of the trunk (n_shared = 0)
The step is the C-ABI sequence of the inner task on feature rows: forward (y, g), cvf_metric_apply_stats on the identity layer
(q, batch sums, loss tail), backward, cvf_slab_reduce.  The two forms alternate `--repeats` times in one process; each repeat is
the median of `--steps` steps timed with HIP events.  Prints one JSON line: per form the repeats' medians, their median, the
spread (largest minus smallest repeat), the ef_general launches' share, and the workspace sizes.
    python tools/bench_ef_shared.py [--frames 20000] [--steps 30] [--repeats 3]

--mode transfer: the transfer-operator step of a SharedEigenFunctions model instead - trunk [66,128,128], heads [128,128,1], k = 3
(three nets [66,128,128,128,1] whose first two layers are the trunk) at B = 20 000 frames and as many lagged partners, in two forms:
    shared   cvf_ef_general_shared_transfer_fwd / _backward, n_shared = 2: the trunk forward once over the 2T tiles, the heads'
             adjoints summed at the trunk boundary, the trunk backward once
    copies   the plain general route (cvf_ef_general_fwd / _backward) on K explicit copies of the trunk
Its step: forward (y of both tile sets), cvf_ef_stats (time-lagged batch sums, loss tail), backward, cvf_slab_reduce.  Same
alternation, same JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd")):
    sys.path.insert(0, p)
from colvarsfinder import _hip, core  # noqa: E402
from colvarsfinder.pp import identity_desc  # noqa: E402

DIMS, K, NS = [66, 128, 128, 128, 128, 1], 2, 2


class Form:
    def __init__(self, ns, B, dev):
        lib = _hip.lib()
        L = len(DIMS) - 1
        self.ns, self.B = ns, B
        self.fl = fl = core._SharedTrunkFlat(DIMS, [1] * (L - 1) + [0], K, ns, dev)
        g = torch.Generator().manual_seed(3)
        fl.theta.copy_((torch.rand(fl.n, generator=g) * 2 - 1) * 0.09)
        self.T = T = _hip.ntiles(B)
        D = DIMS[0]
        f32, f64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.float64)
        self.rows = torch.randn(B, D, generator=g).to(dev)
        self.w, self.a = (torch.rand(B, generator=g) + 0.5).to(dev), torch.ones(D, **f32)
        self.pp = identity_desc(D)
        cfg = _hip.EFCfg()
        cfg.k, cfg.lag_idx, cfg.sort_eigvals, cfg.alpha, cfg.beta, cfg.dt = K, 0, 1, 1.0, 1.0, 1.0
        cfg.eig_w[0], cfg.eig_w[1] = 1.0, 0.7
        self.cfg = cfg
        self.n_saved = lib.cvf_ef_general_shared_saved_floats(fl.desc, T, ns)
        self.n_rows = lib.cvf_ef_general_shared_slab_rows(fl.desc, T, ns)
        assert self.n_saved > 0 and self.n_rows > 0, lib.cvf_last_error()
        self.feat = torch.empty(T * D * 64, **f32)
        self.y, self.g = torch.empty(T * K * 64, **f32), torch.empty(T * K * D * 64, **f32)
        self.q, self.e = torch.empty(T * K * D * 64, **f32), torch.empty(T * K * 64, **f32)
        self.saved, self.slab = torch.empty(self.n_saved, **f32), torch.empty(self.n_rows * fl.n, **f32)
        self.grad = torch.zeros(fl.n, **f32)
        self.scratch = torch.zeros(lib.cvf_metric_stats_scratch_doubles(B, K), **f64)
        self.stats, self.lv, self.coef = torch.zeros(lib.cvf_ef_nstats(K, 0), **f64), torch.zeros(3 + 2 * K, **f64), torch.zeros(4 * K + K * K, **f64)
        _hip.check(lib.cvf_align_feature_fwd(self.pp, _hip.ptr(self.rows), B, _hip.ptr(self.feat), None, None, None, _hip.stream()), "features")

    def step(self, ev=None):
        lib, P, s, fl = _hip.lib(), _hip.ptr, _hip.stream(), self.fl
        mark = (lambda: None) if ev is None else (lambda: ev.append(torch.cuda.Event(enable_timing=True)) or ev[-1].record())
        mark()
        _hip.check(lib.cvf_ef_general_shared_fwd(fl.desc, self.ns, P(fl.theta), P(self.feat), self.T, P(self.y), P(self.g), P(self.saved), s), "fwd")
        mark()
        _hip.check(lib.cvf_metric_apply_stats(self.pp, P(self.rows), self.B, None, P(self.a), K, P(self.g), P(self.q), P(self.e), None, None,
                                              self.cfg, P(self.w), P(self.y), P(self.scratch), P(self.stats), P(self.lv), P(self.coef), s), "metric")
        mark()
        _hip.check(lib.cvf_ef_general_shared_backward(self.cfg, fl.desc, self.ns, P(fl.theta), self.B, P(self.w), P(self.feat), P(self.y),
                                                      P(self.q), P(self.coef), P(self.slab), None, P(self.saved), s), "backward")
        mark()
        _hip.check(lib.cvf_slab_reduce(P(self.slab), self.n_rows, fl.n, P(self.grad), None, s), "reduce")
        mark()


class TransferForm:
    """ns = None: the plain entries on copies of the trunk; else the shared transfer entries with that n_shared."""
    DIMS, K, NS, LAG = [66, 128, 128, 128, 1], 3, 2, 2

    def __init__(self, ns, B, dev):
        lib, dims, k = _hip.lib(), self.DIMS, self.K
        L = len(dims) - 1
        self.ns, self.B = ns, B
        self.fl = fl = core._SharedTrunkFlat(dims, [1] * (L - 1) + [0], k, ns or 0, dev)
        g = torch.Generator().manual_seed(3)
        fl.theta.copy_((torch.rand(fl.n, generator=g) * 2 - 1) * 0.09)
        self.T = T = _hip.ntiles(B)
        self.nt, D = 2 * T, dims[0]
        f32, f64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.float64)
        rows = torch.randn(B + self.LAG, D, generator=g).to(dev)
        w = (torch.rand(B + self.LAG, generator=g) + 0.5).to(dev)
        self.w, self.w_lag = w[:B].contiguous(), w[self.LAG:].contiguous()
        pp = identity_desc(D)
        cfg = _hip.EFCfg()
        cfg.k, cfg.lag_idx, cfg.sort_eigvals, cfg.alpha, cfg.beta, cfg.dt = k, self.LAG, 1, 1.0, 1.0, 1.0
        for i in range(k):
            cfg.eig_w[i] = 1.0 - 0.15 * i
        self.cfg = cfg
        if ns is None:
            self.n_saved, self.n_rows = lib.cvf_ef_general_saved_floats(fl.desc, self.nt, self.LAG), lib.cvf_ef_general_slab_rows(fl.desc, self.nt)
        else:
            self.n_saved = lib.cvf_ef_general_shared_transfer_saved_floats(fl.desc, self.nt, ns)
            self.n_rows = lib.cvf_ef_general_shared_transfer_slab_rows(fl.desc, self.nt, ns)
        assert self.n_saved > 0 and self.n_rows > 0, lib.cvf_last_error()
        self.feat = torch.empty(self.nt * D * 64, **f32)
        self.y = torch.empty(self.nt * k * 64, **f32)
        self.saved, self.slab = torch.empty(self.n_saved, **f32), torch.empty(self.n_rows * fl.n, **f32)
        self.grad = torch.zeros(fl.n, **f32)
        self.scratch = torch.zeros(lib.cvf_ef_stats_scratch_doubles(k, self.LAG), **f64)
        self.stats, self.lv = torch.zeros(lib.cvf_ef_nstats(k, self.LAG), **f64), torch.zeros(3 + 2 * k, **f64)
        self.coef = torch.zeros(4 * k + k * k, **f64)
        for half, x in ((self.feat, rows[:B].contiguous()), (self.feat[T * D * 64:], rows[self.LAG:].contiguous())):
            _hip.check(lib.cvf_align_feature_fwd(pp, _hip.ptr(x), B, _hip.ptr(half), None, None, None, _hip.stream()), "features")

    def step(self, ev=None):
        lib, P, s, fl, k = _hip.lib(), _hip.ptr, _hip.stream(), self.fl, self.K
        mark = (lambda: None) if ev is None else (lambda: ev.append(torch.cuda.Event(enable_timing=True)) or ev[-1].record())
        mark()
        if self.ns is None:
            _hip.check(lib.cvf_ef_general_fwd(fl.desc, P(fl.theta), P(self.feat), self.nt, P(self.y), None, P(self.saved), s), "fwd")
        else:
            _hip.check(lib.cvf_ef_general_shared_transfer_fwd(fl.desc, self.ns, P(fl.theta), P(self.feat), self.nt, P(self.y), P(self.saved), s), "fwd")
        mark()
        _hip.check(lib.cvf_ef_stats(self.cfg, self.B, P(self.w), P(self.y), None, P(self.w_lag), P(self.y[self.T * k * 64:]), P(self.scratch),
                                    P(self.stats), P(self.lv), P(self.coef), s), "stats")
        mark()
        if self.ns is None:
            _hip.check(lib.cvf_ef_general_backward(self.cfg, fl.desc, P(fl.theta), self.B, P(self.w), P(self.w_lag), P(self.feat), P(self.y), None,
                                                   P(self.coef), P(self.slab), None, P(self.saved), s), "backward")
        else:
            _hip.check(lib.cvf_ef_general_shared_transfer_backward(self.cfg, fl.desc, self.ns, P(fl.theta), self.B, P(self.w), P(self.w_lag),
                                                                   P(self.feat), P(self.y), P(self.coef), P(self.slab), None, P(self.saved), s),
                       "backward")
        mark()
        _hip.check(lib.cvf_slab_reduce(P(self.slab), self.n_rows, fl.n, P(self.grad), None, s), "reduce")
        mark()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["generator", "transfer"], default="generator")
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.mode == "transfer":
        forms = {"shared": TransferForm(TransferForm.NS, a.frames, dev), "copies": TransferForm(None, a.frames, dev)}
        dims, k, ns = TransferForm.DIMS, TransferForm.K, TransferForm.NS
    else:
        forms = {"shared": Form(NS, a.frames, dev), "copies": Form(0, a.frames, dev)}
        dims, k, ns = DIMS, K, NS
    for f in forms.values():
        for _ in range(5):
            f.step()
    torch.cuda.synchronize()
    rep = {n: dict(total=[], fwd=[], backward=[]) for n in forms}
    for _ in range(a.repeats):
        for n, f in forms.items():
            evs = []
            for _ in range(a.steps):
                ev = []
                f.step(ev)
                evs.append(ev)
            torch.cuda.synchronize()
            us = lambda i, j: statistics.median(e[i].elapsed_time(e[j]) * 1e3 for e in evs)   # noqa: E731
            rep[n]["total"].append(us(0, 4))
            rep[n]["fwd"].append(us(0, 1))
            rep[n]["backward"].append(us(2, 3))
    out = dict(mode=a.mode, dims=dims, k=k, n_shared=ns, frames=a.frames, steps=a.steps)
    for n, f in forms.items():
        t = rep[n]["total"]
        out[n] = dict(step_us=[round(v, 1) for v in t], median_us=round(statistics.median(t), 1), spread_us=round(max(t) - min(t), 1),
                      fwd_us=round(statistics.median(rep[n]["fwd"]), 1), backward_us=round(statistics.median(rep[n]["backward"]), 1),
                      saved_bytes=4 * f.n_saved, slab_bytes=4 * f.n_rows * f.fl.n, slab_rows=int(f.n_rows), n_params=int(f.fl.n))
    out["shared_faster_by_us"] = round(out["copies"]["median_us"] - out["shared"]["median_us"], 1)
    out["faster_than_spread"] = out["shared_faster_by_us"] > out["copies"]["spread_us"]
    out["not_slower_by_more_than_spread"] = out["shared_faster_by_us"] >= -out["copies"]["spread_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
