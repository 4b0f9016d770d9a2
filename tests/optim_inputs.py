"""CPU references shared by the optimiser tests.

Adam: torch.optim.Adam from a given state, and the conditioned metrics of tests/test_optimizer_gpu.py.

The full-pack cases of tests/optim_cases.py (FWD_CASES): k tanh nets D -> H x NH -> 1 with torch.nn.Linear's initialisation, 70
frames of N(0, 1) features; y and g = dy/dfeat in fp64 through oracle/nnref.py, and in fp32 with every rounding pinned (sums
over a layer's inputs term by term in fp32, tanh rounded from fp64) so that the figure the bars derive from does not depend
on the CPU or the BLAS that evaluates it."""
import zlib

import numpy as np
import torch

from oracle import nnref
from tests import optim_cases as OC


def fwd_inputs(case):
    """(feat [B, D] fp32, state dict fp32, dims)."""
    H, NH, D, k = case
    seed = zlib.crc32(repr(tuple(case)).encode()) % 100_000
    dims = [D] + [H] * NH + [1]
    gen = torch.Generator().manual_seed(seed)
    sd = nnref.init_eigenfunctions(dims, k, gen)
    feat = torch.randn(OC.FWD_B, D, generator=gen)
    return feat, sd, dims


def fwd_oracle64(case, inp=None):
    """(y [B, k], g [B, k, D]) in fp64: oracle/nnref.py's nets and autograd."""
    feat, sd, _ = fwd_inputs(case) if inp is None else inp
    k = case[3]
    sd64 = {n: p.double() for n, p in sd.items()}
    x = feat.double().requires_grad_(True)
    y = nnref.eigenfunctions_forward(sd64, k, x)
    g = torch.stack([torch.autograd.grad(y[:, i].sum(), x, retain_graph=True)[0] for i in range(k)], 1)
    return y.detach().numpy(), g.numpy()


def fwd_pinned32(case, inp=None):
    """The same in fp32 with fixed roundings (elementwise numpy only)."""
    feat, sd, dims = fwd_inputs(case) if inp is None else inp
    k, L = case[3], len(dims) - 1
    x = feat.numpy()
    ys, gs = [], []
    for i in range(k):
        W = [sd[f"eigen_funcs.{i}.{l + 1}.weight"].numpy() for l in range(L)]
        b = [sd[f"eigen_funcs.{i}.{l + 1}.bias"].numpy() for l in range(L)]
        h, hs = x, []
        for l in range(L):
            z = np.broadcast_to(b[l], (x.shape[0], dims[l + 1])).astype(np.float32)
            for j in range(dims[l]):
                z = z + h[:, j:j + 1] * W[l][:, j]
            h = np.tanh(z.astype(np.float64)).astype(np.float32) if l < L - 1 else z
            hs.append(h)
        ys.append(h[:, 0])
        s = np.ones((x.shape[0], 1), np.float32)            # dy / d(layer output), from the output layer back
        for l in range(L - 1, -1, -1):
            if l < L - 1:
                s = s * (np.float32(1.0) - hs[l] * hs[l])
            nxt = np.zeros((x.shape[0], dims[l]), np.float32)
            for o in range(dims[l + 1]):
                nxt = nxt + s[:, o:o + 1] * W[l][o]
            s = nxt
        gs.append(s)
    return np.stack(ys, 1).astype(np.float64), np.stack(gs, 1).astype(np.float64)


def fwd_errors(y, g, y64, g64):
    """(largest error of y over its largest entry, the same for g)."""
    return float(np.abs(y - y64).max() / np.abs(y64).max()), float(np.abs(g - g64).max() / np.abs(g64).max())


def fwd_worst_e32():
    worst = [0.0, 0.0]
    for c in OC.FWD_CASES:
        inp = fwd_inputs(c)
        e = fwd_errors(*fwd_pinned32(c, inp), *fwd_oracle64(c, inp))
        worst = [max(a, b_) for a, b_ in zip(worst, e)]
    return worst


# ---------------------------------------------------------------------------------------------------- Adam
def torch_adam(th0, g, m0, v0, t, lr, betas, eps, dtype):
    """torch.optim.Adam on the CPU (what the reference builds: torch.optim.Adam(params, lr=...)) with its state set to step t - 1."""
    p = th0.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0.to(dtype).clone(), "exp_avg_sq": v0.to(dtype).clone()}
    p.grad = g.to(dtype).clone()
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == t
    return [x.detach().double().numpy() for x in (p, st["exp_avg"], st["exp_avg_sq"])]


def adam_metrics(got, ref64, th0, g, m0, t, lr, betas, eps):
    """The metrics of the module docstring as {name: value}: m, v, th, and th over each block of theta0 alone (th_0, th_1e-4,
    th_1; th is their maximum).  Entries whose denominator is 0 must match exactly."""
    th, m, v = (np.asarray(x, dtype=np.float64) for x in got)
    th64, m64, v64 = ref64
    th0, g, m0 = (x.double().numpy() for x in (th0, g, m0))
    a = np.abs(m0) + np.abs(g)
    s_t = lr / (1.0 - betas[0] ** t)
    den64 = np.sqrt(v64) / np.sqrt(1.0 - betas[1] ** t) + eps
    den_th = s_t * a / den64 + 2.0 ** -24 * np.abs(th0)
    out = {}

    def worst(name, diff, den, sel=None):
        live = den > 0
        assert (diff[~live] == 0).all(), name
        if sel is not None:
            live = live & sel
        out[name] = float((diff[live] / den[live]).max()) if live.any() else 0.0

    worst("m", np.abs(m - m64), a)
    worst("v", np.abs(v - v64), v64)
    worst("th", np.abs(th - th64), den_th)
    # th0 = 0: the relative error of the update itself; in the other blocks the rounding of th0 - update, half an ulp of
    # th0, is of the size of the denominator's second term, so each block is held to its own fp32 figure
    scale = np.abs(th0)
    worst("th_0", np.abs(th - th64), den_th, scale == 0)
    worst("th_1e-4", np.abs(th - th64), den_th, (scale > 0) & (scale < 2e-3))
    worst("th_1", np.abs(th - th64), den_th, scale >= 2e-3)
    return out
