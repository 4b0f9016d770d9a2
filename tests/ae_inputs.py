"""Inputs and CPU oracles of the autoencoder step sweep (tests/ae_cases.py), shared by the CPU test that ties the error bars
to the fp32 oracle (tests/test_ae_instances.py) and by the GPU sweep (tests/test_ae_sweep_gpu.py).  Needs torch, no GPU."""
import zlib

import numpy as np
import torch

from oracle import losses, nnref
from tests import ae_cases as A
from tests.synth import make_molecule_traj

ACT_FN = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu, "elu": torch.nn.functional.elu,
          "leaky_relu": torch.nn.functional.leaky_relu, "softplus": torch.nn.functional.softplus}
EXTRA_ROWS = 37   # feature rows beyond the batch that an `idx` case gathers from


def inputs(case):
    """(feature rows [n, d0] fp32, idx [B] int64 or None, batch weights [B] fp32, initial state dict fp32): a synthetic
    trajectory's leading d0 coordinates, a permutation's head as the index vector, torch.nn.Linear's initialisation."""
    seed = zlib.crc32(case.id.encode()) % 100_000   # (stable when cases are added)
    d0, B = case.e_dims[0], case.B
    n = B + (EXTRA_ROWS if case.idx else 0)
    traj, w, _ = make_molecule_traj((d0 + 2) // 3, n, seed=seed, scale=1.0, sigma=0.3)
    rows = np.ascontiguousarray(traj.reshape(n, -1)[:, :d0])
    idx = np.random.RandomState(seed).permutation(n)[:B].astype(np.int64) if case.idx else None
    wb = (w if idx is None else w[idx]).astype(np.float32)
    sd0 = nnref.init_autoencoder(list(case.e_dims), list(case.d_dims), torch.Generator().manual_seed(seed), torch.float32)
    return rows, idx, wb, sd0


def mlp_desc(case):
    """cvf_mlp_desc of the chain over a flat buffer in parameters() order (colvarsfinder.nn.mlp_layout for an AutoEncoder)."""
    from colvarsfinder import _hip
    d, dm, ac, pos = _hip.MLPDesc(), A.dims(case), A.acts(case), 0
    d.n_nets, d.n_layers = 1, len(dm) - 1
    for l in range(len(dm) - 1):
        d.dims[l], d.dims[l + 1], d.act[l] = dm[l], dm[l + 1], ac[l]
        d.w_off[0][l], pos = pos, pos + dm[l] * dm[l + 1]
        d.b_off[0][l], pos = pos, pos + dm[l + 1]
    d.n_params = pos
    return d


def oracle(case, inp, dtype, adam_steps=0, lr=1e-3):
    """oracle.losses.ae_loss on the gathered frames in `dtype`, with autograd: (loss, flat gradient in parameters() order) as
    float64 numpy; with adam_steps > 0 also the flat parameters after that many torch.optim.Adam steps on the same batch."""
    rows, idx, wb, sd0 = inp
    F = torch.as_tensor(rows if idx is None else rows[idx]).to(dtype)
    w = torch.as_tensor(wb).to(dtype)
    sd = {k: p.to(dtype).clone().requires_grad_(True) for k, p in sd0.items()}
    loss = losses.ae_loss(sd, F, w, activation=ACT_FN[case.act])
    loss.backward()
    out = [float(loss.detach()), torch.cat([p.grad.reshape(-1) for p in sd.values()]).double().numpy()]
    if adam_steps:
        opt = torch.optim.Adam(list(sd.values()), lr=lr)
        for step in range(adam_steps):
            if step:
                opt.zero_grad()
                losses.ae_loss(sd, F, w, activation=ACT_FN[case.act]).backward()
            opt.step()
        out.append(torch.cat([p.detach().reshape(-1) for p in sd.values()]).double().numpy())
    return out


def errors(loss, grad, loss64, grad64):
    """(relative loss error, largest gradient entry error over the largest gradient entry) against the fp64 oracle."""
    return abs(loss - loss64) / abs(loss64), float(np.abs(grad - grad64).max() / np.abs(grad64).max())


def oracle_fp32(case, inp):
    """The same loss and gradient in fp32 (plain torch on the CPU): ae_loss's weighted sum of squared errors and its autograd
    gradient on one 64-frame tile at a time, the tiles' sums added in fp64.  A single fp32 evaluation of the whole batch leaves
    the order of its sums over the frames - and an error that grows with the batch, up to 8e-6 of the largest gradient entry at
    140 000 frames - to the BLAS build and the core count of the machine; tile by tile the figure is the error of the fp32 chain
    itself, reproducible, and never larger than the whole-batch one, so a bar derived from it can only be tighter."""
    rows, idx, wb, sd0 = inp
    F = torch.as_tensor(rows if idx is None else rows[idx])
    w = torch.as_tensor(wb)
    sd = {k: p.clone().requires_grad_(True) for k, p in sd0.items()}
    params = list(sd.values())
    num, g = 0.0, torch.zeros(sum(p.numel() for p in params), dtype=torch.float64)
    for s0 in range(0, F.shape[0], A.TILE):
        Fc, wc = F[s0:s0 + A.TILE], w[s0:s0 + A.TILE]
        out = nnref.autoencoder_forward(sd, Fc, ACT_FN[case.act])
        part = (wc * torch.sum((out - Fc) ** 2, dim=1)).sum()              # losses.ae_loss's numerator
        grads = torch.autograd.grad(part, params)
        num += float(part.detach())
        g += torch.cat([q.reshape(-1) for q in grads]).double()
    wsum = float(w.double().sum())
    return num / wsum, (g / wsum).numpy()


def e32(case, inp=None, ref=None):
    """The fp32 oracle's own distance from the fp64 oracle: what the bars are derived from."""
    inp = inputs(case) if inp is None else inp
    ref = oracle(case, inp, torch.float64) if ref is None else ref
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        l32, g32 = oracle_fp32(case, inp)
    finally:
        torch.set_num_threads(n)
    return errors(l32, g32, ref[0], ref[1])


def group_e32(cases=None):
    """{group: [worst loss e32, worst gradient e32]} over the cases with a value comparison; a loss-only case is held to the
    loss bar alone, so its gradient does not enter."""
    worst = {}
    for c in A.CASES if cases is None else cases:
        if A.route(c) == "refused":
            continue
        e = e32(c)
        w = worst.setdefault(A.group(c), [0.0, 0.0])
        w[0] = max(w[0], e[0])
        if c.grad:
            w[1] = max(w[1], e[1])
    return worst


# ---------------------------------------------------------------------------------------------------- RegAutoEncoderTask
REGAE_HYPER = dict(alpha=0.8, gamma=[1.0, 4.0], eta=[0.0, 0.3, 0.5], dt=0.5)


def regae_inputs(c):
    """(trajectory [n, d] fp32, weights [n] fp64, idx [B] int64, eig_w, initial state dict fp32)."""
    seed = zlib.crc32(c.id.encode()) % 100_000
    rs = np.random.RandomState(seed)
    lag = max(c.lag_ae, c.lag_reg)
    n = c.B + lag + (EXTRA_ROWS if c.idx else 0)
    traj = rs.normal(size=(n, c.d))
    for t in range(1, n):          # AR(1), correlation 0.7 per row: lagged differences of the size of the signal itself, so that
        traj[t] = 0.7 * traj[t - 1] + 0.714 * traj[t]   # the transfer-operator sums (y_lag - y)^2 do not cancel their leading digits
    traj = (traj - traj.mean(0)).astype(np.float32)
    w = rs.uniform(0.5, 1.5, size=n)
    w /= w.mean()
    idx = (np.sort(rs.permutation(n - lag)[:c.B]) if c.idx else np.arange(c.B)).astype(np.int64)
    e, d, r, _ = A.regae_dims(c)
    sd0 = nnref.init_regautoencoder(e, d, r, c.K, torch.Generator().manual_seed(seed), torch.float32)
    return traj, w, idx, [1.0 - 0.1 * i for i in range(c.K)], sd0


def _rounded_tanh(x):
    """tanh evaluated in fp64 and rounded to x's precision (torch.tanh itself for fp64): the fp32 vector tanh of torch differs
    in its last digit between instruction sets."""
    return torch.tanh(x.double()).to(x.dtype)


def regae_oracle(c, inp, dtype):
    """The first step's loss row [loss, ae, npl, pen, eig_1..K, 0, norm, orth] and flat gradient (state-dict order), float64."""
    traj, w, idx, eig_w, sd0 = inp
    h = REGAE_HYPER
    # the chain in `dtype`, the batch statistics in fp64 whatever `dtype` is (fp64 weights promote every weighted sum): the split
    # the kernels make (fp32 chain, fp64 sums).  Variances and lagged differences formed in fp32 cancel their leading digits
    # by amounts that differ from one CPU to the next, which is no measure of an fp32 chain.
    F, W = torch.as_tensor(traj).to(dtype), torch.as_tensor(w.astype(np.float32)).double()
    sd = {k: p.to(dtype).clone().requires_grad_(True) for k, p in sd0.items()}
    act = _rounded_tanh
    ae = losses.regae_mse(sd, F[idx], F[idx + c.lag_ae], W[idx], activation=act)
    eig, npl, pen, cvec = losses.regae_eigen_loss(sd, c.K, F[idx], W[idx], F[idx + c.lag_reg], W[idx + c.lag_reg], eig_w=eig_w,
                                                  lag_idx=c.lag_reg, dt=h["dt"], activation=act)
    en, eo = losses.regae_enc_norm(sd, F[idx], W[idx], activation=act), losses.regae_enc_orth(sd, F[idx], W[idx], activation=act)
    lo = h["alpha"] * ae + h["gamma"][0] * npl + h["gamma"][1] * pen + h["eta"][1] * en + h["eta"][2] * eo
    lo.backward()
    row = np.asarray([float(v.detach()) for v in (lo, ae, npl, pen)] + [float(v) for v in eig] + [0.0, float(en.detach()), float(eo.detach())])
    return row, torch.cat([p.grad.reshape(-1) for p in sd.values()]).double().numpy(), list(cvec)


def regae_errors(c, row, grad, ref_row, ref_grad):
    """{term of A.REGAE_TERMS: error}: relative (eig: the worst eigenvalue), the gradient's of its largest entry."""
    K = c.K
    rel = lambda i: abs(row[i] - ref_row[i]) / max(abs(ref_row[i]), 1e-300)
    out = dict(loss=rel(0), ae=rel(1), npl=rel(2), pen=rel(3), eig=max(rel(4 + i) for i in range(K)), norm=rel(5 + K), orth=rel(6 + K))
    if grad is not None:
        out["grad"] = float(np.abs(grad - ref_grad).max() / np.abs(ref_grad).max())
    return out


class _FixedOrderLinear(torch.autograd.Function):
    """torch.nn.functional.linear whose every rounding is fixed: the sums over a layer's inputs (forward) and outputs (backward)
    run term by term in `x`'s precision with elementwise operations only, the sums over the frames (weight and bias gradients)
    in fp64.  A BLAS call leaves the order of these sums, and with it the last digits, to the CPU it runs on."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        out = bias.expand(x.shape[0], -1).clone()
        for j in range(weight.shape[1]):
            out = out + x[:, j:j + 1] * weight[:, j]
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        gx = torch.zeros_like(x)
        for o in range(weight.shape[0]):
            gx = gx + g[:, o:o + 1] * weight[o]
        return gx, (g.double().T @ x.double()).to(x.dtype), g.double().sum(0).to(x.dtype)


def regae_e32(c, inp=None, ref=None):
    """{term: distance of the fp32 oracle from the fp64 oracle}: the same oracle functions on fp32 tensors, with the Linear
    layers' sums in a fixed order (_FixedOrderLinear) so that the figure does not depend on the CPU that evaluates it."""
    inp = regae_inputs(c) if inp is None else inp
    ref = regae_oracle(c, inp, torch.float64) if ref is None else ref
    n, linear = torch.get_num_threads(), torch.nn.functional.linear
    torch.set_num_threads(1)
    torch.nn.functional.linear = _FixedOrderLinear.apply
    try:
        row, grad, _ = regae_oracle(c, inp, torch.float32)
    finally:
        torch.nn.functional.linear = linear
        torch.set_num_threads(n)
    return regae_errors(c, row, grad, ref[0], ref[1])


def regae_group_e32():
    """{term: worst e32 over REGAE_CASES}."""
    worst = dict.fromkeys(A.REGAE_TERMS, 0.0)
    for c in A.REGAE_CASES:
        for term, e in regae_e32(c).items():
            worst[term] = max(worst[term], e)
    return worst
