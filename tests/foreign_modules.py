"""Preprocessing modules written in plain torch - what users hand the tasks as ``pp_layer`` instead of a molann layer - for the
tests of the foreign-module path (colvarsfinder.pp.FactoredMetric, CVF_PP_FACTORED)."""

import itertools

import torch


class PairDistances(torch.nn.Module):
    """All N (N - 1) / 2 pairwise distances of the atoms of ``[B, N, 3]`` frames."""

    def __init__(self, n_atoms):
        super().__init__()
        pairs = torch.tensor(list(itertools.combinations(range(n_atoms), 2)), dtype=torch.long)
        self.register_buffer("i", pairs[:, 0].contiguous())
        self.register_buffer("j", pairs[:, 1].contiguous())

    def forward(self, x):
        d = x[:, self.i, :] - x[:, self.j, :]
        return torch.sqrt((d * d).sum(dim=-1))


class SmoothContacts(torch.nn.Module):
    """Sigmoid contact values ``1 / (1 + exp((d_ij - r0) / s))`` of a few atom pairs: fewer features than coordinates."""

    def __init__(self, pairs, r0=3.0, s=0.5):
        super().__init__()
        p = torch.tensor(pairs, dtype=torch.long)
        self.register_buffer("i", p[:, 0].contiguous())
        self.register_buffer("j", p[:, 1].contiguous())
        self.r0, self.s = float(r0), float(s)

    def forward(self, x):
        d = x[:, self.i, :] - x[:, self.j, :]
        r = torch.sqrt((d * d).sum(dim=-1))
        return torch.sigmoid((self.r0 - r) / self.s)


class Polar(torch.nn.Module):
    """``[B, 2]`` points -> ``(r, cos theta, sin theta)``."""

    def forward(self, x):
        r = torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])
        return torch.stack([r, x[:, 0] / r, x[:, 1] / r], dim=1)


class Radius(torch.nn.Module):
    """``[B, 2]`` points -> ``[B, 1]`` distance from a centre (one feature, two coordinates)."""

    def forward(self, x):
        d = x - torch.tensor([0.3, -0.2], dtype=x.dtype, device=x.device)
        return torch.sqrt((d * d).sum(dim=1, keepdim=True))


class BatchCentred(torch.nn.Module):
    """Coordinates minus the batch mean: NOT frame-local (every frame's features depend on all frames)."""

    def forward(self, x):
        y = x.reshape(x.shape[0], -1)
        return y - y.mean(dim=0, keepdim=True)


class Flat3D(torch.nn.Module):
    """Returns a 3-D tensor: refused (the tasks need ``[B, d_r]``)."""

    def forward(self, x):
        return x.reshape(x.shape[0], -1, 1)
