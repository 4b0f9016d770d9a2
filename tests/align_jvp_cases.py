"""Shared inputs and references of the tests of ``cvf_align_feature_jvp`` (tests/test_align_jvp_gpu.py).

Shapes: those of tests/test_align_vjp_gpu.py (``case``), the weighted large frames of tests/weighted_large_cases.py (a leading
``w``: ``wmixed65``) and two feature layers without alignment (``feat10``: the mixed list on 10 atoms, every atom read;
``feat65``: a random list on 65 atoms, some atoms unread).  The reference is the fp64 oracle (``oracle.pp.AlignFeature`` /
``features_of``) with the tangent taken by ``torch.autograd.forward_ad`` and the cotangent by reverse mode; every reference is
computed once per (shape, batch, angle mode) and shared read-only."""
import functools
import types

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from tests.synth import make_molecule_traj
from tests.test_align_vjp_gpu import LARGE_TOL, MIXED, SMALL_TOL, case, random_features, rel_err  # noqa: F401  (re-exported)
from tests.weighted_large_cases import frames as weighted_frames, weights_for

FEATURES_ONLY = {"feat10": (10, MIXED), "feat65": (65, random_features(65, 65))}


@functools.lru_cache(maxsize=None)
def inputs(name, B):
    """Everything about a shape that does not depend on the device: atoms, tables, frames, a tangent u and a cotangent seed."""
    s = types.SimpleNamespace(name=name, B=B, weights_any_size=False)
    if name in FEATURES_ONLY:
        s.n, s.feats = FEATURES_ONLY[name]
        s.align, s.w = None, None
        s.traj, _, s.ref = make_molecule_traj(s.n, B, seed=900 + s.n + B)
    elif name.startswith("w") and name[1:] in ("mixed65", "mixed1000"):   # weighted alignment on a frame of more than 64 atoms
        s.n, s.align, s.feats, _ = case(name[1:])
        s.traj, _, s.ref = weighted_frames(s.n, B, seed=700 + s.n)
        s.w, s.weights_any_size = weights_for(s.n, len(s.align)), True
    else:
        s.n, s.align, s.feats, s.w = case(name)
        s.traj, _, s.ref = make_molecule_traj(s.n, B, seed=100 + s.n)
    s.traj.setflags(write=False)
    gen = torch.Generator().manual_seed(17 * B + s.n)
    s.u = torch.randn(B, s.n, 3, generator=gen, dtype=torch.float64)
    s.gen_seed = 29 * B + s.n
    used = {a for _, atoms in s.feats for a in atoms} | set(s.align or [])
    s.unused = [a for a in range(s.n) if a not in used]
    s.tol = SMALL_TOL if 3 * s.n <= 192 or s.align is None else LARGE_TOL   # (the two bars are one number; the name says which kernel)
    return s


def cotangent(s, d_r):
    return torch.randn(s.B, d_r, generator=torch.Generator().manual_seed(s.gen_seed), dtype=torch.float64)


def layer_of(s, angle_value, dev, **kw):
    from colvarsfinder import pp
    if s.align is None:
        return pp.AlignFeatureLayer(s.n, None, None, s.feats, angle_value, **kw).to(dev)
    return pp.AlignFeatureLayer(s.n, s.align, s.ref[s.align], s.feats, angle_value, align_weights=s.w,
                                weights_any_size=s.weights_any_size, **kw).to(dev)


def oracle_of(s, angle_value):
    """The fp64 oracle of the shape as a callable on [B, N, 3] (build and call under the fp64 default dtype)."""
    from oracle.pp import AlignFeature, features_of
    if s.align is None:
        return lambda x: features_of(x, s.feats, angle_value)
    return AlignFeature(s.align, s.ref[s.align], s.feats, angle_value, align_weights=s.w)


@functools.lru_cache(maxsize=None)
def oracle_refs(name, B, angle_value):
    """(q_ref [B, d_r] = J u, gx_ref [B, 3N] = J^T g, g [B, d_r]) in fp64."""
    s = inputs(name, B)
    torch.set_default_dtype(torch.float64)
    try:
        f = oracle_of(s, angle_value)
        x = torch.tensor(s.traj, dtype=torch.float64)
        with fwAD.dual_level():
            q = fwAD.unpack_dual(f(fwAD.make_dual(x, s.u))).tangent.clone()
        g = cotangent(s, q.shape[1])
        xr = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad(f(xr), xr, g)
    finally:
        torch.set_default_dtype(torch.float32)
    q, gx = q.numpy(), gx.reshape(B, -1).numpy()
    q.setflags(write=False)
    gx.setflags(write=False)
    return q, gx, g


def abi_fwd(layer, traj):
    """(x [B, N, 3] fp32 on the device, aux rows or None) of one cvf_align_feature_fwd call."""
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    dev = layer.rec.device
    x = torch.tensor(np.asarray(traj)).to(device=dev, dtype=torch.float32).contiguous()
    B = x.shape[0]
    desc = layer.pp_desc()
    out = torch.empty(B, layer.d_r, device=dev)
    aux = torch.empty(_hip.ntiles(B), _hip.AUX_ROWS, _hip.TILE, device=dev) if layer.aligned else None
    _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, None, P(out), P(aux), P(_hip.align_scratch(desc, B, dev)), _hip.stream()),
               "cvf_align_feature_fwd")
    return x, aux


def abi_jvp(layer, x, aux, u):
    """q [B, d_r] of cvf_align_feature_jvp; q starts as NaN."""
    from colvarsfinder import _hip
    u = u.to(device=x.device, dtype=torch.float32).reshape(x.shape).contiguous()
    q = torch.full((x.shape[0], layer.d_r), float("nan"), device=x.device)
    _hip.check(_hip.lib().cvf_align_feature_jvp(layer.pp_desc(), _hip.ptr(x), x.shape[0], _hip.ptr(aux), _hip.ptr(u), _hip.ptr(q),
                                                _hip.stream()), "cvf_align_feature_jvp")
    torch.cuda.synchronize()
    return q


def abi_vjp(layer, x, aux, g):
    """gx [B, 3N] of cvf_align_feature_vjp; gx starts as NaN."""
    from colvarsfinder import _hip
    g = g.to(device=x.device, dtype=torch.float32).contiguous()
    gx = torch.full((x.shape[0], 3 * x.shape[1]), float("nan"), device=x.device)
    _hip.check(_hip.lib().cvf_align_feature_vjp(layer.pp_desc(), _hip.ptr(x), x.shape[0], _hip.ptr(aux), _hip.ptr(g), _hip.ptr(gx),
                                                _hip.stream()), "cvf_align_feature_vjp")
    torch.cuda.synchronize()
    return gx
