"""Shared inputs and references of the tests of ``cvf_align_feature_hvp`` (tests/test_align_hvp_gpu.py, tests/test_align_hvp_host.py).

Shapes, frames, tangents and cotangents are those of tests/align_jvp_cases.py.  The reference is the fp64 oracle
(``oracle.pp.AlignFeature`` / ``features_of``) differentiated twice in reverse mode, ``h_ref = grad(<grad(f(x), g), u>, x)``; the
*fp32 twin* is the same graph through the same oracle code in fp32 on the CPU.  Every reference is computed once per (shape,
batch, angle mode, tangent) and shared read-only.

Error measure: per frame ``e_f = max_j |h - h_ref| / max_j |h_ref|``, the worst frame counts.  Bar of a case:
``max(1.5e-5, 3 x the twin's worst-frame e_f on the same inputs)`` - 1.5e-5 is the bar of the VJP and of the JVP, 3 the project's
margin over a twin; the twin term is there because the Hessian amplifies near-degenerate angles and dihedrals
in ANY fp32 evaluation (the twin alone misses 1.5e-5 on some shapes)."""
import functools

import numpy as np
import torch

from tests.align_jvp_cases import abi_fwd, abi_jvp, abi_vjp, cotangent, inputs, layer_of, oracle_of  # noqa: F401  (re-exported)

FLOOR = 1.5e-5
TWIN_MARGIN = 3.0


def tangent(s, which):
    """Tangent number ``which`` of the shape: 0 is ``s.u`` of tests/align_jvp_cases.py, the others are drawn here."""
    if which == 0:
        return s.u
    gen = torch.Generator().manual_seed(1000 * which + 17 * s.B + s.n)
    return torch.randn(s.B, s.n, 3, generator=gen, dtype=torch.float64)


def frame_errors(got, want):
    """e_f of every frame: [B]."""
    got = np.asarray(got, dtype=np.float64).reshape(len(want), -1)
    want = np.asarray(want, dtype=np.float64).reshape(len(want), -1)
    return np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)


def double_backward(f, x, g, u):
    """(gx, h) = (grad(f(x), g), grad(<gx, u>, x)) through any differentiable ``f``; ``x`` is not modified."""
    x = x.detach().clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(f(x), x, g, create_graph=True)
    (h,) = torch.autograd.grad(gx, x, u.reshape(x.shape))
    return gx.detach(), h


def _oracle_hvp(s, angle_value, u, dtype):
    torch.set_default_dtype(dtype)   # (the oracle's buffers take the default type when it is built)
    try:
        f = oracle_of(s, angle_value)
        x = torch.tensor(s.traj, dtype=dtype)
        d_r = f(x[:1]).shape[1]
        _, h = double_backward(f, x, cotangent(s, d_r).to(dtype), u.to(dtype))
    finally:
        torch.set_default_dtype(torch.float32)
    return h.double().reshape(s.B, -1).numpy()


@functools.lru_cache(maxsize=None)
def hvp_refs(name, B, angle_value, which=0):
    """(h_ref [B, 3N] fp64, twin_err: the fp32 twin's worst-frame e_f, bar of the case)."""
    s = inputs(name, B)
    u = tangent(s, which)
    h_ref = _oracle_hvp(s, angle_value, u, torch.float64)
    assert np.isfinite(h_ref).all() and (np.abs(h_ref).max(axis=1) > 0).all()
    twin_err = float(frame_errors(_oracle_hvp(s, angle_value, u, torch.float32), h_ref).max())
    h_ref.setflags(write=False)
    return h_ref, twin_err, max(FLOOR, TWIN_MARGIN * twin_err)


def abi_hvp(layer, x, aux, g, u):
    """h [B, 3N] of cvf_align_feature_hvp; h starts as NaN."""
    from colvarsfinder import _hip
    g = g.to(device=x.device, dtype=torch.float32).contiguous()
    u = u.to(device=x.device, dtype=torch.float32).reshape(x.shape).contiguous()
    h = torch.full((x.shape[0], 3 * x.shape[1]), float("nan"), device=x.device)
    _hip.check(_hip.lib().cvf_align_feature_hvp(layer.pp_desc(), _hip.ptr(x), x.shape[0], _hip.ptr(aux), _hip.ptr(g), _hip.ptr(u),
                                                _hip.ptr(h), _hip.stream()), "cvf_align_feature_hvp")
    torch.cuda.synchronize()
    return h


# ------------------------------------------------------------------------------------------------
# The closed form of the rigid-body part (position records) in fp64 NumPy, one frame - the formulas the kernels evaluate
# (csrc/k1_hvp.hip, header), in the notation of oracle/pp.py.
# ------------------------------------------------------------------------------------------------
def rigid_hvp_np(x, align_idx, ref_pos, pos_atoms, g, u, weights=None):
    """h [N, 3] = d/dx <g, J(x) u> of the aligned positions of ``pos_atoms`` (g [n_pos, 3], u [N, 3]); ``weights``: the per-atom
    alignment weights, any positive scale."""
    from oracle.pp import _ax, _skew
    x, u, g = (np.asarray(v, dtype=np.float64) for v in (x, u, g))
    al, n = np.asarray(align_idx), len(align_idx)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64) * (n / np.sum(weights))   # mean 1
    ref = np.asarray(ref_pos, dtype=np.float64)
    ref_c = w[:, None] * (ref - (w[:, None] * ref).mean(axis=0))       # as the kernels store it: centred, times w_b
    c = (w[:, None] * x[al]).mean(axis=0)
    H = (x[al] - c).T @ ref_c
    U, _, Vh = np.linalg.svd(H)
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vh))]) @ Vh
    S = R.T @ H
    Kinv = np.linalg.inv(np.trace(S) * np.eye(3) - 0.5 * (S + S.T))
    ubar = (w[:, None] * u[al]).mean(axis=0)
    dH = (u[al] - ubar).T @ ref_c
    dR = R @ _skew(Kinv @ _ax(R.T @ dH))
    dS = dR.T @ H + R.T @ dH
    dK = np.trace(dS) * np.eye(3) - 0.5 * (dS + dS.T)
    M = sum(np.outer(x[a] - c, g[i]) for i, a in enumerate(pos_atoms))
    dM = sum(np.outer(u[a] - ubar, g[i]) for i, a in enumerate(pos_atoms))
    sv = Kinv @ _ax(R.T @ M)
    ds = Kinv @ (_ax(dR.T @ M + R.T @ dM) - dK @ sv)
    dZ = dR @ _skew(sv) + R @ _skew(ds)
    h = np.zeros_like(x)
    dp = g @ dR.T                                   # dR g_a per position record
    for i, a in enumerate(pos_atoms):
        h[a] += dp[i]
    h[al] += ref_c @ dZ.T - w[:, None] * dp.sum(axis=0) / n
    return h
