"""Bias energy and forces along a CV in one launch (csrc/cv_bias.hip, cvf_cv_*_bias_*; the term formulas: csrc/cvf_bias.hpp): the
models, the bias cases, the bias written independently in torch (the reference of both test files) and the bars.
`tests/test_cv_bias_host.py` (CPU) and `tests/test_cv_bias_gpu.py` (GPU) share it.

Shapes are the smallest that exercise every index: 7 atoms aligned on 5 of them that are not 0..4 under one feature of each of the
four types (the wave kernel), the same feature list spread over 70 atoms (the workgroup kernel; per-atom alignment weights in one
model), one CVF_PP_IDENTITY model with n_coord = 6; nets [d_r, 5, 1] x 2 (form A), [d_r, 4, 2] (form B), a SharedEigenFunctions
with k = 2 (form C).  B = 3 different frames throughout.

The reference of U is written here without a look at csrc/cvf_bias.hpp: the Hermite interpolant in its textbook basis on the node
positions lo + j / inv_h, U' by torch autograd of that U (never a coded derivative), everything in fp64 on the fp32 parameters.
"""
import numpy as np
import torch

from tests.synth import make_molecule_traj

B = 3
FEATS7 = [("position", (2, 5)), ("bond", (0, 6)), ("angle", (1, 3, 4)), ("dihedral", (0, 2, 4, 6))]
ALIGN7 = [1, 2, 3, 5, 6]

# Bars (metric: max abs error per frame / the reference's max abs over the frames, for U and for the force; fp64 autograd of
# U(xi(x)) as the reference).  Each is three times the worst case measured on the MI355X over BIAS_CASES x every model below (the
# project's convention) and stays within the standing bar of the coef-form gradient (tests/test_cv_jacobian_gpu.J_TOL = 1.5e-6)
# times max(1, kappa), taken with max(1, kappa) = 1 for every case (kappa is 0.7 .. 1.5 here): the only new error source is
# kappa * delta xi.  Achieved: beside each bar and in DESIGN.md section 4.18 (the kernels have no atomics: the figures repeat).
U_TOL = 6.6e-7     # achieved 2.19e-7 (wave-A, linear); 2.3e-8 .. 2.2e-7 over the 56 (model, case) pairs
F_TOL = 1.5e-6     # achieved 6.88e-7 (wave-C, linear), 6.5e-8 .. 6.9e-7 over the pairs; three times that is 2.06e-6, past the standing bar
DU_TOL = 3.6e-7    # achieved 1.18e-7 (large-B, table); not asked for by name - dU is what the force is built from

MODELS_WAVE = ["wave-A", "wave-B", "wave-C", "wave-identity"]
MODELS_LARGE = ["large-A", "large-B", "large-C", "large-A-weighted"]
BIAS_CASES = ["harmonic", "upper_wall", "lower_wall", "linear", "table", "table-node-at-xi", "three-on-one"]


def spread(feats, n_from, n_to):
    """The feature list with its atoms spread over n_to atoms (an injective, increasing map)."""
    m = lambda a: a * (n_to - 1) // (n_from - 1)
    return [(t, tuple(m(a) for a in atoms)) for t, atoms in feats]


def model_parts(mid):
    """(n_atoms or None, align, features, weights, frames [B, ...] fp32, ref)."""
    if mid == "wave-identity":
        return None, None, None, None, np.random.RandomState(6).normal(size=(B, 6)).astype(np.float32), None
    if mid.startswith("wave"):
        traj, _, ref = make_molecule_traj(7, B, seed=407, sigma=0.8)
        return 7, ALIGN7, FEATS7, None, traj, ref
    traj, _, ref = make_molecule_traj(70, B, seed=470, sigma=0.8)
    align = [a for a in range(70) if a % 7 not in (0, 4)]            # 50 atoms, atom 0 not among them
    w = np.random.RandomState(5).uniform(0.3, 2.5, size=len(align)) if mid.endswith("weighted") else None
    return 70, align, spread(FEATS7, 7, 70), w, traj, ref


def hip_layer(mid, dev=None):
    from colvarsfinder import pp
    n, align, feats, w, _, ref = model_parts(mid)
    if n is None:
        return torch.nn.Identity()
    layer = pp.AlignFeatureLayer(n, align, ref[align], feats, False, align_weights=w, weights_any_size=w is not None)
    return layer if dev is None else layer.to(dev)


def torch_layer(mid, dtype):
    """The layer in plain torch on the CPU (oracle.pp.AlignFeature, as tests/cv_frame_cases.torch_layer builds it)."""
    from oracle.pp import AlignFeature
    n, align, feats, w, _, ref = model_parts(mid)
    if n is None:
        return torch.nn.Identity()
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return AlignFeature(align, ref[align], feats, False, align_weights=w)
    finally:
        torch.set_default_dtype(old)


def d_r_of(mid):
    layer = hip_layer(mid)
    return 6 if isinstance(layer, torch.nn.Identity) else layer.d_r


def nets_of(mid):
    """The torch module (CPU, fp32, seeded) of a model id: form A, B or C by the id's letter (identity: form A)."""
    from colvarsfinder import nn
    d_r = d_r_of(mid)
    torch.manual_seed(2000 + sum(map(ord, mid)))
    form = "A" if mid == "wave-identity" else mid.split("-")[1]
    if form == "A":
        return nn.EigenFunctions([d_r, 5, 1], 2, activation=torch.nn.Tanh())
    if form == "B":
        return torch.nn.Sequential(torch.nn.Linear(d_r, 4), torch.nn.Tanh(), torch.nn.Linear(4, 2))
    return nn.SharedEigenFunctions([d_r, 4], [4, 3, 1], 2)


def plan_of(nets):
    """(MLPDesc, cut, k, theta fp32 CPU, n_shared): cut = upto_layer (forms A, B) or n_shared (form C, the _shared entries)."""
    from colvarsfinder import core, nn
    if type(nets) is nn.SharedEigenFunctions:
        d, L, k, params, ns = core._CVModel._nets_plan_shared(nets)
        return d, ns, k, torch.cat([p.detach().reshape(-1).float() for p in params]), ns
    d, upto, k, params = core._CVModel._nets_plan(nets)
    return d, upto, k, torch.cat([p.detach().reshape(-1).float() for p in params]), 0


def xi_of(mid, nets, X, dtype):
    """xi [B, k] of frames X (a tensor of `dtype`, may require grad) through the torch layer and a copy of the nets, on the CPU."""
    import copy
    pp = torch_layer(mid, dtype)
    net = copy.deepcopy(nets).to(device="cpu", dtype=dtype)
    return net(pp(X)).reshape(X.shape[0], -1)


# ------------------------------------------------------------------------------------------------ the bias, independently
def f32(v):
    return float(np.float32(v))


def hermite_u(x, lo, inv_h, u_nodes, du_nodes):
    """U(x) of a table term in x's type: nodes at lo + j / inv_h, textbook cubic Hermite basis, linear continuation outside."""
    n = len(u_nodes)
    h = 1.0 / inv_h
    un, dn = torch.as_tensor(u_nodes, dtype=x.dtype), torch.as_tensor(du_nodes, dtype=x.dtype)
    pos = lo + torch.arange(n, dtype=x.dtype) * h
    j = torch.clamp(torch.searchsorted(pos, x.detach().contiguous(), right=True) - 1, 0, n - 2)   # (x on the last node: the last interval)
    t = (x - pos[j]) / h
    inner = ((1 + 2 * t) * (1 - t) ** 2 * un[j] + t * (1 - t) ** 2 * h * dn[j] + t ** 2 * (3 - 2 * t) * un[j + 1]
             + t ** 2 * (t - 1) * h * dn[j + 1])
    below = un[0] + dn[0] * (x - pos[0])
    above = un[-1] + dn[-1] * (x - pos[-1])
    return torch.where(x < pos[0], below, torch.where(x > pos[-1], above, inner))


def ref_bias(terms, xi):
    """U [B] of xi [B, k] for a list of term dicts (the vocabulary of colvarsfinder.export.bias_desc), in xi's type; the
    parameters are taken as the fp32 numbers the kernels get."""
    U = torch.zeros_like(xi[:, 0])
    for t in terms:
        x = xi[:, t["cv"]]
        kind = t["kind"]
        if kind == "table":
            U = U + hermite_u(x, f32(t["lo"]), f32(t["inv_h"]), np.float32(t["u"]).astype(np.float64), np.float32(t["du"]).astype(np.float64))
            continue
        kappa, c = f32(t["kappa"]), f32(t.get("center", 0.0))
        e = 0.5 * kappa * (x - c) ** 2
        if kind == "harmonic":
            U = U + e
        elif kind == "upper_wall":
            U = U + torch.where(x > c, e, torch.zeros_like(e))
        elif kind == "lower_wall":
            U = U + torch.where(x < c, e, torch.zeros_like(e))
        elif kind == "linear":
            U = U + kappa * x
        else:
            raise AssertionError(kind)
    return U


def ref_u_du(terms, xi_np):
    """(U [B], dU [B, k]) in fp64, dU by autograd of ref_bias."""
    xi = torch.tensor(np.asarray(xi_np, dtype=np.float64), requires_grad=True)
    U = ref_bias(terms, xi)
    dU, = torch.autograd.grad(U.sum(), xi, allow_unused=True)
    return U.detach().numpy(), (torch.zeros_like(xi) if dU is None else dU).numpy()


def smooth_table(cv, lo, inv_h, n_nodes, x0):
    """A table term whose nodes sample f(x) = 1 + sin(x - x0) + 0.5 (x - x0): values, slopes and curvature of order 1."""
    lo, inv_h = np.float32(lo), np.float32(inv_h)
    x = np.float64(lo) + np.arange(n_nodes) / np.float64(inv_h)
    return {"kind": "table", "cv": cv, "lo": float(lo), "inv_h": float(inv_h), "u": 1.0 + np.sin(x - x0) + 0.5 * (x - x0), "du": np.cos(x - x0) + 0.5}


def terms_for(case, xi0):
    """The terms of a bias case, placed around xi0 [B, k] (fp32, what a prior cvf_cv_frame_eval gave for the B = 3 frames) so that
    the frames fall on either side of what the case is about.  CV 0 carries the case; every case but three-on-one also puts a
    harmonic term on the last CV, so that every coefficient of the sweep is in use.  The restraints sit 1.5 from the frames: U and
    dU/dxi are then of the order of xi itself, and an error delta xi of the nets shows as kappa delta xi and not magnified by a
    small denominator (the metric divides by the largest |U| and |force| of the case)."""
    xi0 = np.asarray(xi0, dtype=np.float64)
    k = xi0.shape[1]
    lo_, mid_, hi_ = np.sort(xi0[:, 0])
    assert hi_ - mid_ > 1e-3 and mid_ - lo_ > 1e-3, "the frames' xi_0 lie too close to place a bias between them"
    other = [{"kind": "harmonic", "cv": k - 1, "kappa": 0.8, "center": float(xi0[:, k - 1].min() - 1.5)}] if k > 1 else []
    if case == "harmonic":
        return [{"kind": "harmonic", "cv": 0, "kappa": 1.3, "center": float(lo_ - 1.5)}] + other
    if case == "upper_wall":     # two frames above the wall, one below
        return [{"kind": "upper_wall", "cv": 0, "kappa": 1.5, "center": float(0.5 * (lo_ + mid_))}] + other
    if case == "lower_wall":     # two frames below the wall, one above
        return [{"kind": "lower_wall", "cv": 0, "kappa": 1.5, "center": float(0.5 * (mid_ + hi_))}] + other
    if case == "linear":
        return [{"kind": "linear", "cv": 0, "kappa": -1.2}] + other
    h = 0.3 * min(mid_ - lo_, hi_ - mid_)
    if case == "table":          # five nodes: one frame below lo, one inside interval 1 of 0..3, one above the last node
        return [smooth_table(0, mid_ - 1.5 * h, 1.0 / h, 5, mid_)] + other
    if case == "table-node-at-xi":   # node 2 sits on fp32(xi) of the middle frame: a power-of-two spacing for which lo + 2 h is exact
        h2 = 2.0 ** np.floor(np.log2(h))
        while float(np.float32(mid_) - np.float32(2.0 * h2)) + 2.0 * h2 != mid_:
            h2 *= 0.5
        return [smooth_table(0, np.float32(mid_) - np.float32(2.0 * h2), 1.0 / h2, 5, mid_)] + other
    if case == "three-on-one":   # a restraint and two walls on CV 0
        return [{"kind": "harmonic", "cv": 0, "kappa": 0.7, "center": float(lo_ - 1.5)},
                {"kind": "upper_wall", "cv": 0, "kappa": 1.1, "center": float(0.5 * (mid_ + hi_))},
                {"kind": "lower_wall", "cv": 0, "kappa": 0.9, "center": float(0.5 * (lo_ + mid_))}]
    raise AssertionError(case)


def reference(mid, nets, frames, terms):
    """(U [B], dU [B, k], force [B, n_coord]) by torch fp64 autograd of U(xi(x)) on the CPU."""
    X = torch.tensor(np.asarray(frames), dtype=torch.float64, requires_grad=True)
    xi = xi_of(mid, nets, X, torch.float64)
    xi.retain_grad()
    U = ref_bias(terms, xi)
    U.sum().backward()
    return U.detach().numpy(), xi.grad.numpy(), -X.grad.reshape(X.shape[0], -1).numpy()


def rel_rows(got, want):
    """max abs error per frame / the reference's max abs (over all frames)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())
