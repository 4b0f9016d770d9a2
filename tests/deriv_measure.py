"""The per-frame, per-feature-type error measure of the derivative tests of the alignment + feature layer, for any feature list
(tests/align_deriv_cases.py, tests/test_align_vjp_gpu.py, tests/test_align_jvp_gpu.py, tests/test_align_deriv_host.py).  Imports
no other test module, so every one of them can import it at module level.

VJP: one run per type with the cotangent restricted to the type's columns, one with the dense cotangent; the reference of a type is
the fp64 oracle built from the list's records of that type (independent terms of J^T g).  JVP: the output columns grouped by type.
``e_f = max_j |got - ref| / max_j |ref|`` per frame, the worst frame counts.  Bar: ``max(FLOOR, TWIN_MARGIN x the fp32 twin's
worst-frame error on the same inputs and type)``, and never above ``CEILING``: where three times the twin exceeds it the bar IS the
ceiling, which asks more of the kernel than the rule does (``TWIN_ABOVE_CEILING`` names the shapes of the two older tests where
that happens or comes close; the lists of tests/align_deriv_cases.py are drawn so that it never does)."""
import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

FLOOR, TWIN_MARGIN, CEILING = 1.5e-5, 3.0, 1e-4
DENSE = "dense"

# (test, shape, angle_value, type): unfiltered lists (tests/test_align_vjp_gpu.py: random_features, MIXED) whose fp32 twin alone is
# within a factor two of CEILING / TWIN_MARGIN on some frame - an angle near the ends of acos, a nearly straight dihedral axis.
# Their bars are capped at CEILING; every other (shape, type) of the two tests keeps 3 x twin <= CEILING (asserted on the CPU).
TWIN_ABOVE_CEILING = {
    ("vjp", "weighted12_mixed", True, "angle"), ("vjp", "mixed65", True, "angle"),        # 3 x twin = 2.1e-4, 1.7e-4
    ("jvp", "weighted12_mixed", True, "angle"), ("jvp", "mixed65", True, "angle"),        # 2.5e-4, 1.9e-4
    ("vjp", "mixed10", False, "dihedral"), ("jvp", "wmixed65", False, "dihedral"),        # 6.7e-5, 6.5e-5: close to it
}


def frame_errors(got, want):
    """e_f of every frame: [B]."""
    got = np.asarray(got, dtype=np.float64).reshape(len(want), -1)
    want = np.asarray(want, dtype=np.float64).reshape(len(want), -1)
    return np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)


def bar_of(twin):
    return min(max(FLOOR, TWIN_MARGIN * twin), CEILING)


def columns_of(feats, angle):
    """{type: output columns} of a feature list, in list order."""
    cols, out = {}, 0
    for t, atoms in feats:
        w = 3 * len(atoms) if t == "position" else (2 if t == "dihedral" and not angle else 1)
        cols.setdefault(t, []).extend(range(out, out + w))
        out += w
    return {t: np.asarray(c) for t, c in cols.items()}


def oracle_builder(n, align, ref, weights, angle):
    """oracle_for(feature list): the oracle of the list under the current default dtype (grouped evaluation above 64 atoms)."""
    from oracle.pp import AlignFeature, features_of

    def oracle_for(feats):
        if align is None:
            return lambda x: features_of(x, feats, angle, n > 64)
        return AlignFeature(align, ref[align], feats, angle, align_weights=weights, compact=n > 64)

    return oracle_for


def _both_dtypes(fn):
    out = []
    for dtype in (torch.float64, torch.float32):
        torch.set_default_dtype(dtype)   # (the oracle's buffers take the default type when it is built)
        try:
            out.append(fn(dtype))
        finally:
            torch.set_default_dtype(torch.float32)
    return out


def masked(g, cols):
    """g restricted to the columns `cols` (None: all of it)."""
    if cols is None:
        return g
    gm = torch.zeros_like(g)
    gm[:, cols] = g[:, cols]
    return gm


def vjp_type_refs(feats, angle, oracle_for, traj, g):
    """{type or DENSE: (columns or None, J^T g_type [B, 3N] in fp64, the fp32 twin's worst-frame error)}."""
    B, out = len(traj), {}
    for t, c in [(DENSE, None)] + list(columns_of(feats, angle).items()):
        sub = feats if c is None else [f for f in feats if f[0] == t]

        def run(dtype):
            x = torch.tensor(np.asarray(traj), dtype=dtype, requires_grad=True)
            (gx,) = torch.autograd.grad(oracle_for(sub)(x), x, (g if c is None else g[:, c]).to(dtype))
            return gx.double().reshape(B, -1).numpy()

        r64, r32 = _both_dtypes(run)
        out[t] = (c, r64, float(frame_errors(r32, r64).max()))
    return out


def jvp_type_refs(feats, angle, oracle_for, traj, u):
    """(J u [B, d_r] in fp64, {type: (columns, the fp32 twin's worst-frame error inside them)})."""
    def run(dtype):
        x = torch.tensor(np.asarray(traj), dtype=dtype)
        with fwAD.dual_level():
            return fwAD.unpack_dual(oracle_for(feats)(fwAD.make_dual(x, u.to(dtype)))).tangent.double().numpy().copy()

    r64, r32 = _both_dtypes(run)
    return r64, {t: (c, float(frame_errors(r32[:, c], r64[:, c]).max())) for t, c in columns_of(feats, angle).items()}
