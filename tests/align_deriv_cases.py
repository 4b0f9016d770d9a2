"""Case table, mirrors and references of the direct tests of the four derivative entry points of the alignment + feature layer,
``cvf_align_feature_vjp``, ``_vjp_rows``, ``_jvp`` and ``_hvp`` (tests/test_align_deriv_host.py, tests/test_align_deriv_gpu.py), on
every compiled instance of their kernels (csrc/k1_vjp.hip, k1_vjp_large.hpp, k1_jvp.hip, k1_hvp.hip; without alignment
csrc/k1_features.hip).

Which instance a call launches is asked of ``cvf_align_feature_deriv_route`` - the function the launches themselves decide by.  Its
rules are mirrored below (``vjp_small``, ``rows_small``, ``jvp_small``, ``hvp_small``, ``rows_large``, ``feat_plan``, ``feat_bytes``);
the host test fails when a mirror and the library disagree.

Feature lists are drawn on ``metric_cases.frames(n, seed)``, each record accepted by ``_ok_bond / _ok_angle / _ok_dihedral`` on all
130 frames (no bond shorter than 1, no bond angle within 37 degrees of straight).  Every aligned list has a partial alignment set and
position records; the last atom of every frame is read by nothing.

Reference: ``oracle.pp.AlignFeature`` / ``features_of`` in fp64 (``compact=True`` above 64 atoms) - reverse mode for J^T g, ``forward_ad``
for J u, a double backward for the Hessian-vector product; lists of more than 256 records are evaluated ``compact`` as well (the
per-record graph of 2 758 records costs a quarter of a minute per case, the grouped one the same formulas in a second).  The *fp32 twin* is the same graph in fp32 on the CPU.  The cotangent
restricted to the columns of one feature type is J^T g of the list's records of that type alone (the records are independent terms
of J^T g), so the reference of a type is the oracle built from those records; the dense reference is computed on the whole list, and
``reference`` asserts that the types add up to it.

Error measure: per frame and per feature type.  VJP, vjp_rows, HVP: one run per type with the cotangent restricted to the type's
columns, one with the dense cotangent; ``e_f = max_j |got - ref| / max_j |ref|`` per frame, the worst frame counts.  JVP: the output
columns grouped by type, the same per-frame ratio inside each group.  Bar of a case, quantity and type: ``max(FLOOR, TWIN_MARGIN x the
twin's worst-frame error on the same inputs and type)``, never above ``CEILING`` - a condition on the inputs that the host test
asserts on the CPU.  The bars are never read off the kernels.

What the table cannot reach, with the arithmetic:

* ``jvp_align_kernel<true, false>`` is not compiled: the tables are never staged without the q image.
* The small-frame kernels at fewer than 64 atoms with their tables outside the LDS would need more records still
  (``6 n_rec + 4 n_align > 40 960 - 128 stride`` floats for the VJP: 21 600 records at 40 atoms); 64 atoms is where the lists are
  shortest, so the ``<false>`` instances run there only.
* ``lg = 0`` of the features VJP needs ``n_slot + n_ref > 2 730`` (``(n_slot + n_ref) 12 x 2 > 65 536``), of the metric kernel at one
  net ``n_slot + n_ref > 3 072``; both are within the limits of include/cvf.h and in the table."""
import ctypes as C
import functools
import types
from collections import namedtuple

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from tests.align_hvp_cases import double_backward
from tests.deriv_measure import DENSE, bar_of, columns_of, frame_errors  # noqa: F401  (re-exported)
from tests.metric_cases import (BATCHES, CEILING, FLOOR, TILE, TWIN_MARGIN, _ok_angle, _ok_bond, _ok_dihedral, frames, n_tiles,  # noqa: F401
                                same_bits, x_tile_stride)
from tests.synth import diag_coeff_for

LIMIT = 160 * 1024                  # LDS of a workgroup
SMALL_ROWS_BUDGET = 40 * 1024       # vjp_rows_small_kernel: gradient images per pass
LARGE_ROWS_BUDGET = 64 * 1024       # vjp_rows_[weighted_]large_kernel: rows per launch
FEAT_BUDGET, METRIC_BUDGET = 64 * 1024, 72 * 1024   # kLdsBudget, kMetricBudget (csrc/k1_features.hip)
MAX_SLOT, MAX_REF, MAX_NETS = 4096, 6144, 8
VJP, VJP_ROWS, JVP, HVP, FWD, METRIC = range(6)     # CVF_DERIV_*
IDENTITY, FEATURES, SMALL, LARGE = range(4)         # CVF_DERIV_ROUTE_*
WHICH = {"vjp": VJP, "rows": VJP_ROWS, "jvp": JVP, "hvp": HVP, "fwd": FWD, "metric": METRIC}
TYPES = ("position", "bond", "angle", "dihedral")


# ------------------------------------------------------------------------------------------------ mirrored rules
def img_bytes(nc):
    return TILE * x_tile_stride(nc) * 4


def tables_bytes(n_rec, nal):
    return (6 * n_rec + 4 * nal) * 4


def vjp_small(nc, n_rec, nal):
    """(tables_lds, lds_bytes) of vjp_align_kernel."""
    base = 2 * img_bytes(nc)
    t = int(base + tables_bytes(n_rec, nal) <= LIMIT)
    return t, base + t * tables_bytes(n_rec, nal)


def rows_small(nc, n_rec, nal, k):
    """(tables_lds, kg, lds_bytes) of vjp_rows_small_kernel."""
    img, tab = img_bytes(nc), tables_bytes(n_rec, nal)
    per_row = img + 12 * TILE * 4
    t = int(img + per_row + tab <= LIMIT)
    fixed = img + t * tab
    if fixed + per_row * k <= SMALL_ROWS_BUDGET:
        kg = k
    else:
        kg = (SMALL_ROWS_BUDGET - fixed if SMALL_ROWS_BUDGET > fixed + per_row else per_row) // per_row
    kg = max(kg, 1)
    return t, kg, fixed + per_row * kg


def jvp_small(nc, d_r, n_rec, nal):
    """(tables_lds, q_lds, lds_bytes) of jvp_align_kernel."""
    tiles, q, tab = 2 * img_bytes(nc), TILE * (d_r | 1) * 4, tables_bytes(n_rec, nal)
    ql = int(tiles + q <= LIMIT)
    tl = int(ql and tiles + q + tab <= LIMIT)
    return tl, ql, tiles + ql * q + tl * tab


def hvp_small(nc, n_rec, nal):
    """(tables_lds, lds_bytes) of hvp_align_kernel."""
    base = 3 * img_bytes(nc)
    t = int(base + tables_bytes(n_rec, nal) <= LIMIT)
    return t, base + t * tables_bytes(n_rec, nal)


def rows_large(n_ref, k):
    """(kg, launches, lds_bytes of the first launch) of vjp_rows_[weighted_]large_kernel."""
    per_row = (3 * n_ref + 60) * 4
    kg = k if per_row * k <= LARGE_ROWS_BUDGET else max(LARGE_ROWS_BUDGET // per_row, 1)
    return kg, (k + kg - 1) // kg, per_row * kg


def feat_plan(bytes_per_frame, budget=FEAT_BUDGET):
    """(lg, lds_bytes): the frames per workgroup halve until their image fits the budget."""
    lg = 6
    while lg > 0 and (bytes_per_frame << lg) > budget:
        lg -= 1
    return lg, bytes_per_frame << lg


def feat_bytes(which, n_slot, n_ref, k=1):
    """(bytes per frame, budget, u_lds, rows_per_launch) of the CVF_PP_FEATURES launch `which`."""
    if which == FWD:
        return n_slot * 12, FEAT_BUDGET, 0, 1
    if which in (VJP, VJP_ROWS):
        return (n_slot + n_ref) * 12, FEAT_BUDGET, 0, k if which == VJP_ROWS else 1
    if which == JVP:
        return n_slot * 24, FEAT_BUDGET, 0, 1
    if which == HVP:
        u = int((2 * n_slot + n_ref) * 12 <= LIMIT)
        return ((1 + u) * n_slot + n_ref) * 12, FEAT_BUDGET, u, 1
    kc = k
    while kc > 1 and n_slot * 12 + kc * n_ref * 12 > METRIC_BUDGET:
        kc -= 1
    passes = (k + kc - 1) // kc
    kc = (k + passes - 1) // passes
    return n_slot * 12 + kc * n_ref * 12, METRIC_BUDGET, 0, kc


# ------------------------------------------------------------------------------------------------ cases
# kind: small (aligned, at most 64 atoms) | large (aligned, more) | feat (no alignment).  counts = (position atoms, bonds, angles,
# dihedrals).  runs: the entry points the GPU test takes the case through.  k: the cotangents of vjp_rows (and the nets of the
# features metric).
Case = namedtuple("Case", "id kind n counts n_align weighted angle B k runs seed")
ALL4 = ("vjp", "rows", "jvp", "hvp")


def _small(id, n, counts, B, k, runs=ALL4, nal=14, weighted=False, angle=False, seed=3):
    return Case(id, "small", n, tuple(counts), nal, weighted, angle, B, k, tuple(runs), seed)


def _large(id, n, counts, B, k, weighted, angle=False, seed=0):
    return Case(id, "large", n, tuple(counts), 2 * n // 3, weighted, angle, B, k, ALL4, seed)


def _feat(id, n, n_slot, n_pos, n_ang, n_dih, B, k=2, angle=False, seed=0):
    n_bond = (n_slot - n_pos + 1) // 2                      # the bonds that pair up the pool atoms without a position record
    return Case(id, "feat", n, (n_pos, n_bond, n_ang, n_dih), n_slot, False, angle, B, k, ALL4 + ("fwd", "metric"), seed)


def counts_of(counts, angle):
    """(n_rec, d_r, n_ref) of a list with these counts."""
    p, b, a, d = counts
    return p + b + a + d, 3 * p + b + a + (1 if angle else 2) * d, p + 2 * b + 3 * a + 4 * d


def edge(pred, counts, angle=False):
    """The two lists on the sides of a threshold: bonds are added to `counts` while pred(n_rec, d_r) holds - (last list that
    keeps it, first that does not), one record apart."""
    p, b, a, d = counts
    assert pred(*counts_of(counts, angle)[:2]), counts
    while pred(*counts_of((p, b + 1, a, d), angle)[:2]):
        b += 1
    return (p, b, a, d), (p, b + 1, a, d)


NC64, NAL = 192, 14
VJP_EDGE = edge(lambda r, d: vjp_small(NC64, r, NAL)[0], (8, 1000, 862, 430))
ROWS_EDGE = edge(lambda r, d: rows_small(NC64, r, NAL, 3)[0], (8, 1000, 800, 364))
HVP_EDGE = edge(lambda r, d: hvp_small(NC64, r, NAL)[0], (8, 100, 160, 73))
JVPQ_EDGE = edge(lambda r, d: jvp_small(NC64, d, r, NAL)[1], (8, 20, 69, 20))
JVPT_EDGE = edge(lambda r, d: jvp_small(NC64, d, r, NAL)[0], (4, 20, 60, 20))
HEAVY = (8, 1400, 900, 450)

SMALL_CASES = [
    _small("heavy64", 64, HEAVY, 65, 3),
    _small("heavy64w", 64, HEAVY, 5, 8, weighted=True, angle=True),
    _small("vjp-tables-under", 64, VJP_EDGE[0], 5, 1, ("vjp",)),
    _small("vjp-tables-over", 64, VJP_EDGE[1], 1, 1, ("vjp",), angle=True),
    _small("rows-tables-under", 64, ROWS_EDGE[0], 5, 3, ("rows",)),
    _small("rows-tables-over", 64, ROWS_EDGE[1], 1, 8, ("rows",)),
    _small("hvp-tables-under", 64, HVP_EDGE[0], 64, 1, ("hvp",)),
    _small("hvp-tables-over", 64, HVP_EDGE[1], 63, 1, ("hvp",), angle=True),
    _small("jvp-q-under", 64, JVPQ_EDGE[0], 5, 1, ("jvp",)),
    _small("jvp-q-over", 64, JVPQ_EDGE[1], 130, 1, ("jvp",)),
    _small("jvp-tables-under", 64, JVPT_EDGE[0], 63, 1, ("jvp",)),
    _small("jvp-tables-over", 64, JVPT_EDGE[1], 65, 1, ("jvp",)),
    _small("qwin40", 40, (1, 200, 120, 60), 65, 1, ("jvp",), nal=10, angle=True),
    _small("rows10-k8", 10, (3, 3, 2, 2), 65, 8, ("vjp", "rows"), nal=6),
    _small("rows14-k3", 14, (4, 3, 2, 2), 130, 3, ("vjp", "rows"), nal=6, weighted=True),
]

R700, R1400 = (20, 100, 80, 60), (20, 200, 160, 125)        # n_ref = 700, 1400
LARGE_CASES = [
    # n % 4 != 0: the scalar-store instances; two launches at n_ref = 700 (kg = 7), three at 1400 (kg = 3)
    _large("lrows-n66-r700-u", 66, R700, 65, 8, False),
    _large("lrows-n66-r700-w", 66, R700, 5, 8, True, angle=True),
    _large("lrows-n66-r1400-u", 66, R1400, 63, 8, False, angle=True),
    _large("lrows-n66-r1400-w", 66, R1400, 65, 8, True),
    # n % 4 == 0: the 16-byte stores (and, with the output row offset by 4 bytes, the scalar ones again)
    _large("lrows-n68-r700-u", 68, R700, 65, 8, False, angle=True),
    _large("lrows-n68-r700-w", 68, R700, 1, 8, True),
    _large("lrows-n68-r1400-u", 68, R1400, 5, 8, False),
    _large("lrows-n68-r1400-w", 68, R1400, 65, 8, True, angle=True),
]
MISALIGNED = ("lrows-n68-r1400-u", "lrows-n68-r700-w")      # gx_rows / h_rows offset by 4 bytes: must equal the aligned call bit for bit

FEAT_CASES = [
    _feat("feat-s10", 12, 10, 4, 2, 1, 65),
    _feat("feat-s40", 48, 40, 10, 6, 4, 130, angle=True),
    _feat("feat-s80", 100, 80, 20, 14, 10, 63, k=1),
    _feat("feat-s160", 200, 160, 40, 30, 20, 64, k=1),
    _feat("feat-s330", 400, 330, 80, 60, 40, 65, k=1, angle=True),
    _feat("feat-s680", 800, 680, 170, 120, 80, 5, k=1),
    _feat("feat-s1000", 1200, 1000, 250, 180, 120, 65, k=8, angle=True),
    _feat("feat-s1400", 1600, 1400, 350, 250, 160, 1),
    _feat("feat-s4000", 4096, 4000, 2200, 300, 250, 5),
]

CASES = SMALL_CASES + LARGE_CASES + FEAT_CASES
BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------------ builders
@functools.lru_cache(maxsize=None)
def build(case):
    """Everything about a case that does not depend on the device: features, align set, weights, frames, cotangent, tangent."""
    s = types.SimpleNamespace(case=case)
    traj, _, s.ref = frames(case.n, case.seed)
    x = traj.astype(np.float64)
    s.traj = traj[:case.B]
    rs = np.random.RandomState(500 + 31 * case.n + sum(case.counts) + case.seed)
    p, b, a, d = case.counts
    n_read = case.n - 1                                       # the last atom is read by nothing
    if case.kind == "feat":
        pool = sorted(int(i) for i in rs.choice(n_read, case.n_align, replace=False))     # (n_align: n_slot of a features case)
        s.align, s.aw = None, None
    else:
        pool = list(range(n_read))
        s.align = sorted(int(i) for i in rs.choice(n_read, case.n_align, replace=False))
        s.aw = rs.uniform(0.2, 3.0, size=case.n_align) if case.weighted else None

    def draw(m, ok):
        for _ in range(10000):
            atoms = tuple(int(pool[i]) for i in rs.choice(len(pool), m, replace=False))
            if ok(x, *atoms):
                return atoms
        raise AssertionError(case.id)

    order = [pool[i] for i in rs.permutation(len(pool))]
    feats = [("position", tuple(order[:p]))]
    bonds = []
    if case.kind == "feat":                                   # every pool atom is read: pair up those without a position record
        rest = order[p:]
        if len(rest) % 2:
            rest.append(order[int(rs.randint(p))])
        for i, j in zip(rest[0::2], rest[1::2]):
            while not _ok_bond(x, i, j):                      # (a partner too close: any other pool atom, which then has one more bond)
                j = int(pool[int(rs.randint(len(pool)))])
            bonds.append((i, j))
        assert len(bonds) == b, case.id
    bonds += [draw(2, _ok_bond) for _ in range(b - len(bonds))]
    feats += [("bond", t) for t in bonds]
    feats += [("angle", draw(3, _ok_angle)) for _ in range(a)]
    feats += [("dihedral", draw(4, _ok_dihedral)) for _ in range(d)]
    s.feats = feats
    used = {i for _, atoms in feats for i in atoms} | set(s.align or [])
    s.unused = [i for i in range(case.n) if i not in used]
    # output columns of every type, in list order
    s.cols, out = {t: [] for t in TYPES}, 0
    for t, atoms in feats:
        w = 3 * len(atoms) if t == "position" else (2 if t == "dihedral" and not case.angle else 1)
        s.cols[t] += list(range(out, out + w))
        out += w
    s.d_r = out
    s.cols = {t: np.asarray(c) for t, c in s.cols.items() if c}
    gen = torch.Generator().manual_seed(17 * case.B + case.n + sum(case.counts))
    s.g = torch.randn(case.B, s.d_r, generator=gen, dtype=torch.float64)
    s.u = torch.randn(case.B, case.n, 3, generator=gen, dtype=torch.float64)
    s.gk = torch.randn(case.B, case.k, s.d_r, generator=gen, dtype=torch.float32)      # the nets' cotangents of the features metric
    s.a = diag_coeff_for(case.n, 3 + case.seed).astype(np.float32)
    return s


def cotangent(s, t):
    """g [B, d_r] fp64 restricted to the columns of type t (DENSE: all of it)."""
    if t == DENSE:
        return s.g
    g = torch.zeros_like(s.g)
    g[:, s.cols[t]] = s.g[:, s.cols[t]]
    return g


def layer_of(case, dev=None):
    from colvarsfinder import pp
    s = build(case)
    if case.kind == "feat":
        layer = pp.AlignFeatureLayer(case.n, None, None, s.feats, case.angle)
    else:
        layer = pp.AlignFeatureLayer(case.n, s.align, s.ref[s.align], s.feats, case.angle, align_weights=s.aw, weights_any_size=True)
    return layer if dev is None else layer.to(dev)


@functools.lru_cache(maxsize=None)
def counts(case):
    """(n_coord, n_rec, d_r, n_align, n_slot, n_ref) of the case's layer."""
    layer = layer_of(case)
    assert layer.d_r == build(case).d_r, case.id
    assert case.kind == "small" or layer.derivative_table_limits() is None, case.id      # (the small-frame kernels read rec, not mrec)
    return 3 * case.n, layer.rec.shape[0], layer.d_r, layer.align_idx.numel(), layer._n_slot, layer._n_ref


def host_desc(case):
    """cvf_pp_desc with the counts and flags of the case's layer and NULL tables (align_w: a non-NULL token when weighted) - all
    that cvf_align_feature_deriv_route reads."""
    from colvarsfinder import _hip
    layer = layer_of(case)
    d = _hip.PPDesc()
    d.mode = _hip.PP_ALIGN if layer.aligned else _hip.PP_FEATURES
    d.n_coord, d.n_align, d.n_rec = 3 * layer.n_atoms, layer.align_idx.numel(), layer.rec.shape[0]
    d.d_r, d.use_angle_value, d.flags = layer.d_r, int(layer.use_angle_value), layer._flags
    d.has_position = 1
    d.n_slot, d.n_rec_slot, d.n_mrec, d.n_ref = layer._n_slot, layer._n_rec_slot, layer.mrec.shape[0], layer._n_ref
    d.align_w = 64 if layer.align_w is not None else None
    return d


def expected_plan(case, which, k=None, aligned16=True, B=None):
    """The fields of cvf_deriv_plan the mirrors predict."""
    k, B = (k or case.k), (B or case.B)
    nc, n_rec, d_r, nal, n_slot, n_ref = counts(case)
    P = dict(family=0, tables_lds=0, q_lds=0, u_lds=0, weighted=int(case.weighted), vec4=0, lg=0, rows_per_launch=1, launches=1,
             lds_bytes=0, grid=0)
    if case.kind == "feat":
        bpf, budget, u, rpl = feat_bytes(which, n_slot, n_ref, k)
        lg, lds = feat_plan(bpf, budget)
        P.update(family=FEATURES, u_lds=u, lg=lg, rows_per_launch=rpl, lds_bytes=lds, grid=n_tiles(B) * (TILE >> lg))
    elif case.kind == "small":
        P.update(family=SMALL, grid=n_tiles(B))
        if which == VJP:
            P["tables_lds"], P["lds_bytes"] = vjp_small(nc, n_rec, nal)
        elif which == VJP_ROWS:
            P["tables_lds"], P["rows_per_launch"], P["lds_bytes"] = rows_small(nc, n_rec, nal, k)
        elif which == JVP:
            P["tables_lds"], P["q_lds"], P["lds_bytes"] = jvp_small(nc, d_r, n_rec, nal)
        else:
            P["tables_lds"], P["lds_bytes"] = hvp_small(nc, n_rec, nal)
    else:
        P.update(family=LARGE, grid=B, vec4=int(nc % 4 == 0 and aligned16 and which != JVP))
        if which == VJP_ROWS:
            P["rows_per_launch"], P["launches"], P["lds_bytes"] = rows_large(n_ref, k)
        elif which != JVP:
            P["lds_bytes"] = 12 * n_ref
    return P


def instances(case):
    """{(kernel, template arguments)} the case's runs launch, from the mirrors."""
    out = set()
    for run in case.runs:
        which = WHICH[run]
        for al in ((True, False) if case.id in MISALIGNED and run != "jvp" else (True,)):
            P = expected_plan(case, which, aligned16=al)
            w = "weighted_" if case.weighted else ""
            if case.kind == "feat":
                out.add((f"features_{'vjp' if run == 'rows' else run}_kernel", ()))
            elif case.kind == "small":
                out.add({VJP: ("vjp_align_kernel", (P["tables_lds"],)), VJP_ROWS: ("vjp_rows_small_kernel", (P["tables_lds"],)),
                         JVP: ("jvp_align_kernel", (P["tables_lds"], P["q_lds"])), HVP: ("hvp_align_kernel", (P["tables_lds"],))}[which])
            else:
                out.add({VJP: (f"vjp_{w}large_kernel", (P["vec4"],)), VJP_ROWS: (f"vjp_rows_{w}large_kernel", (P["vec4"],)),
                         JVP: ("jvp_large_kernel", (int(case.weighted),)), HVP: ("hvp_large_kernel", (int(case.weighted),))}[which])
    return out


# ------------------------------------------------------------------------------------------------ references
def _oracle(case, feats, dtype):
    from oracle.pp import AlignFeature, features_of
    s = build(case)
    compact = case.n > 64 or len(feats) > 256      # (the oracle's grouped evaluation: the same formulas, a graph of a few dozen nodes)
    if case.kind == "feat":
        return lambda x: features_of(x, feats, case.angle, compact)
    return AlignFeature(s.align, s.ref[s.align], feats, case.angle, align_weights=s.aw, compact=compact)


def _derivs(case, dtype):
    """{quantity: {type: array}} through the oracle in `dtype`: vjp and hvp [B, 3N] per type and dense, jvp [B, d_r]."""
    s = build(case)
    want_h = "hvp" in case.runs
    want_g = want_h or "vjp" in case.runs or "rows" in case.runs
    out = {"vjp": {}, "hvp": {}, "jvp": None, "fwd": None, "metric": None}
    torch.set_default_dtype(dtype)   # (the oracle's buffers take the default type when it is built)
    try:
        x = torch.tensor(s.traj, dtype=dtype)
        u = s.u.to(dtype)
        for t in ([DENSE] + list(s.cols) if want_g else []):
            feats = s.feats if t == DENSE else [f for f in s.feats if f[0] == t]
            g = (s.g if t == DENSE else s.g[:, s.cols[t]]).to(dtype)
            f = _oracle(case, feats, dtype)
            if want_h and not (case.kind == "feat" and t == "position"):
                gx, h = double_backward(f, x, g, u)
                out["hvp"][t] = h.double().reshape(case.B, -1).numpy()
            else:
                xr = x.clone().requires_grad_(True)
                (gx,) = torch.autograd.grad(f(xr), xr, g)
                if want_h:                              # a position record without alignment is a copy: no curvature
                    out["hvp"][t] = np.zeros((case.B, 3 * case.n))
            out["vjp"][t] = gx.double().reshape(case.B, -1).numpy()
        f = _oracle(case, s.feats, dtype)
        if "jvp" in case.runs:
            with fwAD.dual_level():
                out["jvp"] = fwAD.unpack_dual(f(fwAD.make_dual(x, u))).tangent.double().numpy().copy()
        if "fwd" in case.runs:
            out["fwd"] = f(x).double().numpy()
        if "metric" in case.runs:                       # per net: u = J^T g, E = sum a u^2, q = J (a u)  (tests/metric_cases.py)
            a = torch.tensor(s.a, dtype=dtype).reshape(1, case.n, 3)
            qs, Es = [], []
            for i in range(case.k):
                xr = x.clone().requires_grad_(True)
                (ui,) = torch.autograd.grad(f(xr), xr, s.gk[:, i].to(dtype))
                Es.append((a * ui * ui).sum(dim=(1, 2)).double().numpy())
                with fwAD.dual_level():
                    qs.append(fwAD.unpack_dual(f(fwAD.make_dual(x, (a * ui).detach()))).tangent.double().numpy().copy())
            out["metric"] = (np.stack(qs, axis=1), np.stack(Es, axis=1))
    finally:
        torch.set_default_dtype(torch.float32)
    return out


def type_errors(s, got, want):
    """{type: worst-frame error} of a [B, d_r] output, its columns grouped by type."""
    return {t: float(frame_errors(np.asarray(got)[:, c], want[:, c]).max()) for t, c in s.cols.items()}


def metric_q_errors(q, q_ref):
    """e_f of every (frame, net): [B, k]."""
    return np.abs(np.asarray(q, dtype=np.float64) - q_ref).max(axis=2) / np.abs(q_ref).max(axis=2)


def exact_zero(case, q, t):
    """The quantity is exactly 0 (and must come out so): the curvature of the position records of a layer without alignment."""
    return case.kind == "feat" and q == "hvp" and t == "position"


Ref = namedtuple("Ref", "ref twin bar")


@functools.lru_cache(maxsize=None)
def reference(case):
    """ref[quantity]: the fp64 arrays ({type: [B, 3N]} for vjp and hvp, [B, d_r] for jvp and fwd); twin[quantity][type]: the fp32
    twin's worst-frame error; bar[quantity][type] = max(FLOOR, TWIN_MARGIN x twin)."""
    s = build(case)
    r64, r32 = _derivs(case, torch.float64), _derivs(case, torch.float32)
    twin = {}
    for q in ("vjp", "hvp"):
        if not r64[q]:
            continue
        total = sum(r64[q][t] for t in s.cols)
        assert np.abs(total - r64[q][DENSE]).max() <= 1e-10 * np.abs(r64[q][DENSE]).max(), (case.id, q, "the types do not add up")
        for t, v in r64[q].items():
            assert np.isfinite(v).all() and ((np.abs(v).max(axis=1) > 0).all() or exact_zero(case, q, t)), (case.id, q, t)
            v.setflags(write=False)
        twin[q] = {t: 0.0 if exact_zero(case, q, t) else float(frame_errors(r32[q][t], r64[q][t]).max()) for t in r64[q]}
    for q in ("jvp", "fwd"):
        if r64[q] is not None:
            assert np.isfinite(r64[q]).all(), (case.id, q)
            r64[q].setflags(write=False)
            twin[q] = type_errors(s, r32[q], r64[q])
    if r64["metric"] is not None:
        (q, E), (q32, E32) = r64["metric"], r32["metric"]
        assert np.isfinite(q).all() and (E > 0).all() and (np.abs(q).max(axis=2) > 0).all(), case.id
        twin["metric"] = {"q": float(metric_q_errors(q32, q).max()), "E": float((np.abs(E32 - E) / E).max())}
    bar = {q: {t: bar_of(e) for t, e in d.items()} for q, d in twin.items()}
    return Ref(r64, twin, bar)


# ------------------------------------------------------------------------------------------------ the C ABI
def abi_route(desc, B, which, k=1, aligned16=True):
    """(return code, the fields of cvf_align_feature_deriv_route's plan as a dict)."""
    from colvarsfinder import _hip
    plan = _hip.DerivPlan()
    rc = _hip.lib().cvf_align_feature_deriv_route(C.byref(desc), B, which, k, int(aligned16), C.byref(plan))
    return rc, {name: getattr(plan, name) for name, _ in plan._fields_ if name != "reserved"}


def abi_prepare(case, dev):
    """The layer on the device, its descriptor, x and - aligned layers - the aux rows of one cvf_align_feature_fwd call."""
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    s = build(case)
    p = types.SimpleNamespace(case=case, s=s, B=case.B, layer=layer_of(case, dev), dev=dev)
    p.x = torch.tensor(s.traj).to(dev).contiguous()
    p.desc = p.layer.pp_desc()
    p.feat = torch.full((case.B, p.layer.d_r), float("nan"), device=dev)
    p.aux = torch.zeros(n_tiles(case.B), _hip.AUX_ROWS, TILE, device=dev) if p.layer.aligned else None
    _hip.check(lib.cvf_align_feature_fwd(p.desc, P(p.x), case.B, None, P(p.feat), P(p.aux), P(_hip.align_scratch(p.desc, case.B, dev)),
                                         _hip.stream()), "cvf_align_feature_fwd")
    torch.cuda.synchronize()
    return p


def _out(p, shape, misaligned):
    """An output of `shape` that starts as NaN; misaligned: 4 bytes past a 16-byte boundary."""
    n = int(np.prod(shape))
    buf = torch.full((n + 4,), float("nan"), device=p.dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + n] if misaligned else buf[:n]
    assert out.data_ptr() % 16 == (4 if misaligned else 0) and out.is_contiguous()
    return out, shape


def _f32(p, t):
    return t.to(device=p.dev, dtype=torch.float32).contiguous()


def abi_vjp(p, g, misaligned=False):
    from colvarsfinder import _hip
    P = _hip.ptr
    g = _f32(p, g)
    out, shape = _out(p, (p.B, 3 * p.case.n), misaligned)
    _hip.check(_hip.lib().cvf_align_feature_vjp(p.desc, P(p.x), p.B, P(p.aux), P(g), P(out), _hip.stream()), "cvf_align_feature_vjp")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(shape)


def abi_rows(p, g_rows, misaligned=False):
    from colvarsfinder import _hip
    P = _hip.ptr
    g = _f32(p, g_rows)
    k = g.shape[1]
    out, shape = _out(p, (p.B, k, 3 * p.case.n), misaligned)
    _hip.check(_hip.lib().cvf_align_feature_vjp_rows(p.desc, P(p.x), p.B, P(p.aux), k, P(g), P(out), _hip.stream()),
               "cvf_align_feature_vjp_rows")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(shape)


def abi_jvp(p, u):
    from colvarsfinder import _hip
    P = _hip.ptr
    u = _f32(p, u.reshape(p.B, -1))
    out, shape = _out(p, (p.B, p.layer.d_r), False)
    _hip.check(_hip.lib().cvf_align_feature_jvp(p.desc, P(p.x), p.B, P(p.aux), P(u), P(out), _hip.stream()), "cvf_align_feature_jvp")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(shape)


def abi_hvp(p, g, u, misaligned=False):
    from colvarsfinder import _hip
    P = _hip.ptr
    g, u = _f32(p, g), _f32(p, u.reshape(p.B, -1))
    out, shape = _out(p, (p.B, 3 * p.case.n), misaligned)
    _hip.check(_hip.lib().cvf_align_feature_hvp(p.desc, P(p.x), p.B, P(p.aux), P(g), P(u), P(out), _hip.stream()), "cvf_align_feature_hvp")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(shape)


def abi_metric(p, gk):
    """(q [B, k, d_r], E [B, k]) of cvf_metric_apply on a layer without alignment; the outputs start as NaN."""
    from colvarsfinder import _hip
    from tests.metric_cases import from_tiled, to_tiled
    P = _hip.ptr
    k, T = gk.shape[1], n_tiles(p.B)
    gt = torch.tensor(to_tiled(gk.numpy(), p.B)).to(p.dev)
    q = torch.full(tuple(gt.shape), float("nan"), device=p.dev)
    e = torch.full((T, k, TILE), float("nan"), device=p.dev)
    a = torch.tensor(p.s.a, device=p.dev)
    _hip.check(_hip.lib().cvf_metric_apply(p.desc, P(p.x), p.B, None, P(a), k, P(gt), P(q), P(e), None, None, _hip.stream()),
               "cvf_metric_apply")
    torch.cuda.synchronize()
    return from_tiled(q.cpu().numpy(), p.B), from_tiled(e.cpu().numpy()[:, :, None, :], p.B)[:, :, 0]
