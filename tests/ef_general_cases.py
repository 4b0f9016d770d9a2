"""The per-layer eigenfunction step (csrc/ef_general.hip: cvf_ef_general_fwd / _backward and the _shared_ pair): its cases at
the edges of the 64 x 64 core of csrc/cvf_gemm64.hpp, Python mirrors of its host rules, the builders of its inputs, the fp64
reference and the error bars the GPU module holds it to.

Plain Python at import (no torch, no GPU).  `tests/test_ef_general_cases_host.py` (CPU) checks the mirrors against the library,
the edges the table claims, the refusals, and ties the bars to the fp32 CPU oracle; `tests/test_ef_general_edges_gpu.py` runs
every case through the C entries against the fp64 oracle.

A case is (id, dims ending in 1, k, activation, B, mode, n_shared): `mode` "gen" (generator: y, g = dy/dr, the tangent chain
along q and the two-part weight gradient) or "tr" (transfer operator: 2T tiles, the frames and then their lagged partners, a
one-part gradient); `n_shared` None for the plain entries, else the shared-trunk entries (generator mode only).  The C entries
take any chain, so each edge is met at the smallest chain that has it.

Two shapes differ from the smallest imaginable ones, for a reason of the loss and not of the kernels: the one-frame batches are
TWO frames (B = 2).  With one frame the weighted variance of every output is 0 and the loss is 0 / 0 in any arithmetic, fp64
included, so there is nothing to compare; two frames leave the same single ragged tile (62 padded lanes instead of 63) and the
same clamp of the padded lanes' weights.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace

TILE = 64                     # CVF_TILE
MAX_NETS, MAX_LAYERS = 8, 12  # CVF_MAX_NETS, CVF_MAX_LAYERS
MAX_ROWS = 256                # kMaxRows
SLAB_BYTES = 128 << 20        # kSlabBytes
MAX_WIDTH, MAX_D0 = 4096, 65536
KC = 32                       # kKC: the K stage of the layer products
ACTS = ("tanh", "sigmoid", "relu", "elu", "leaky_relu", "softplus")   # CVF_ACT_* 1..6
ALPHA, BETA, LAG, DT = 12.0, 1.2, 2, 0.5

Case = namedtuple("Case", "id dims k act B mode ns")

MANY_B = TILE * MAX_ROWS + 37        # 257 tiles; transfer mode: 514 on 256 rows, row 0 sums tiles 0, 256 (base) and 512 (lagged)
HALF_B = TILE * (MAX_ROWS // 2) + 37  # 129 tiles; transfer mode: 258 on 256 rows, rows 0 and 1 add the lagged tiles 256 and 257
CAP_DIMS, CAP_B = (384, 170, 1), TILE * MAX_ROWS + 5   # k = 2: 131 242 parameters, 255 rows fit 128 MiB; 257 tiles
WIDE_DIMS = (8, 4096, 4096, 1)                         # k = 1: 16 822 273 parameters, one slab row, the widest layer
DEEP_DIMS = (6, 9, 7, 9, 7, 9, 7, 9, 7, 9, 7, 9, 1)    # eleven hidden layers (CVF_MAX_LAYERS - 1), narrow


def _both(id, dims, k, act, B):
    return [Case(f"{id}-{m}", tuple(dims), k, act, B, m, None) for m in ("gen", "tr")]


CASES = (
    # ---- a hidden width as M (64-row block) and as K (32-deep stage), every activation; chains of two hidden layers have
    #      sigma' in the operand load AND sigma' / sigma'' in the epilogue of the adjoint product, chains of one the former only
    _both("w1", [3, 1, 1], 1, "tanh", 2)
    + _both("w31", [67, 31, 1], 2, "sigmoid", 63)
    + _both("w32", [67, 32, 1], 2, "relu", 64)
    + _both("w33", [3, 33, 1], 2, "elu", 65)
    + _both("w63-31", [67, 63, 31, 1], 2, "softplus", 130)
    + _both("w64-64", [67, 64, 64, 1], 2, "leaky_relu", 257)
    + _both("w65-d0-1-k8", [1, 65, 1], MAX_NETS, "tanh", 130)
    + _both("unequal", [7, 130, 5, 70, 1], 2, "tanh", 130)
    # ---- a width as Ki of the weight gradient with the bias column Ki + 1 across a 64-column block; d0 as M of the transposed
    #      g product and as K of layer 0
    + _both("ki-63-64-63", [63, 64, 63, 1], 2, "tanh", 70)
    + _both("ki-64-63-64", [64, 63, 64, 1], 2, "sigmoid", 130)
    + _both("ki-65-65", [65, 65, 1], 2, "softplus", 65)
    + _both("ki-31-33-32", [31, 33, 32, 1], 2, "relu", 63)
    + _both("ki-32-31-33", [32, 31, 33, 1], 2, "leaky_relu", 64)
    + _both("d0-384", [384, 65, 33, 1], 2, "elu", 65)
    + _both("d0-384-B-2", [384, 65, 33, 1], 2, "tanh", 2)
    # ---- depth (one hidden layer: above)
    + _both("deep11", DEEP_DIMS, 1, "tanh", 130)
    # ---- more tiles than slab rows
    + [Case("many-tiles-gen", (3, 5, 1), 2, "tanh", MANY_B, "gen", None),
       Case("lagged-wrap-tr", (3, 5, 1), 2, "tanh", HALF_B, "tr", None),
       Case("many-tiles-tr", (3, 5, 1), 2, "tanh", MANY_B, "tr", None)]
    # ---- the other two branches of the slab-row rule
    + [Case("slab-capped-gen", CAP_DIMS, 2, "tanh", CAP_B, "gen", None),
       Case("one-row-4096-gen", WIDE_DIMS, 1, "tanh", 130, "gen", None)]
    # ---- a shared trunk on wide inputs (generator mode: transfer mode is not built for it)
    + [Case("shared-1-of-2", (65, 64, 33, 1), 3, "tanh", 70, "gen", 1),
       Case("shared-all", (33, 63, 65, 1), 2, "softplus", 130, "gen", 2)]
)
CASES = tuple(CASES)
BY_ID = {c.id: c for c in CASES}
# the small two-tile ragged chain of the once-only checks (same bits twice; garbage in the padded lanes)
RAGGED = {"gen": BY_ID["ki-63-64-63-gen"], "tr": BY_ID["ki-63-64-63-tr"]}


def group(case):
    """The group whose bars the case is held to: mode x (B < 1000 | B >= 1000), the eleven-layer chain on its own."""
    return case.mode, "deep" if case.dims == DEEP_DIMS else "small" if case.B < 1000 else "large"


# ---------------------------------------------------------------------------------------------------- the host's rules
def n_tiles(B):
    return (B + TILE - 1) // TILE


def step_tiles(case):
    """Tiles of a step: T in generator mode, 2T (the frames, then their lagged partners) in transfer mode."""
    return n_tiles(case.B) * (2 if case.mode == "tr" else 1)


def n_params(dims, k, ns=None):
    size = [dims[l + 1] * (dims[l] + 1) for l in range(len(dims) - 1)]
    return sum(size[:ns or 0]) + k * sum(size[ns or 0:])


def g64_rows(n_par, tiles):
    """g64_rows (csrc/cvf_gemm64.hpp): min(tiles, 256, 128 MiB / (4 n_params)), at least 1."""
    return max(1, min(tiles, MAX_ROWS, SLAB_BYTES // (4 * max(n_par, 1))))


def row_tiles(rho, tiles, rows):
    """The tiles slab row rho sums, in order (efg_wgrad_kernel)."""
    return list(range(rho, tiles, rows))


def efg_layout(dims, k, tiles, gen, ns=None):
    """efg_layout (csrc/ef_general.hip): offsets, in floats, of the images of `saved`, and their total.  Generator mode: h_l per
    hidden layer (a shared layer's once, not per net), then u_l and zdot_l per hidden layer, alpha, gamma; transfer mode: h_l, two
    images as wide as the widest hidden layer, alpha."""
    NH, per, pos = len(dims) - 2, tiles * TILE * k, 0
    L = SimpleNamespace(h=[], u=[], z=[], zb=[])
    for l in range(NH):
        L.h.append(pos)
        pos += (per // k if l < (ns or 0) else per) * dims[l + 1]
    if gen:
        for l in range(NH):
            L.u.append(pos)
            pos += per * dims[l + 1]
            L.z.append(pos)
            pos += per * dims[l + 1]
    else:
        for _ in range(2):
            L.zb.append(pos)
            pos += per * max(dims[1:-1])
    L.alpha, pos = pos, pos + per
    L.gamma, pos = pos, pos + (per if gen else 0)
    L.total = pos
    return L


def efg_why(dims, k, acts, n_par=None, n_layers=None):
    """efg_why (csrc/ef_general.hip) for nets laid out net by net over a flat buffer of `n_par` parameters: None, or the
    reason the library gives.  `acts`: one code per Linear layer; `n_layers` overrides len(dims) - 1 (a description past what
    `dims` can hold)."""
    L = len(dims) - 1 if n_layers is None else n_layers
    if not 1 <= k <= MAX_NETS:
        return f"{k} nets: 1 to {MAX_NETS} are supported"
    if not 2 <= L <= MAX_LAYERS:
        return f"{L - 1} hidden layers: 1 to {MAX_LAYERS - 1} are supported"
    if dims[L] != 1:
        return "the nets' output must be a scalar"
    if not 1 <= dims[0] <= MAX_D0:
        return f"{dims[0]} input features: 1 to {MAX_D0} are supported"
    for l in range(1, L):
        if not 1 <= dims[l] <= MAX_WIDTH:
            return f"hidden layer {l} is {dims[l]} wide: 1 to {MAX_WIDTH} units are supported"
    if any(not 0 <= a <= 6 for a in acts[:L]):
        return "an activation code outside include/cvf.h"
    if n_par is not None and n_par != n_params(dims, k):
        return "the flat buffer holds parameters outside the nets"
    return "an activation after the output layer" if acts[L - 1] != 0 else None


def act_codes(case):
    return [ACTS.index(case.act) + 1] * (len(case.dims) - 2) + [0]


# ---------------------------------------------------------------------------------------------------- inputs
def _act_fn(name):
    import torch
    import torch.nn.functional as F
    return {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu, "elu": F.elu, "leaky_relu": F.leaky_relu,
            "softplus": F.softplus}[name]


def eig_w(k):
    return [1.0 - 0.1 * i for i in range(k)]


# The parameters are torch's default init, U(-1/sqrt(in), 1/sqrt(in)), with the WEIGHTS TIMES TWO.  The default init shrinks the
# signal by about sqrt(3) per layer (more behind a sigmoid or a 5-wide layer): the outputs of the eleven-layer chain vary in
# their seventh digit, those of the sigmoid chains in their third, and the weighted variance of the outputs - the denominator of
# every eigenvalue - loses those digits in ANY fp32 evaluation, the CPU oracle's included (its own loss then misses the project's
# ceilings).  Twice the weights keep the variation at the size of the outputs; four times behind a sigmoid, whose outputs are all
# positive, so that the next layer sees a constant with a small variation on it.  The rule looks at the activation alone.
GAIN, GAIN_SIGMOID = 2.0, 4.0


@functools.lru_cache(maxsize=None)
def inputs(case):
    """CPU, fp32: the state dict (torch's default init; with a shared trunk net 0's first `ns` layers stand for every net's),
    features X [B][d0], weights w, the metric's diagonal a; in transfer mode the lagged partners X_lag - independent random
    frames - and their weights w_lag != w."""
    import torch
    from oracle import nnref
    g = torch.Generator().manual_seed(4200 + 13 * CASES.index(case))
    sd = nnref.init_eigenfunctions(list(case.dims), case.k, g)
    gain = GAIN_SIGMOID if case.act == "sigmoid" else GAIN
    sd = {n: (p * gain if n.endswith("weight") else p) for n, p in sd.items()}
    d0 = case.dims[0]
    inp = SimpleNamespace(sd=sd, X=torch.randn(case.B, d0, generator=g), w=torch.rand(case.B, generator=g) + 0.5,
                          a=torch.rand(d0, generator=g) + 0.5, X_lag=None, w_lag=None)
    if case.mode == "tr":
        inp.X_lag, inp.w_lag = torch.randn(case.B, d0, generator=g), torch.rand(case.B, generator=g) + 0.5
    return inp


def flat(sd, dims, k, ns=None):
    """The flat vector in the layout of core._SharedTrunkFlat: the shared layers once (net 0's), then net by net the rest, each
    layer's weights and then its bias.  ns None / 0: the plain layout."""
    import torch
    L, ns = len(dims) - 1, ns or 0
    out = [sd[f"eigen_funcs.0.{l + 1}.{n}"].reshape(-1) for l in range(ns) for n in ("weight", "bias")]
    for i in range(k):
        out += [sd[f"eigen_funcs.{i}.{l + 1}.{n}"].reshape(-1) for l in range(ns, L) for n in ("weight", "bias")]
    return torch.cat(out)


def tile_rows(X):
    """[B][d] rows -> the tiled layout [T][d][64] (flattened), zero in the padded lanes of the last tile."""
    import torch
    B, d = X.shape
    T = n_tiles(B)
    P = torch.zeros(T * TILE, d, dtype=X.dtype)
    P[:B] = X
    return P.reshape(T, TILE, d).permute(0, 2, 1).contiguous().reshape(-1)


def feat_tiled(case, inp=None):
    """feat_tiled of a step: [T][d0][64], in transfer mode [2T][d0][64] - the frames' tiles, then their lagged partners'."""
    import torch
    inp = inputs(case) if inp is None else inp
    t = tile_rows(inp.X)
    return t if case.mode == "gen" else torch.cat([t, tile_rows(inp.X_lag)])


def untile(t, *inner):
    """A tiled tensor [tiles][*inner][64] -> rows [tiles * 64][*inner]: the valid frames of pass p are rows p T 64 .. + B."""
    n = len(inner)
    return t.reshape(-1, *inner, TILE).permute(0, n + 1, *range(1, n + 1)).reshape(-1, *inner)


def valid_rows(case):
    """Row indices (after `untile`) of the valid frames of y_tiled: B, or in transfer mode B of each pass."""
    rows = list(range(case.B))
    return rows if case.mode == "gen" else rows + [n_tiles(case.B) * TILE + r for r in range(case.B)]


# ---------------------------------------------------------------------------------------------------- the reference
def oracle(case, dtype):
    """oracle.losses.ef_loss on the identity preprocessing in `dtype`, on the CPU: dict of numpy fp64 arrays - y [B or 2B][k]
    (the frames, then their lagged partners), g = dy/dr [B][k][d0] (generator mode), lv = [loss, npl, pen], eig (sorted), cvec,
    grad (flat, the layout of `flat`; shared layers are the SAME leaves for every net, so autograd sums their gradients)."""
    import numpy as np
    import torch
    from oracle import losses, nnref
    inp, k, ns, act = inputs(case), case.k, case.ns or 0, _act_fn(case.act)
    torch.set_default_dtype(dtype)
    try:
        sd = {n: p.detach().to(dtype).clone().requires_grad_(True) for n, p in inp.sd.items()}
        for i in range(1, k):
            for l in range(ns):
                for n in ("weight", "bias"):
                    sd[f"eigen_funcs.{i}.{l + 1}.{n}"] = sd[f"eigen_funcs.0.{l + 1}.{n}"]
        w = inp.w.to(dtype)
        if case.mode == "gen":
            X = inp.X.to(dtype).requires_grad_(True)
            y = nnref.eigenfunctions_forward(sd, k, X, act)
            g = torch.stack([torch.autograd.grad(y[:, i].sum(), X, retain_graph=i + 1 < k)[0] for i in range(k)], dim=1)
            lo, eo, no, po, co = losses.ef_loss(sd, k, lambda x: x, X, w, alpha=ALPHA, eig_w=eig_w(k), diag_coeff=inp.a.to(dtype),
                                                beta=BETA, activation=act)
        else:
            X, Xl, g = inp.X.to(dtype), inp.X_lag.to(dtype), None
            with torch.no_grad():
                y = nnref.eigenfunctions_forward(sd, k, torch.cat([X, Xl]), act)
            lo, eo, no, po, co = losses.ef_loss(sd, k, lambda x: x, X, w, Xl, inp.w_lag.to(dtype), alpha=ALPHA, eig_w=eig_w(k),
                                                lag_idx=LAG, dt=DT, activation=act)
        lo.backward()
        grad = flat({n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in sd.items()}, case.dims, k, ns)
    finally:
        torch.set_default_dtype(torch.float32)
    return dict(y=y.detach().double().numpy(), g=None if g is None else g.detach().double().numpy(),
                lv=np.asarray([float(v.detach()) for v in (lo, no, po)]), eig=eo.double().numpy(), cvec=[int(c) for c in co],
                grad=grad.double().numpy())


@functools.lru_cache(maxsize=None)
def reference(case):
    """The fp64 oracle of a case: computed once, shared by every test that needs it, never modified."""
    return oracle(case, __import__("torch").float64)


QUANTITIES = ("y", "g", "loss", "eig", "grad")


def errors(got, want):
    """Distances of a result from the fp64 one: y and g (generator mode) as largest entry error over the largest entry, the loss
    vector and the eigenvalues relative, the gradient as largest entry error over the largest entry."""
    import numpy as np
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)))     # noqa: E731
    big = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())                      # noqa: E731
    e = dict(y=big(got["y"], want["y"]), loss=rel(got["lv"], want["lv"]), eig=rel(got["eig"], want["eig"]),
             grad=big(got["grad"], want["grad"]))
    if want["g"] is not None:
        e["g"] = big(got["g"], want["g"])
    return e


@functools.lru_cache(maxsize=None)
def e32(case):
    """The distances of the fp32 CPU evaluation of the oracle from its fp64 evaluation: the source of the bars."""
    import torch
    return errors(oracle(case, torch.float32), reference(case))


def group_e32(cases=None):
    """{group: {quantity: worst e32 over the group's cases}}."""
    worst = {}
    for c in CASES if cases is None else cases:
        w = worst.setdefault(group(c), {})
        for q, v in e32(c).items():
            w[q] = max(w.get(q, 0.0), v)
    return worst


# ---------------------------------------------------------------------------------------------------- error bars
# The project's ceilings - conditions, not measurements: 1e-4 for the loss and the eigenvalues (and for y, of which they are
# sums), 3e-4 for the gradient (and for g = dy/dr, a gradient too).  Every bar below must stay under its ceiling.
CEILING = dict(y=1e-4, g=3e-4, loss=1e-4, eig=1e-4, grad=3e-4)

# group -> quantity -> bar: EIGHT TIMES the worst distance of the fp32 CPU oracle (`oracle(case, torch.float32)`: torch's own fp32
# kernels on the CPU) from the fp64 oracle over the group's cases, rounded up to two digits - the rule of ae_general_cases.BARS,
# measured against the reference, never against the kernels; the factor 8 covers the different summation order of the MFMA
# path.  tests/test_ef_general_cases_host.py recomputes the maxima and holds every bar between 4 and 16 times its source, and
# under its ceiling.
BARS = {
    ("gen", "small"): dict(y=6.1e-06, g=6.4e-06, loss=1.3e-05, eig=1.1e-05, grad=2.6e-05),
    ("gen", "large"): dict(y=2.6e-06, g=5.9e-06, loss=1.7e-06, eig=2.2e-06, grad=4.5e-06),
    ("gen", "deep"): dict(y=3.7e-06, g=2.2e-06, loss=6.0e-07, eig=3.3e-07, grad=6.7e-06),
    ("tr", "small"): dict(y=4.5e-06, loss=2.5e-05, eig=3.3e-05, grad=3.5e-05),
    ("tr", "large"): dict(y=1.2e-06, loss=1.3e-06, eig=9.2e-07, grad=1.6e-06),
    ("tr", "deep"): dict(y=2.7e-06, loss=5.1e-05, eig=5.1e-05, grad=1.7e-04),
}
