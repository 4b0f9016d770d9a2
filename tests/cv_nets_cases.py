"""The nets' part of a CV and of its Jacobian on per-layer HIP kernels (csrc/cv_nets.hip, cvf_cv_nets_*): the cases, an fp64 and
an fp32 CPU evaluation of (xi, G = d xi / d r) by plain torch, the Python mirror of the scratch formula and the error bars.

Plain Python at import (no torch, no GPU).  `tests/test_cv_nets_host.py` (CPU) checks the mirror and the refusals against the
library and ties the bars to the fp32 evaluation; `tests/test_cv_nets_gpu.py` runs every case through the C ABI.

The shapes are the smallest at which the kernels can still go wrong: cvn_layer_kernel works on 64-row blocks of the A operand and
32-deep K stages on 16 x 16 x 4 matrix tiles over 64-frame tiles; the sweep's first launch forms its B operand from the seed row,
the middle ones ping-pong between two images (three layers or more), the last one writes g; a one-layer chain has no product at
all (cvn_linear_kernel).
"""
import collections
import contextlib
import functools

TILE, MAX_NETS, MAX_LAYERS, MAX_WIDTH, MAX_D0, MAX_VALUES_K = 64, 8, 12, 4096, 65536, 4096
ACTS = ("tanh", "sigmoid", "relu", "elu", "leaky_relu", "softplus")   # codes 1..6 of include/cvf.h

# form "A": `nets` scalar chains of `dims` side by side (EigenFunctions); form "B": the first `upto` layers of one chain `dims`.
# layout "own": the evaluated chains fill the flat buffer; "ae": nn.mlp_layout of AutoEncoder(dims[:upto + 1], dims[upto:]).
Case = collections.namedtuple("Case", "id form dims nets upto act B layout want_g")


def _a(name, dims, k, B=70, act="tanh"):
    return Case(f"A-{name}-k{k}-B{B}", "A", tuple(dims), k, len(dims) - 1, act, B, "own", True)


def _b(name, dims, B=70, upto=None, layout="own", want_g=True):
    return Case(f"B-{name}-B{B}", "B", tuple(dims), 1, len(dims) - 1 if upto is None else upto, "tanh", B, layout, want_g)


EDGE_B = (1, 63, 64, 65, 130)      # one frame, either side of a full tile, two tiles and a tail
DEEP = [6] + [4] * 11 + [1]        # CVF_MAX_LAYERS layers: eleven hidden layers of 4 units

CASES = (
    # ---- form A.  [5,3,1]: everything narrower than one matrix tile, at every batch edge (k = 3)
    [_a("tiny", [5, 3, 1], 3, B) for B in EDGE_B] + [_a("tiny", [5, 3, 1], k) for k in (1, 8)]
    + [_a(name, dims, k) for name, dims in (("config3", [66, 20, 20, 20, 1]),
                                            ("straddle", [30, 65, 33, 1]),    # either side of the 64-row block and the 32-deep stage
                                            ("wide-one-hidden", [7, 130, 1]),
                                            ("twelve-layers", DEEP)) for k in (1, 3, 8)]
    + [_a(f"act-{act}", [9, 12, 12, 1], 3, act=act) for act in ACTS]
    # ---- form B
    + [_b("small", [6, 8, 2], B) for B in EDGE_B]
    + [_b("straddle", [30, 65, 33, 3]), _b("single-linear", [9, 4]), _b("k8", [12, 16, 8]), _b("wide", [64, 4096, 2]),
       _b("ae-encoder", [10, 16, 2, 16, 10], upto=2, layout="ae"),
       _b("values-k100", [20, 32, 100], want_g=False)]
)


def k_of(c):
    return c.nets if c.form == "A" else c.dims[c.upto]


def acts(c):
    """cvf_mlp_desc.act: the case's activation after every layer but a chain's last (for "ae": the encoder's and the decoder's)."""
    code, L = ACTS.index(c.act) + 1, len(c.dims) - 1
    return [0 if l in (c.upto - 1, L - 1) else code for l in range(L)]


def layout(c):
    """(w_off, b_off) per chain and layer, n_params: chain after chain, per layer weight [out, in] then bias - which is also
    model.parameters() order of an AutoEncoder's encoder followed by its decoder."""
    w_off, b_off, pos = [], [], 0
    for _ in range(c.nets):
        w_off.append([])
        b_off.append([])
        for l in range(len(c.dims) - 1):
            w_off[-1].append(pos)
            pos += c.dims[l] * c.dims[l + 1]
            b_off[-1].append(pos)
            pos += c.dims[l + 1]
    return w_off, b_off, pos


def mlp_desc(c):
    from colvarsfinder import _hip
    m, (w_off, b_off, n) = _hip.MLPDesc(), layout(c)
    m.n_nets, m.n_layers, m.n_params = c.nets, len(c.dims) - 1, n
    for l, a in enumerate(acts(c)):
        m.dims[l], m.dims[l + 1], m.act[l] = c.dims[l], c.dims[l + 1], a
    for i in range(c.nets):
        for l in range(m.n_layers):
            m.w_off[i][l], m.b_off[i][l] = w_off[i][l], b_off[i][l]
    return m


# ---------------------------------------------------------------------------------------------------- the host's rules
def n_tiles(B):
    return (B + TILE - 1) // TILE


def scratch_floats(c, B=None, want_g=None):
    """cvn_layout: the tiled features, a_1..a_upto per chain, and for g on chains of three layers or more two images of v_l per CV
    as wide as the widest of dims[1..upto-2]."""
    B, want_g = c.B if B is None else B, c.want_g if want_g is None else want_g
    d, L = c.dims, c.upto
    rows = d[0] + c.nets * sum(d[1:L + 1])
    if want_g and L >= 3:
        rows += 2 * k_of(c) * max(d[1:L - 1])
    return n_tiles(B) * TILE * rows


# ---------------------------------------------------------------------------------------------------- inputs and evaluations
@functools.lru_cache(maxsize=None)
def inputs(c):
    """(theta [n_params] fp32, features [B, d0] fp32) as numpy arrays: torch.nn.Linear's initialisation (an AutoEncoder's own for
    the "ae" layout), standard normal features."""
    import zlib
    import torch
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()) % 100_000)
    if c.layout == "ae":
        import __graft_entry__  # noqa: F401  (puts the package on sys.path)
        from colvarsfinder import nn
        rng = torch.get_rng_state()
        torch.manual_seed(g.initial_seed())
        model = nn.AutoEncoder(list(c.dims[:c.upto + 1]), list(c.dims[c.upto:]))
        torch.set_rng_state(rng)
        lay = nn.mlp_layout(model)
        w_off, b_off, n = layout(c)
        assert lay["n_params"] == n and [(w, b) for w, b, *_ in lay["nets"][0]] == list(zip(w_off[0], b_off[0]))
        theta = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    else:
        w_off, b_off, n = layout(c)
        theta = torch.empty(n)
        for i in range(c.nets):
            for l in range(len(c.dims) - 1):
                bound = c.dims[l] ** -0.5
                nw, nb = c.dims[l] * c.dims[l + 1], c.dims[l + 1]
                theta[w_off[i][l]:w_off[i][l] + nw] = (2 * torch.rand(nw, generator=g) - 1) * bound
                theta[b_off[i][l]:b_off[i][l] + nb] = (2 * torch.rand(nb, generator=g) - 1) * bound
    feats = torch.randn(c.B, c.dims[0], generator=g)
    return theta.numpy().copy(), feats.numpy().copy()


def _act_fn(name, code):
    import torch
    from tests import ae_inputs as I
    if code == 0:
        return lambda x: x
    # evaluated in fp64 and rounded to the argument's precision (ae_inputs._rounded_tanh: torch's fp32 vector functions differ in
    # their last digit between instruction sets)
    return lambda x: I.ACT_FN[name](x.double()).to(x.dtype)


def evaluate(c, dtype):
    """(xi [B, k], G [B, k, d0] or None for a values-only case) of the case in `dtype` by plain torch on the CPU, as float64 numpy
    arrays: Linear layers and activations as torch applies them, G by one autograd.grad per CV (frames are independent)."""
    import torch
    theta, feats = inputs(c)
    th, r = torch.as_tensor(theta).to(dtype), torch.as_tensor(feats).to(dtype).requires_grad_(c.want_g)
    w_off, b_off, _ = layout(c)
    ac, outs = acts(c), []
    for i in range(c.nets):
        h = r
        for l in range(c.upto):
            fin, fout = c.dims[l], c.dims[l + 1]
            W = th[w_off[i][l]:w_off[i][l] + fin * fout].view(fout, fin)
            b = th[b_off[i][l]:b_off[i][l] + fout]
            h = _act_fn(c.act, ac[l])(torch.nn.functional.linear(h, W, b))
        outs.append(h)
    xi = torch.cat(outs, dim=1)
    assert xi.shape == (c.B, k_of(c))
    G = None
    if c.want_g:
        G = torch.stack([torch.autograd.grad(xi[:, i].sum(), r, retain_graph=True)[0] for i in range(k_of(c))], dim=1)
        G = G.double().numpy()
    return xi.detach().double().numpy(), G


@contextlib.contextmanager
def _fixed_order_fp32():
    from tests import regae_general_cases as R
    with R._fixed_order_fp32():
        yield


@functools.lru_cache(maxsize=None)
def reference(c):
    """The fp64 evaluation, computed once per process and shared (callers must not write into it)."""
    import torch
    return evaluate(c, torch.float64)


def rel_err(got, want):
    """tests/test_cv_jacobian_gpu.py: max |got - want| over max |want|."""
    import numpy as np
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


@functools.lru_cache(maxsize=None)
def worst_e32():
    """{"xi", "g"}: the worst distance of the fp32 CPU evaluation (one thread, the Linear layers' sums in a fixed order: the
    setting of regae_general_cases.e32) from the fp64 one over CASES."""
    import torch
    worst = dict(xi=0.0, g=0.0)
    for c in CASES:
        xi64, g64 = reference(c)
        with _fixed_order_fp32():
            xi32, g32 = evaluate(c, torch.float32)
        worst["xi"] = max(worst["xi"], rel_err(xi32, xi64))
        if c.want_g:
            worst["g"] = max(worst["g"], rel_err(g32, g64))
    return worst


BAR_FACTOR = 8   # the factor of regae_general_cases.BARS: the matrix cores sum in another order than the CPU


def bars():
    """{"xi", "g"}: BAR_FACTOR times worst_e32() - derived from the fp32 CPU evaluation where the test runs, never from the kernels."""
    return {term: BAR_FACTOR * e for term, e in worst_e32().items()}
