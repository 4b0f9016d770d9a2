"""Joint 2-D grid bias terms and hill deposition (csrc/cvf_bias.hpp: cvf_bias_term2_eval, cvf_hill_row, cvf_hill_node_add;
csrc/cv_bias_hills.hip): the grids, the bias and the hills written independently in torch fp64 (the reference
of both test files), the stand-alone host program and the bars.  `tests/test_cv_bias2_host.py` (CPU) and
`tests/test_cv_bias2_gpu.py` (GPU) share it; models, frames and the 1-D reference come from `tests/cv_bias_cases.py`.

The reference is written without a look at csrc/cvf_bias.hpp: the bicubic Hermite interpolant as the 4 x 4 quadratic form of the
textbook basis on the clamped point P, its first and mixed derivatives at P by torch autograd (never a coded derivative), the
extension U(P) + d1U d_1 + d2U d_2 + d12U d_1 d_2 outside, and the gradient of the whole by autograd again; the hills as plain
Gaussians in fp64 with their derivatives by autograd.  Everything in fp64 on the fp32 parameters.

The grid is 5 x 4 - not square, so a transposed index shows - with unequal spacings."""
import os
import subprocess

import numpy as np
import torch

from tests import codeobj
from tests import cv_bias_cases as Bc

EPS = float(np.finfo(np.float32).eps)
N1, N2 = 5, 4

# Bars of the GPU tests (metric of tests/cv_bias_cases.rel_rows: max abs error / the reference's max abs over the frames; fp64
# autograd of U(xi(x)) as the reference).  Each is three times the worst case measured on the MI355X over GRID_CASES x the eight
# models of tests/cv_bias_cases, 80 pairs (the project's convention); the kernels have no atomics, so the figures repeat.  Achieved:
# beside each bar and in DESIGN.md section 4.19.
U_TOL = 5.6e-7       # achieved 1.87e-7 (wave-B, above-1); 1.4e-8 .. 1.9e-7 over the 80 (model, case) pairs
DU_TOL = 1.06e-6     # achieved 3.53e-7 (wave-identity, on-node); 8.7e-9 .. 3.5e-7.  Above the 1-D bar (3.6e-7): a slope of the
#                      bicubic goes through two interpolations, and "on-node" has the smallest spacing (inv_h multiplies roundings)
F_TOL = 1.49e-6      # achieved 4.97e-7 (wave-C, above-1); 8.3e-8 .. 5.0e-7 - within the standing bar of the coef form (1.5e-6)
# deposit on the host (test_cv_bias2_host.py): table and heights against fp64, max abs error / the reference's max abs per column of
# the node (U, d1, d2, d12).  A Gaussian in fp32: expf is good to 1 - 2 ulp and its argument, of order 1 near the centre where the
# hill matters, carries a few roundings; each node adds a handful of such terms.  Measured 0.6 - 0.9 eps.
DEP_TOL = 16 * EPS
# deposit on the GPU: three times the worst measured there, which is 2.49 eps (the 33 x 9 grid under 65 hills: 65 roundings per node);
# the 1-D and 5 x 4 cases measure 0.6 - 1.0 eps against fp64, 0.4 - 1.2 eps against the host program, the heights 0.2 - 1.0 eps
DEP_GPU_TOL = 7.5 * EPS

GRID_CASES = ["interior", "below-1", "above-1", "below-2", "above-2", "corner-low", "corner-high", "on-node", "plus-harmonic", "cv-swapped"]


# ------------------------------------------------------------------------------------------------ the bias, independently
def basis(t, h):
    """The textbook cubic Hermite basis on a cell of width h: weights of (f_j, f_{j+1}, f'_j, f'_{j+1})."""
    return torch.stack([(1 + 2 * t) * (1 - t) ** 2, t ** 2 * (3 - 2 * t), t * (1 - t) ** 2 * h, t ** 2 * (t - 1) * h], dim=-1)


def bicubic_at(P, lo, h, nodes):
    """U at points P [M, 2] INSIDE the grid (edges included): nodes [n1, n2, 4] = (U, d1U, d2U, d12U), node (j1, j2) at lo + j h."""
    n = nodes.shape[:2]
    j, t = [], []
    for a in (0, 1):
        pos = lo[a] + torch.arange(n[a], dtype=P.dtype) * h[a]
        ja = torch.clamp(torch.searchsorted(pos, P[:, a].detach().contiguous(), right=True) - 1, 0, n[a] - 2)   # (the last node line: the last cell)
        j.append(ja)
        t.append((P[:, a] - pos[ja]) / h[a])
    bx, by = basis(t[0], h[0]), basis(t[1], h[1])
    U = torch.zeros_like(P[:, 0])
    for a in (0, 1):            # corner (j1 + a, j2 + b); f and its axis-1 slope pair with bx[a], bx[2 + a], likewise along axis 2
        for b in (0, 1):
            c = nodes[j[0] + a, j[1] + b]
            U = U + bx[:, a] * by[:, b] * c[:, 0] + bx[:, 2 + a] * by[:, b] * c[:, 1] + bx[:, a] * by[:, 2 + b] * c[:, 2] \
                + bx[:, 2 + a] * by[:, 2 + b] * c[:, 3]
    return U


def grid_u(x, lo, inv_h, nodes):
    """U at x [M, 2] anywhere, differentiable in x: the bicubic on P = x clamped to the grid, continued by its first and mixed
    derivatives at P (autograd) along d = x - P.  NaN is not handled here."""
    nodes = torch.as_tensor(nodes, dtype=x.dtype)
    h = [1.0 / inv_h[0], 1.0 / inv_h[1]]
    hi = [lo[a] + (nodes.shape[a] - 1) * h[a] for a in (0, 1)]
    if not x.requires_grad:
        x = x.clone().requires_grad_(True)
    P = torch.stack([torch.clamp(x[:, a], lo[a], hi[a]) for a in (0, 1)], dim=1)
    UP = bicubic_at(P, lo, h, nodes)
    g, = torch.autograd.grad(UP.sum(), P, create_graph=True)
    g12 = torch.autograd.grad(g[:, 0].sum(), P, create_graph=True)[0][:, 1]
    d = x - P
    return UP + g[:, 0] * d[:, 0] + g[:, 1] * d[:, 1] + g12 * d[:, 0] * d[:, 1]


def term_nodes(t):
    return np.stack([np.float32(t[key]).astype(np.float64) for key in ("u", "d1", "d2", "d12")], axis=2)


def term_axes(t):
    lo = [Bc.f32(v) for v in t["lo"]]
    inv_h = [Bc.f32(v) for v in t["inv_h"]] if "inv_h" in t else [Bc.f32(1.0 / v) for v in t["h"]]
    return lo, inv_h


def ref_bias2(terms, xi):
    """U [B] of xi [B, k] for term dicts that may hold "table2d" terms; every other kind by tests/cv_bias_cases.ref_bias."""
    U = torch.zeros_like(xi[:, 0])
    for t in terms:
        if t["kind"] == "table2d":
            lo, inv_h = term_axes(t)
            U = U + grid_u(torch.stack([xi[:, t["cv"]], xi[:, t["cv2"]]], dim=1), lo, inv_h, term_nodes(t))
        else:
            U = U + Bc.ref_bias([t], xi)
    return U


def ref_u_du(terms, xi_np):
    """(U [B], dU [B, k]) in fp64, dU by autograd of ref_bias2."""
    xi = torch.tensor(np.asarray(xi_np, dtype=np.float64), requires_grad=True)
    U = ref_bias2(terms, xi)
    dU, = torch.autograd.grad(U.sum(), xi, allow_unused=True)
    return U.detach().numpy(), (torch.zeros_like(xi) if dU is None else dU).numpy()


def reference(mid, nets, frames, terms):
    """(U [B], dU [B, k], force [B, n_coord]) by torch fp64 autograd of U(xi(x)) on the CPU (tests/cv_bias_cases.reference with 2-D terms)."""
    X = torch.tensor(np.asarray(frames), dtype=torch.float64, requires_grad=True)
    xi = Bc.xi_of(mid, nets, X, torch.float64)
    xi.retain_grad()
    U = ref_bias2(terms, xi)
    U.sum().backward()
    return U.detach().numpy(), xi.grad.numpy(), -X.grad.reshape(X.shape[0], -1).numpy()


def smooth_grid(cv, cv2, lo, inv_h, x0, n=(N1, N2)):
    """A "table2d" term whose nodes sample f(x, y) = 1 + sin(x - x0) cos(0.7 (y - y0)) + 0.5 (x - x0) + 0.3 (y - y0) + 0.4 (x - x0)(y - y0):
    values, slopes and the mixed derivative of order 1."""
    lo, inv_h = [np.float32(v) for v in lo], [np.float32(v) for v in inv_h]
    x = (np.float64(lo[0]) + np.arange(n[0]) / np.float64(inv_h[0]) - x0[0])[:, None]
    y = (np.float64(lo[1]) + np.arange(n[1]) / np.float64(inv_h[1]) - x0[1])[None, :]
    return {"kind": "table2d", "cv": cv, "cv2": cv2, "lo": (float(lo[0]), float(lo[1])), "inv_h": (float(inv_h[0]), float(inv_h[1])),
            "u": 1.0 + np.sin(x) * np.cos(0.7 * y) + 0.5 * x + 0.3 * y + 0.4 * x * y,
            "d1": np.cos(x) * np.cos(0.7 * y) + 0.5 + 0.4 * y,
            "d2": -0.7 * np.sin(x) * np.sin(0.7 * y) + 0.3 + 0.4 * x,
            "d12": -0.7 * np.cos(x) * np.sin(0.7 * y) + 0.4 + 0.0 * x * y}


# ------------------------------------------------------------------------------------------------ the hills, independently
def ref_deposit(term, table_nodes, centres, height, sigma, inv_kdt):
    """One deposit call in fp64: (new nodes, hills [B, 4]).  `term` is a "table" or "table2d" dict (for its axes), table_nodes the
    nodes before the call ([n, 2] or [n1, n2, 4], fp64), centres [B] or [B, 2] the fp32 centres.  Every height from the nodes
    BEFORE the call; a non-finite centre gives w = 0 and adds nothing; node positions are the fp32 numbers lo + fp32(j) / inv_h."""
    two_d = term["kind"] == "table2d"
    nodes = np.array(table_nodes, dtype=np.float64)
    c = np.asarray(centres, dtype=np.float64).reshape(len(centres), -1)
    if two_d:
        lo, inv_h = term_axes(term)
        sig = [Bc.f32(sigma[0]), Bc.f32(sigma[1])]
    else:
        lo, inv_h, sig = [Bc.f32(term["lo"])], [Bc.f32(term["inv_h"])], [Bc.f32(sigma)]
    pos = [(np.float32(lo[a]) + np.arange(nodes.shape[a], dtype=np.float32) / np.float32(inv_h[a])).astype(np.float64) for a in range(len(lo))]
    hills = np.zeros((len(c), 4))
    add = torch.zeros(nodes.shape, dtype=torch.float64)
    for b, cb in enumerate(c):
        hills[b, :len(cb)] = cb
        if not np.isfinite(cb).all():
            hills[b, 3] = np.nan
            continue
        x = torch.tensor(cb[None, :])
        if two_d:
            V = float(grid_u(x, lo, inv_h, nodes).detach()[0])
        else:
            V = float(Bc.hermite_u(x[:, 0], lo[0], inv_h[0], nodes[:, 0], nodes[:, 1])[0])
        w = Bc.f32(height) * np.exp(-V * Bc.f32(inv_kdt))
        hills[b, 2:] = w, V
        # the Gaussian and its derivatives on the nodes, by autograd in the node positions
        if two_d:
            X, Y = torch.meshgrid(torch.tensor(pos[0]), torch.tensor(pos[1]), indexing="ij")
            X, Y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
            G = w * torch.exp(-0.5 * ((X - cb[0]) ** 2 / sig[0] ** 2 + (Y - cb[1]) ** 2 / sig[1] ** 2))
            g1, g2 = torch.autograd.grad(G.sum(), (X, Y), create_graph=True)
            g12, = torch.autograd.grad(g1.sum(), Y)
            add = add + torch.stack([G, g1, g2, g12], dim=2).detach()
        else:
            X = torch.tensor(pos[0], requires_grad=True)
            G = w * torch.exp(-0.5 * (X - cb[0]) ** 2 / sig[0] ** 2)
            g1, = torch.autograd.grad(G.sum(), X)
            add = add + torch.stack([G, g1], dim=1).detach()
    return nodes + add.numpy(), hills


def rel_cols(got, want):
    """max abs error / the reference's max abs, per column of the last axis; the largest of them."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    return float(max(np.abs(got[:, c] - want[:, c]).max() / max(np.abs(want[:, c]).max(), 1e-300) for c in range(want.shape[1])))


# ------------------------------------------------------------------------------------------------ the host program
def build_program(out_dir, sanitize=True):
    """tools/bias2_host.cpp as a plain executable; returns run().  sanitize=True builds it with the address and undefined-behaviour
    sanitizers: that is for the CPU tests only (tests/test_cv_bias2_host.py).  The GPU tests take sanitize=False - the same source
    and optimisation level without the sanitizer flags, which prints the same fp32 numbers (the CPU tests compare the two builds bit
    for bit): no sanitizer runs inside a test marked gpu."""
    cxx = f"{codeobj.LLVM}/clang++"
    assert os.path.exists(cxx), f"{cxx}: the toolchain that builds the library is missing"
    exe = os.path.join(str(out_dir), "bias2_host" if sanitize else "bias2_host_plain")
    checks = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([cxx, "-O1", "-g", "-std=c++17"] + checks + ["-I" + os.path.join(codeobj.ROOT, "include"), "-I" + codeobj.CSRC, os.path.join(codeobj.ROOT, "tools", "bias2_host.cpp"), "-o", exe],
                   check=True, timeout=300)

    def run(terms, k, xi=(), deposits=(), table=None):
        """The program on term dicts (the vocabulary of export.bias_desc, which lays the table out) at points xi [P, k], then the
        deposit calls (term, height, sigma, sigma2, inv_kdt, xi rows [B, k]) in order.  `table` replaces the description's own
        (the same layout).  Returns (points [P, 1 + k + number of 2-D terms], hills [sum B, 4], table [n_table]) as fp64 arrays of
        the fp32 numbers printed."""
        from colvarsfinder import export
        d, tab = export.bias_desc(terms, k)
        tab = np.zeros(0, dtype=np.float32) if tab is None else tab.numpy()
        if table is not None:
            assert len(table) == len(tab)
            tab = np.asarray(table, dtype=np.float32)
        xi = np.asarray(xi, dtype=np.float32).reshape(-1, k)
        r = lambda v: repr(float(np.float32(v)))
        lines = [f"{k} {d.n_terms} {len(tab)} {len(xi)} {len(deposits)}"]
        for i in range(d.n_terms):
            e = d.term[i]
            lines.append(f"{e.kind} {e.cv} {r(e.kappa)} {r(e.center)} {e.tab_off} {e.n_nodes} {r(e.lo)} {r(e.inv_h)} {e.cv2} {e.n_nodes2} {r(e.lo2)} {r(e.inv_h2)}")
        lines.append(" ".join(r(v) for v in tab))
        lines += [" ".join(r(v) for v in row) for row in xi]
        for term, height, sigma, sigma2, inv_kdt, rows in deposits:
            rows = np.asarray(rows, dtype=np.float32).reshape(-1, k)
            lines.append(f"{term} {r(height)} {r(sigma)} {r(sigma2)} {r(inv_kdt)} {len(rows)}")
            lines += [" ".join(r(v) for v in row) for row in rows]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, timeout=60).stdout
        rows = {"P": [], "H": [], "T": []}
        for line in out.strip().split("\n"):
            rows[line[0]].append([float(v) for v in line[1:].split()])
        assert len(rows["P"]) == len(xi) and len(rows["T"]) == 1
        points = np.array(rows["P"]).reshape(len(xi), -1) if len(xi) else np.zeros((0, 1 + k))
        exact = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)    # (%.9g rounds back to the fp32 number)
        return exact(points), exact(np.array(rows["H"]).reshape(-1, 4)), exact(rows["T"][0])

    return run


def layout_of(terms, k):
    """(BiasDesc, table as numpy fp32) of the terms on the CPU: where export.bias_desc puts each term's nodes."""
    from colvarsfinder import export
    d, tab = export.bias_desc(terms, k)
    return d, (None if tab is None else tab.numpy())


# ------------------------------------------------------------------------------------------------ the deposit cases (host and GPU)
H1, LO1 = 0.25, -0.75                                                      # the 1-D grid: 6 nodes at -0.75 .. 0.5
GRID_LO, GRID_H = (-0.5, 0.25), (0.25, 0.5)                                 # the 5 x 4 grid: x -0.5 .. 0.5, y 0.25 .. 1.75 (all exact in fp32)
NANF = float("nan")
HILLS_1D = [[0.07], [1.3], [NANF]]                                          # inside, outside the grid, a NaN centre
HILLS_2D = [[0.07, 0.9], [0.8, 2.2], [NANF, 0.5]]


def deposit_terms(dim, filled):
    """The term that receives the hills: the smooth 1-D table of the 1-D host tests / the smooth 5 x 4 grid, or zero-filled ones."""
    if dim == 1:
        t = Bc.smooth_table(0, LO1, 1.0 / H1, 6, 0.1)
        if not filled:
            t = dict(t, u=np.zeros(6), du=np.zeros(6))
        return t
    t = smooth_grid(0, 1, GRID_LO, (1.0 / GRID_H[0], 1.0 / GRID_H[1]), (0.1, 0.8))
    if not filled:
        t = dict(t, **{key: np.zeros((N1, N2)) for key in ("u", "d1", "d2", "d12")})
    return t


def nodes_of(term):
    return np.stack([np.float32(term["u"]), np.float32(term["du"])], axis=1).astype(np.float64) if term["kind"] == "table" else term_nodes(term)


# ------------------------------------------------------------------------------------------------ the grid cases of the GPU tests
def grid_terms(case, xi0):
    """The terms of a grid case, placed from xi0 [B, k] (fp32, what a prior cvf_cv_frame_eval gave): frame 0 falls where the case
    says - region(case) - on the 5 x 4 grid over (CV 0, CV k-1).  The spacings are 0.25 and 0.5 (powers of two, halved for "on-node" until lo + j h
    is exact); the node data are smooth_grid's around frame 0, of order 1 like xi."""
    xi0 = np.asarray(xi0, dtype=np.float32)
    k = xi0.shape[1]
    a, b = (k - 1, 0) if case == "cv-swapped" else (0, k - 1)
    c = xi0[0, [a, b]].astype(np.float64)
    h = (0.25, 0.5)
    # frame 0 at cell coordinates (1.4, 1.3) - in cell (1, 1) of 4 x 3 - unless the case moves it
    s = {"interior": (1.4, 1.3), "below-1": (-0.6, 1.3), "above-1": (4.7, 1.3), "below-2": (1.4, -0.8), "above-2": (1.4, 3.6),
         "corner-low": (-0.6, -0.8), "corner-high": (4.7, 3.6), "on-node": (2.0, 1.0), "plus-harmonic": (1.4, 1.3), "cv-swapped": (1.4, 1.3)}[case]
    h = list(h)
    if case == "on-node":       # node (2, 1) sits on fp32(xi) of frame 0: halve the spacing until lo + j h is exact in fp32
        for i in (0, 1):
            while float(np.float32(c[i]) - np.float32(s[i] * h[i])) + s[i] * h[i] != float(np.float32(c[i])):
                h[i] *= 0.5
    lo = [np.float32(c[i]) - np.float32(s[i] * h[i]) for i in (0, 1)]
    terms = [smooth_grid(a, b, lo, (1.0 / h[0], 1.0 / h[1]), (c[0], c[1]))]
    if case == "plus-harmonic":
        terms.append({"kind": "harmonic", "cv": b, "kappa": 0.8, "center": float(xi0[:, b].min() - 1.5)})
    return terms


def region(term, xi_row):
    """(r1, r2), each -1 (below), 0 (inside, edges included) or +1 (above): where xi_row [k] (fp64) lies on the term's grid; and the
    cell coordinates."""
    lo, inv_h = term_axes(term)
    n = term_nodes(term).shape
    s = [(float(xi_row[term["cv"]]) - lo[0]) * inv_h[0], (float(xi_row[term["cv2"]]) - lo[1]) * inv_h[1]]
    return tuple(-1 if s[i] < 0 else (1 if s[i] > n[i] - 1 else 0) for i in (0, 1)), s


REGION_OF = {"interior": (0, 0), "below-1": (-1, 0), "above-1": (1, 0), "below-2": (0, -1), "above-2": (0, 1), "corner-low": (-1, -1),
             "corner-high": (1, 1), "on-node": (0, 0), "plus-harmonic": (0, 0), "cv-swapped": (0, 0)}
