"""Periodic cells in the bias launches (csrc/cvf_cell.hpp, cvf_cv_*_bias_*_cell_eval, cvf_md_make_whole):
the cells, how a whole frame is torn, the sequential rule written independently in numpy fp64 (the reference of both test files)
and the stand-alone host program.  `tests/test_cell_host.py` (CPU) and `tests/test_cv_bias_cell_gpu.py` (GPU) share it.

The reference is written without a look at csrc/cvf_cell.hpp's prefix sum: atom 0 stays, atom j takes the image of x_j nearest to the
WHOLE atom j - 1, the minimum image axis by axis in the order z, y, x with numpy's rint - everything in fp64 on the fp32 inputs."""
import os
import subprocess

import numpy as np

from tests import codeobj

EPS = float(np.finfo(np.float32).eps)
MARGIN = 1e-3      # every scaled difference of a test input stays this far from a half-integer (a condition on the inputs)

# 9 floats, rows a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz)
ORTHO = np.array([2.0, 0, 0, 0, 4.0, 0, 0, 0, 2.5])                     # every N L is exact in fp32
TRICLINIC = np.array([2.1, 0, 0, 0.37, 3.3, 0, -0.61, 0.83, 2.7])      # nothing exact
SLAB = np.array([2.0, 0, 0, 0.5, 3.0, 0, 0.25, -0.5, 0.0])             # cz = 0: z is not periodic
DYADIC = np.array([2.0, 0, 0, 0.5, 4.0, 0, -0.25, 0.75, 2.5])          # triclinic, every N h exact in fp32 (the GPU tests' bars)
CELLS = {"ortho": ORTHO, "triclinic": TRICLINIC, "slab": SLAB}


def periodic(cell):
    """Which of the axes x, y, z are periodic: a positive finite diagonal entry."""
    d = np.asarray(cell, dtype=np.float64).reshape(3, 3).diagonal()
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def heights(cell):
    """The diagonal entries of the periodic axes (the rule's own measure of a cell's height along an axis)."""
    d = np.asarray(cell, dtype=np.float64).reshape(3, 3).diagonal()
    return d[periodic(cell)]


def image_fp64(cell, d):
    """(n [3] ints, the scaled differences met on the way) of the minimum image of the difference d, axes z, y, x."""
    h = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    h = np.where(np.tril(np.ones((3, 3), dtype=bool)), h, 0.0)      # the upper triangle is not part of the cell
    on = periodic(cell)
    d = np.array(d, dtype=np.float64)
    n, scaled = np.zeros(3, dtype=np.int64), []
    for ax in (2, 1, 0):
        if not on[ax]:
            continue
        q = d[ax] / h[ax, ax]
        scaled.append(q)
        n[ax] = int(np.rint(q))
        d = d - n[ax] * h[ax]
    return n, scaled


def whole_fp64(cell, x):
    """(whole [n, 3] fp64, N [n, 3] ints, min distance of a scaled difference from a half-integer) of one wrapped frame x [n, 3]: the
    sequential rule."""
    h = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    h = np.where(np.tril(np.ones((3, 3), dtype=bool)), h, 0.0)
    on = periodic(cell)
    h = np.where(on[:, None], h, 0.0)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    w, N, margin = np.empty_like(x), np.zeros(x.shape, dtype=np.int64), 0.5
    w[0] = x[0]
    for j in range(1, len(x)):
        n, scaled = image_fp64(cell, x[j] - w[j - 1])
        N[j] = n
        w[j] = x[j] - n @ h
        for q in scaled:
            margin = min(margin, abs(abs(q - np.floor(q)) - 0.5))
    return w, N, margin


def lattice(cell):
    """The three lattice vectors as rows, fp64, zero rows for the axes that are not periodic."""
    h = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    h = np.where(np.tril(np.ones((3, 3), dtype=bool)), h, 0.0)
    return np.where(periodic(cell)[:, None], h, 0.0)


def random_walk(n_atoms, cell, rs):
    """A whole frame [n_atoms, 3] fp64: steps of length at most 0.3 of the shortest cell height, from a point inside the cell."""
    step = 0.3 * heights(cell).min()
    v = rs.normal(size=(n_atoms, 3))
    v *= (step * rs.uniform(0.2, 1.0, size=(n_atoms, 1))) / np.linalg.norm(v, axis=1, keepdims=True)
    v[0] = rs.uniform(0.1, 0.9, size=3) @ np.where(lattice(cell).any(axis=1)[:, None], lattice(cell), np.eye(3))
    return np.cumsum(v, axis=0)


def wrap_fp64(cell, x, centred=False):
    """Every atom of x [n, 3] (fp64) wrapped into the cell, axes z, y, x (into [0, L), or [-L/2, L/2) with centred)."""
    h, x = lattice(cell), np.array(x, dtype=np.float64)
    for ax in (2, 1, 0):
        if h[ax, ax] > 0:
            n = np.floor(x[:, ax] / h[ax, ax] + (0.5 if centred else 0.0))
            x = x - n[:, None] * h[ax][None]
    return x


def tear(cell, x, rs, shifts=2, keep_first=False, centred=False):
    """A wrapped frame as an engine holds it, fp32 [n, 3]: every atom of the whole frame x wrapped into the cell in fp64 and rounded to
    fp32, then moved by a random lattice vector with coefficients in {-shifts .. shifts} (atom 0 left in place with keep_first)."""
    x32 = wrap_fp64(cell, x, centred).astype(np.float32)
    s = rs.randint(-shifts, shifts + 1, size=(len(x32), 3))
    if keep_first:
        s[0] = 0
    return (x32.astype(np.float64) + s @ lattice(cell)).astype(np.float32)


def break_at(cell, x, j0, shift):
    """The whole frame x (fp32 [n, 3]) with the atoms j0 .. moved by the lattice vector of integer coefficients `shift`: one break,
    between atoms j0 - 1 and j0."""
    out = np.asarray(x, dtype=np.float64).copy()
    out[j0:] += np.asarray(shift, dtype=np.float64) @ lattice(cell)
    return out.astype(np.float32)


def build_program(out_dir, sanitize=True):
    """tools/cell_host.cpp as a plain executable; returns run().  sanitize=True builds it with the address and undefined-behaviour
    sanitizers: that is for the CPU tests only (tests/test_cell_host.py).  The GPU tests take sanitize=False - the same source and
    optimisation level without the sanitizer flags, which prints the same bits (the CPU tests compare the two builds): no sanitizer
    runs inside a test marked gpu."""
    cxx = f"{codeobj.LLVM}/clang++"
    assert os.path.exists(cxx), f"{cxx}: the toolchain that builds the library is missing"
    exe = os.path.join(str(out_dir), "cell_host" if sanitize else "cell_host_plain")
    checks = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([cxx, "-O1", "-g", "-std=c++17"] + checks + ["-I" + os.path.join(codeobj.ROOT, "include"), "-I" + codeobj.CSRC,
                    os.path.join(codeobj.ROOT, "tools", "cell_host.cpp"), "-o", exe], check=True, timeout=300)

    def run(cells, frames, triples=()):
        """The program on frames [F, n, 3] (fp32) under cells [F, 9] (fp32; or one [9] for all): (N [F, n, 3] ints, whole [F, n, 3] fp32,
        and per triple (word, nx, ny, nz))."""
        frames = np.asarray(frames, dtype=np.float32)
        F, n = frames.shape[0], frames.shape[1]
        cells = np.broadcast_to(np.asarray(cells, dtype=np.float32).reshape(-1, 9), (F, 9))
        num = lambda v: "nan" if np.isnan(v) else ("inf" if v == np.inf else ("-inf" if v == -np.inf else float(v).hex()))
        lines = [f"{n} {F} {len(triples)}"]
        for f in range(F):
            lines.append(" ".join(num(v) for v in cells[f]))
            lines.append(" ".join(num(v) for v in frames[f].reshape(-1)))
        lines += [" ".join(str(int(v)) for v in t) for t in triples]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, timeout=60).stdout
        rows = {"N": [], "W": [], "S": []}
        for line in out.strip().split("\n"):
            rows[line[0]].append(line[1:].split())
        assert len(rows["N"]) == F and len(rows["W"]) == F and len(rows["S"]) == len(triples)
        N = np.array([[int(v) for v in r] for r in rows["N"]], dtype=np.int64).reshape(F, n, 3)
        W = np.array([[int(v, 16) for v in r] for r in rows["W"]], dtype=np.uint32).reshape(F, n, 3).view(np.float32)
        S = [(int(r[0], 16), int(r[1]), int(r[2]), int(r[3])) for r in rows["S"]]
        return N, W, S

    return run
