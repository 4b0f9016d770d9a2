"""CPU: the periodic cell and the chain that makes a wrapped molecule whole - the ABI, and the text of
csrc/cvf_cell.hpp compiled into the stand-alone host program tools/cell_host.cpp (with -fsanitize=address,undefined, a plain
executable) against the sequential rule in numpy fp64 (tests/cv_cell_cases.py).

Inputs: whole frames of 7 and 70 atoms (a random walk, steps at most 0.3 of the shortest cell height), every atom wrapped into the
cell in fp64, rounded to fp32 and moved by a random lattice vector with coefficients in {-2 .. 2}; an orthorhombic cell whose N L
are exact in fp32, a triclinic cell, a slab (cz = 0).  In fp64 every scaled difference of these inputs is at least 1e-3 away from a
half-integer: asserted of every frame, none is left out (the seeds below were chosen for it)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import codeobj
from tests import cv_cell_cases as Cc

EPS = Cc.EPS
SEED = 2024
N_FRAMES = 4


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return Cc.build_program(tmp_path_factory.mktemp("cell"))


def inputs(name, n_atoms):
    """(cell [9] fp32, whole frames fp64 [F, n, 3], torn frames fp32 [F, n, 3]) of a cell and a size, seeded."""
    cell = Cc.CELLS[name].astype(np.float32)
    rs = np.random.RandomState(SEED + 7 * n_atoms + sum(map(ord, name)))
    whole = np.stack([Cc.random_walk(n_atoms, cell, rs) for _ in range(N_FRAMES)])
    torn = np.stack([Cc.tear(cell, w, rs) for w in whole])
    return cell, whole, torn


# ------------------------------------------------------------------------------------------------ ABI
def test_cell_entry_points_are_declared_bound_and_defined():
    from colvarsfinder import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(_hip.LIB_PATH)
    names = [f"cvf_cv_frame{large}_bias{shared}_cell_{what}" for large in ("", "_large") for shared in ("", "_shared") for what in ("eval", "supported")]
    for name in names + ["cvf_md_make_whole"]:
        assert name in declared and name in _hip._SIGNATURES and hasattr(handle, name), name
    assert set(_hip._SIGNATURES) == declared
    # the cell call takes its namesake's arguments and the cell behind them
    for large in ("", "_large"):
        for shared in ("", "_shared"):
            plain, cell = _hip._SIGNATURES[f"cvf_cv_frame{large}_bias{shared}_eval"], _hip._SIGNATURES[f"cvf_cv_frame{large}_bias{shared}_cell_eval"]
            assert cell[1][:-1] == plain[1] and cell[1][-1] is ctypes.POINTER(_hip.MDCell)


def test_md_cell_layout_matches_the_header(tmp_path):
    from colvarsfinder import _hip
    cc = f"{codeobj.LLVM}/clang"
    assert os.path.exists(cc), f"{cc}: the toolchain that builds the library is missing"
    exprs = ["sizeof(cvf_md_cell)", "offsetof(cvf_md_cell, cell)", "offsetof(cvf_md_cell, cell_frame_stride)", "offsetof(cvf_md_cell, virial_rows)"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cvf.h"\nint main(void) {\n'
                   + "".join(f'  printf("%zu\\n", {e});\n' for e in exprs) + "  return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run([cc, "-I" + os.path.join(codeobj.ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout.split()]
    M = _hip.MDCell
    assert got == [ctypes.sizeof(M), M.cell.offset, M.cell_frame_stride.offset, M.virial_rows.offset]


# ------------------------------------------------------------------------------------------------ the rule against fp64
@pytest.mark.parametrize("n_atoms", [7, 70])
@pytest.mark.parametrize("name", list(Cc.CELLS))
def test_chain_against_the_sequential_rule_in_fp64(program, name, n_atoms):
    cell, whole, torn = inputs(name, n_atoms)
    N, W, _ = program(cell, torn)
    h = np.abs(Cc.lattice(cell))
    moved = 0
    for f in range(N_FRAMES):
        w64, N64, margin = Cc.whole_fp64(cell, torn[f])
        assert margin >= Cc.MARGIN, (name, n_atoms, f, margin)       # the condition on the inputs, of every frame
        assert np.array_equal(N[f], N64), (name, n_atoms, f)         # image counts: exactly the reference's
        moved += int((N64 != 0).any(axis=1).sum())
        x64 = torn[f].astype(np.float64)
        if name == "ortho":      # every N L is exact: one rounding, of the exact difference
            assert np.array_equal(W[f].view(np.uint32), (x64 - N64 @ Cc.lattice(cell)).astype(np.float32).view(np.uint32)), (name, n_atoms, f)
        bound = 4 * EPS * (np.abs(x64) + np.abs(N64) @ h)            # per coordinate: |x| + sum_i |N_i| |h_i|
        err = np.abs(W[f].astype(np.float64) - w64)
        print(f"[cell] {name} n={n_atoms} frame {f}: max error / bound {float((err / bound).max()):.3f}, max |N| {int(np.abs(N64).max())}")
        assert (err <= bound).all(), (name, n_atoms, f, float((err / bound).max()))
        # the reference is the whole frame the input was torn from, up to the rounding of the wrapped coordinates and a lattice vector
        d = w64 - whole[f]
        assert np.abs(d - d[0]).max() <= 64 * EPS * np.abs(x64).max()
        if name == "slab":
            assert (N64[:, 2] == 0).all() and np.array_equal(W[f][:, 2].view(np.uint32), torn[f][:, 2].view(np.uint32))
    assert moved > n_atoms      # the frames are torn: most atoms carry an image count


@pytest.mark.parametrize("name", list(Cc.CELLS))
def test_a_whole_frame_comes_back_bit_for_bit(program, name):
    cell = Cc.CELLS[name].astype(np.float32)
    rs = np.random.RandomState(SEED + 1)
    frames = np.stack([Cc.random_walk(7, cell, rs), rs.uniform(-0.2, 0.2, size=(7, 3))]).astype(np.float32)
    frames[1, 3] = [-0.0, 0.0, -0.0]          # signed zeros keep their sign
    frames[1, 4] = [0.01, -0.01, 0.0]
    frames[1, 5:] = frames[1, 4]
    N, W, _ = program(cell, frames)
    assert (N == 0).all() and np.array_equal(W.view(np.uint32), frames.view(np.uint32))


def test_axes_that_are_not_periodic_are_left_alone(program):
    """A zero, a negative, a NaN and an infinite diagonal entry each switch their axis off - its count is 0, its coordinate keeps its
    bits, its lattice vector (here full of NaN) is never used - and the upper triangle is never read."""
    rs = np.random.RandomState(SEED + 2)
    base = Cc.TRICLINIC.astype(np.float32)
    whole = Cc.random_walk(7, base, rs)
    for ax, bad in ((2, 0.0), (2, -2.7), (2, np.nan), (1, np.nan), (0, -1.0), (0, np.inf), (1, 0.0)):
        cell = base.copy().reshape(3, 3)
        cell[ax, :ax] = np.nan
        cell[ax, ax] = bad
        cell[0, 1], cell[0, 2], cell[1, 2] = np.nan, 7.0, -np.inf       # the upper triangle
        cell = cell.reshape(9)
        clean = base.copy().reshape(3, 3)
        clean[ax] = 0.0
        torn = Cc.tear(clean.reshape(9), whole, rs)
        N, W, _ = program(cell, torn[None])
        w64, N64, margin = Cc.whole_fp64(clean.reshape(9), torn)
        assert margin >= Cc.MARGIN
        assert np.array_equal(N[0], N64) and (N[0][:, ax] == 0).all() and (N64 != 0).any(), (ax, bad)
        assert np.isfinite(W).all()
        assert np.array_equal(W[0][:, 2].view(np.uint32), torn[:, 2].view(np.uint32)) or ax != 2
        bound = 4 * EPS * (np.abs(torn.astype(np.float64)) + np.abs(N64) @ np.abs(Cc.lattice(clean.reshape(9))))
        assert (np.abs(W[0].astype(np.float64) - w64) <= bound).all(), (ax, bad)


def test_the_packed_image_word_saturates(program):
    triples = [(0, 0, 0), (1, -1, 2), (500, -500, 499), (511, -511, 0), (512, -512, 1), (100000, -100000, 2 ** 31 - 1), (-2 ** 31, 5, -7)]
    _, _, S = program(Cc.ORTHO, np.zeros((0, 1, 3), dtype=np.float32), triples)
    clip = lambda v: max(-511, min(511, v))
    for t, (word, nx, ny, nz) in zip(triples, S):
        assert (nx, ny, nz) == tuple(clip(v) for v in t), (t, hex(word))
        assert word < 2 ** 30 and (word == 0) == (t == (0, 0, 0))
    # a chain whose counts pass the word's range: 600 images along x in one step saturate at 511 and stay there
    cell = Cc.ORTHO.astype(np.float32)
    frame = np.zeros((1, 3, 3), dtype=np.float32)
    frame[0, 1, 0] = 1200.0            # 600 cells away
    frame[0, 2, 0] = 1200.5
    N, W, _ = program(cell, frame)
    assert N[0, 1, 0] == 511 and N[0, 2, 0] == 511 and np.isfinite(W).all()


def test_both_builds_print_the_same_bits(program, tmp_path):
    """The GPU tests build the program without the sanitizers (no sanitizer runs in a test marked gpu): the same bits."""
    plain = Cc.build_program(tmp_path, sanitize=False)
    for name in Cc.CELLS:
        cell, _, torn = inputs(name, 70)
        a, b = program(cell, torn), plain(cell, torn)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
