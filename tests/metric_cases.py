"""Case table, builders and references of the direct tests of the generator-mode metric kernels, ``q = J A J^T g`` and
``E = g^T J A J^T g`` per frame and net (tests/test_metric_cases_host.py, tests/test_metric_cases_gpu.py, tests/metric_switch_child.py).

Kernels: ``metric_rows_kernel<F, waves, kGeoPre, kMulti>`` and ``metric_dense_kernel<WEIGHTED>`` (csrc/metric_large.hip, frames of more
than 64 atoms), ``metric_pure_kernel`` and ``metric_align_kernel`` (csrc/k1_align.hip, smaller frames).  Which of them a call launches
is asked of ``cvf_metric_route`` - the function the launch itself decides by; the formulae it uses are mirrored below (``rows_lds``,
``rows_npb``, ``pure_lds``, ...), and the host test fails when a mirror and the library disagree.

Reference: ``oracle.pp.AlignFeature`` in fp64 (``compact=True`` above 64 atoms): ``u = vjp(g)``, ``E_ref = sum a u^2``,
``q_ref = jvp(a * u)``, per frame and net, for a cotangent ``g`` drawn here - no nets.  The *fp32 twin* is the same graph through the
same oracle code in fp32 on the CPU.  Error measure (tests/align_hvp_cases.py): per frame ``max_j |q - q_ref| / max_j |q_ref|``, the
worst frame and net counts; for E ``|E - E_ref| / E_ref``.  Bar of a case and quantity: ``max(1.5e-5, 3 x the twin's error on the same
inputs)`` - 1.5e-5 is the project's VJP / JVP bar, 3 its margin over a twin.  No bar may exceed ``CEILING = 1e-4``:
the feature lists are drawn away from straight angles and short bonds (``_ok_*``) so that the twin alone keeps this; the host test
asserts it on the CPU.  The bars are never read off the kernels.

What the table cannot reach, with the arithmetic (``W`` waves, ``LG = 64 W / F`` lane groups, ``LG kGeoPre`` records in registers):

* ``n_mrec < LG`` at F = 8 and F = 4.  A record owns at most four contribution rows, so ``n_ref <= 4 n_mrec``; F = 8 is taken only
  when ``rows_lds(F = 16)`` exceeds 158 KiB, which needs ``48 n_ref + 8 n_slot > 38 576`` floats and, with ``n_slot <= n_ref``,
  ``n_ref >= 689``: more than ``4 (LG - 1) = 252`` (8 waves) or 508 (16 waves).  F = 4 likewise needs ``n_ref >= 1235``.
* ``n_mrec`` within one of ``LG kGeoPre = 256`` at F = 4 with 8 waves: ``n_ref <= 4 * 257 = 1028 < 1235``.  Every F = 4 list has
  overflow records; with 16 waves ``LG kGeoPre = 512`` and the edge is in reach (the child process runs it).

``test_unreachable_edges_are_unreachable`` asserts both from ``rows_lds``."""
import functools
import math
import types
from collections import namedtuple

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from tests.synth import diag_coeff_for, make_molecule_traj
from tests.test_align_vjp_gpu import MIXED

FLOOR, TWIN_MARGIN, CEILING = 1.5e-5, 3.0, 1e-4
TILE, MAX_NETS = 64, 8
BATCHES = (1, 5, 63, 64, 65, 130)
SCALE, SIGMA = 4.0, 0.25            # frames: make_molecule_traj(n, 130, seed, scale, sigma); a case takes the first B
NCU = 256                           # compute units of the MI355X (cvf_cu_count; also its answer without a device)

# ------------------------------------------------------------------------------------------------ mirrored rules
BUDGET = 158 * 1024                 # kBudget (csrc/metric_large.hip)
N_RED = 13                          # kNRed
FUSE_MAX_GROUPS = 384               # rows kernel: fused first stage up to this many frame groups
FUSE_MAX_TILES = 1024               # kFuseMaxTiles (csrc/cvf_metric.hpp): pure kernel
PURE_ALL_NETS_LDS = 80 * 1024       # metric_pure_kernel: all k nets in one workgroup up to here
K_SLOTS, G_CHUNK = 3, 8             # kSlots (phase B), kGChunk (metric_pure_passes)
ROUTE_ALIGN, ROUTE_PURE, ROUTE_ROWS = 3, 4, 5
PP_ALIGN_CONTIG, PP_PURE_POSITION = 1, 2


def rows_lds(n_ref, n_slot, F, W=8):
    """metric_rows_lds: bytes."""
    return (n_ref * 3 * F + 8 * n_slot + N_RED * W * F + N_RED * F) * 4


def rows_F(n_ref, n_slot, W=8):
    """Frames per workgroup of the rows kernel; None: refused (> 158 KiB even at F = 4)."""
    for F in (16, 8, 4):
        if rows_lds(n_ref, n_slot, F, W) <= BUDGET:
            return F
    return None


def max_ref(F, n_slot, W=8):
    """The largest n_ref that still takes F frames per workgroup."""
    return (BUDGET // 4 - 8 * n_slot - N_RED * W * F - N_RED * F) // (3 * F)


def lane_groups(F, W=8):
    return W * 64 // F


def geo_pre(F, W=8, multi=False, pre_env=7):
    """kGeoPre of the instance cvf_metric_rows_plan picks."""
    if W == 16:
        return 2
    return {16: 5 if multi and pre_env != 7 else 7, 8: 4, 4: 2}[F]


def in_regs(F, W=8, multi=False, pre_env=7):
    """Records whose geometry stays in registers: LG kGeoPre."""
    return lane_groups(F, W) * geo_pre(F, W, multi, pre_env)


def rows_npb(B, k, F, env=None, ncu=NCU):
    """Nets per workgroup: the cost model of cvf_metric_rows_plan, or CVF_METRIC_NPB when it divides k."""
    if env is not None and env > 0 and k % env == 0:
        return env
    per_net = ((B + TILE - 1) // TILE) * (TILE // F)
    best, npb = 0.0, 1
    for c in range(1, k + 1):
        if k % c:
            continue
        wgs = float(per_net * (k // c))
        rounds = float((int(wgs) + ncu - 1) // ncu) if wgs <= 2.0 * ncu else wgs / ncu
        cost = rounds * (7.0 + 17.5 * c)
        if c == 1 or cost < best:
            best, npb = cost, c
    return npb


def x_tile_stride(nc):
    return nc if nc & 3 == 2 else nc | 1


def pure_lds(nc, nal, wpb):
    """lds_for(wpb) of metric_apply's plan: bytes."""
    return (TILE * x_tile_stride(nc) + 3 * nal + nc + wpb * nc * TILE) * 4


def pure_wpb(nc, nal, k):
    return k if pure_lds(nc, nal, k) <= PURE_ALL_NETS_LDS else 1


def align_lds(nc, n_rec, nal):
    return (TILE * (x_tile_stride(nc) + nc) + 6 * n_rec + 4 * nal + nc) * 4


def n_tiles(B):
    return (B + TILE - 1) // TILE


# ------------------------------------------------------------------------------------------------ cases
# kind: rows | pure | align.  rows: a feature list of exactly n_mrec records, n_ref contribution rows and n_slot feature atoms (build:
# rows_features); hubs = ((pool index, records that share the atom), ...), a negative index counts from the last slot.
# npb: CVF_METRIC_NPB of the call (None: unset, the cost model decides).  waves / pre: the process-wide developer switches the case needs
# (CVF_METRIC_WAVES, CVF_METRIC_PRE); anything but (8, 7) runs in the child process (tests/metric_switch_child.py).
Case = namedtuple("Case", "id kind n n_slot n_pos n_mrec n_ref hubs B k npb angle align weighted waves pre seed")


def _rows(id, n, n_slot, n_pos, n_mrec, n_ref, B, k, npb=None, hubs=(), angle=False, align="all", weighted=False, waves=8, pre=7, seed=0):
    return Case(id, "rows", n, n_slot, n_pos, n_mrec, n_ref, tuple(hubs), B, k, npb, angle, align, weighted, waves, pre, seed)


def _pure(n_rec, n_align, k, B, n=None):
    n = n or n_rec
    return Case(f"pure-n{n_rec}-al{n_align}-k{k}-B{B}" + (f"-of{n}" if n != n_rec else ""), "pure", n, n_rec, n_rec, n_rec, n_rec, (), B, k,
                None, False, n_align, False, 8, 7, 0)


def _align(n, weighted, angle, k, B):
    return Case(f"align-n{n}-{'w' if weighted else 'u'}{'-val' if angle else ''}-k{k}-B{B}", "align", n, 10, 4, 10, 0, (), B, k, None, angle,
                "subset", weighted, 8, 7, 0)


M16, M8, M4 = max_ref(16, 100), max_ref(8, 100), max_ref(4, 100)       # 787, 1613, 3265 rows at 100 feature atoms

ROWS_CASES = [
    # ---- LDS thresholds: n_ref just under and just over each (n_slot = 100 of 120 atoms)
    _rows("f16-lds-under", 120, 100, 40, 300, M16, 65, 3, npb=1),
    _rows("f8-lds-over", 120, 100, 40, 300, M16 + 1, 65, 3, npb=1),
    _rows("f8-lds-under", 120, 100, 40, 600, M8, 65, 3, npb=3),
    _rows("f4-lds-over", 120, 100, 40, 600, M8 + 1, 65, 3, npb=3),
    _rows("f4-lds-under", 120, 100, 40, 1100, M4, 63, 2, npb=1),
    # ---- record edges, F = 16 (LG = 32, 224 in registers; slots: LG * 3 = 96)
    _rows("f16-rec-lt-lg", 65, 20, 8, 20, 42, 65, 1),
    _rows("f16-rec-223", 130, 95, 30, 223, 600, 63, 3, npb=1, hubs=((0, 1), (1, 2), (-1, 40))),
    _rows("f16-rec-224", 130, 96, 30, 224, 601, 64, 3, npb=3, hubs=((0, 1), (1, 2), (-1, 40))),
    _rows("f16-rec-225", 130, 97, 30, 225, 602, 65, 6, npb=2, hubs=((0, 1), (1, 2), (-33, 40), (-1, 1))),
    _rows("f16-rec-450", 300, 230, 200, 450, 740, 130, 1),
    _rows("f16-slots-193", 256, 193, 60, 230, 500, 5, 8, npb=8, hubs=((-1, 40),)),
    # ---- record edges, F = 8 (LG = 64, 256 in registers).  (Few bonds fit a list of ~256 records and ~800 rows, so these lists have
    #      60 feature atoms and the slot edges - LG * 3 = 192 - have lists of their own.)
    _rows("f8-rec-255", 130, 60, 20, 255, 800, 63, 3, npb=1, hubs=((0, 1), (1, 2), (-1, 40))),
    _rows("f8-rec-256", 130, 60, 20, 256, 801, 64, 6, npb=3, hubs=((0, 1), (1, 2), (-1, 40))),
    _rows("f8-rec-257", 130, 60, 20, 257, 802, 65, 1, hubs=((0, 1), (1, 2), (-1, 40))),
    _rows("f8-rec-520", 200, 160, 100, 520, 1500, 130, 8, npb=4),
    _rows("f8-slots-191", 220, 191, 100, 400, 1000, 63, 2, npb=2, hubs=((-1, 40),)),
    _rows("f8-slots-192", 220, 192, 100, 400, 1001, 64, 2, npb=1, hubs=((-65, 40), (-1, 1))),
    _rows("f8-slots-193", 220, 193, 100, 400, 1002, 65, 2, npb=2, hubs=((-1, 40),)),
    _rows("f8-k8-npb8", 120, 100, 40, 300, 1000, 5, 8, npb=8),
    # ---- F = 4 (LG = 128, 256 in registers: every list overflows; slots: 384)
    _rows("f4-rec-500", 130, 60, 10, 500, 1640, 63, 3, npb=1, hubs=((0, 1), (1, 2), (-1, 40))),
    _rows("f4-slots-383", 420, 383, 150, 800, 1900, 64, 6, npb=2, hubs=((-129, 40), (-1, 1))),
    _rows("f4-slots-385", 420, 385, 150, 800, 1901, 65, 1, hubs=((-1, 40),)),
    _rows("f4-k8-npb8", 120, 100, 40, 600, 2000, 5, 8, npb=8),
    _rows("f4-k6-npb6", 120, 100, 40, 600, 2000, 130, 6, npb=6),
    # ---- the other axes, on each F
    _rows("f16-angle-value", 130, 100, 30, 240, 640, 65, 3, npb=3, angle=True),
    _rows("f8-angle-value", 130, 100, 30, 300, 1000, 65, 3, npb=1, angle=True),
    _rows("f4-angle-value", 130, 100, 30, 600, 1900, 65, 3, npb=3, angle=True),
    _rows("f16-no-position", 130, 100, 0, 230, 640, 65, 3),
    _rows("f8-no-position", 130, 100, 0, 300, 1000, 65, 2, npb=2),
    _rows("f4-no-position", 130, 100, 0, 600, 1900, 65, 2, npb=1),
    _rows("f16-subset", 300, 100, 30, 240, 640, 65, 3, align="subset"),
    _rows("f8-subset", 300, 100, 30, 300, 1000, 65, 3, npb=3, align="subset"),
    _rows("f4-subset", 300, 200, 60, 600, 1900, 65, 2, align="subset"),
    _rows("f16-weighted", 130, 100, 30, 240, 640, 65, 3, npb=1, weighted=True),
    _rows("f8-weighted-subset", 300, 100, 30, 300, 1000, 65, 3, npb=3, align="subset", weighted=True),
    _rows("f4-weighted-value", 130, 100, 30, 600, 1900, 65, 6, npb=3, weighted=True, angle=True),
    # ---- ragged batches: B mod 64 in {1, F - 1, F, F + 1, 63} (run with zero and with garbage padding)
    _rows("f16-B65", 130, 100, 30, 240, 640, 65, 2, npb=2),
    _rows("f16-B79", 130, 100, 30, 240, 640, 79, 2, npb=1),
    _rows("f16-B16", 130, 100, 30, 240, 640, 16, 2, npb=2),
    _rows("f16-B81", 130, 100, 30, 240, 640, 81, 2, npb=1),
    _rows("f16-B127", 130, 100, 30, 240, 640, 127, 2, npb=2),
    _rows("f8-B1", 130, 100, 30, 300, 1000, 1, 2, npb=1),
    _rows("f8-B71", 130, 100, 30, 300, 1000, 71, 2, npb=2),
    _rows("f8-B8", 130, 100, 30, 300, 1000, 8, 2, npb=1),
    _rows("f8-B73", 130, 100, 30, 300, 1000, 73, 2, npb=2),
    _rows("f8-B63", 130, 100, 30, 300, 1000, 63, 2, npb=1),
    _rows("f4-B1", 130, 100, 30, 600, 1900, 1, 2, npb=2),
    _rows("f4-B67", 130, 100, 30, 600, 1900, 67, 2, npb=1),
    _rows("f4-B4", 130, 100, 30, 600, 1900, 4, 2, npb=2),
    _rows("f4-B69", 130, 100, 30, 600, 1900, 69, 2, npb=1),
    _rows("f4-B127", 130, 100, 30, 600, 1900, 127, 2, npb=2),
]

# the instances behind the process-wide switches: one child process per switch (tests/metric_switch_child.py)
SWITCH_CASES = [
    _rows("w16-f16-rec-lt-lg", 65, 40, 10, 50, 130, 65, 3, npb=1, waves=16),                       # LG = 64
    _rows("w16-f16-rec-129", 130, 100, 30, 129, 300, 63, 3, npb=3, waves=16),                      # 128 in registers
    _rows("w16-f8-rec-257", 130, 60, 20, 257, 802, 65, 2, npb=2, waves=16, hubs=((-1, 40),)),     # LG = 128, 256 in registers
    _rows("w16-f4-rec-511", 130, 60, 10, 511, 1700, 63, 2, npb=1, waves=16),                      # LG = 256, 512 in registers
    _rows("w16-f4-rec-513", 130, 60, 10, 513, 1700, 65, 6, npb=3, waves=16, hubs=((-1, 40),)),
    _rows("pre5-f16-rec-159", 130, 100, 30, 159, 450, 63, 3, npb=3, pre=5),                        # LG = 32, 160 in registers
    _rows("pre5-f16-rec-161", 130, 100, 30, 161, 400, 65, 6, npb=2, pre=5, hubs=((-1, 40),)),
    _rows("pre5-f16-rec-330", 130, 100, 30, 330, 700, 130, 2, npb=2, pre=5),
]

PURE_CASES = [
    _pure(3, 3, 1, 1), _pure(3, 3, 8, 65), _pure(7, 7, 3, 5), _pure(7, 4, 8, 63), _pure(8, 8, 6, 64), _pure(8, 5, 1, 65),
    _pure(9, 9, 8, 130), _pure(9, 5, 3, 65), _pure(16, 16, 5, 65), _pure(16, 16, 6, 65), _pure(16, 10, 3, 64),
    _pure(17, 17, 5, 63), _pure(17, 12, 6, 65), _pure(22, 22, 3, 65), _pure(22, 22, 4, 130), _pure(22, 15, 8, 5),
    _pure(64, 64, 1, 65), _pure(64, 40, 3, 130), _pure(64, 64, 8, 1), _pure(9, 6, 2, 65, n=12),
]

ALIGN_CASES = [_align(10, False, False, 3, 65), _align(10, True, False, 2, 63), _align(10, False, True, 1, 130),
               _align(64, False, False, 2, 65), _align(64, True, True, 3, 64), _align(64, True, False, 8, 5)]

CASES = ROWS_CASES + PURE_CASES + ALIGN_CASES          # run in the test process
ALL_CASES = CASES + SWITCH_CASES
BY_ID = {c.id: c for c in ALL_CASES}

# cvf_metric_apply_stats: (case id of the layer, B, k).  The rows kernel writes one row per frame group of F frames while there are at
# most 384 of them; the pure kernel one per tile up to 1024 tiles.  Frames: the case's 130, repeated.
STATS_CASES = [("f16-angle-value", 384 * 16, 3), ("f16-angle-value", 385 * 16, 3), ("f8-angle-value", 384 * 8, 3),
               ("f8-angle-value", 385 * 8, 3), ("f4-angle-value", 384 * 4, 3), ("f4-angle-value", 385 * 4, 3),
               ("pure-n3-al3-k8-B65", 1024 * 64, 3), ("pure-n3-al3-k8-B65", 1024 * 64 + 1, 3),
               ("f8-B71", 71, 2), ("pure-n7-al4-k8-B63", 63, 8)]

# compiled kernels no case can launch: {(family, template arguments): why}
UNREACHABLE = {}


def n_records(feats):
    return sum(len(atoms) if t == "position" else 1 for t, atoms in feats)


def instance(case):
    """(kernel family, template arguments) the case launches, from the mirrors."""
    if case.kind == "pure":
        return ("metric_pure_kernel", ())
    if case.kind == "align":
        return ("metric_align_kernel", ())
    p = expected_plan(case, with_stats=False)
    return ("metric_rows_kernel", (p["F"], p["waves"], p["geo_pre"], p["multi"]))


def expected_plan(case, with_stats=False, B=None, k=None, npb="case"):
    """The fields of cvf_metric_plan the mirrors predict for the case (B, k, npb: overrides)."""
    B, k = B or case.B, k or case.k
    T = n_tiles(B)
    if case.kind == "pure":
        nal = case.align
        wpb = pure_wpb(3 * case.n, nal, k)
        fused = int(with_stats and T <= FUSE_MAX_TILES)
        return dict(family=ROUTE_PURE, F=0, waves=wpb, geo_pre=0, multi=0, npb=0, nets_per_wg=wpb, fused=fused, fused_rows=T * fused,
                    lds_bytes=pure_lds(3 * case.n, nal, wpb), grid=T * (k // wpb))
    if case.kind == "align":
        s = build(case)
        return dict(family=ROUTE_ALIGN, F=0, waves=1, geo_pre=0, multi=0, npb=0, nets_per_wg=1, fused=0, fused_rows=0,
                    lds_bytes=align_lds(3 * case.n, n_records(MIXED), len(s.align)), grid=T * k)
    W = case.waves
    F = rows_F(case.n_ref, case.n_slot, W)
    n = rows_npb(B, k, F, case.npb if npb == "case" else npb)
    multi = int(W == 16 or n > 1)
    groups = T * (TILE // F)
    fused = int(with_stats and groups <= FUSE_MAX_GROUPS)
    return dict(family=ROUTE_ROWS, F=F, waves=W, geo_pre=geo_pre(F, W, bool(multi), case.pre), multi=multi, npb=n, nets_per_wg=n,
                fused=fused, fused_rows=groups * fused, lds_bytes=rows_lds(case.n_ref, case.n_slot, F, W), grid=groups * k // n)


# ------------------------------------------------------------------------------------------------ builders
@functools.lru_cache(maxsize=None)
def frames(n, seed):
    """(traj [130, n, 3] fp32, frame weights [130], ref [n, 3])"""
    traj, w, ref = make_molecule_traj(n, max(BATCHES), seed=4000 + 7 * n + seed, scale=SCALE, sigma=SIGMA)
    traj.setflags(write=False)
    return traj, w, ref


MIN_BOND, MAX_COS = 1.0, 0.8     # no feature with a bond shorter than 1 or a bond angle within acos(0.8) = 37 degrees of straight, on any frame


def _ok_bond(x, a, b):
    return a != b and float(np.linalg.norm(x[:, a] - x[:, b], axis=1).min()) > MIN_BOND


def _ok_angle(x, a, b, c):
    if len({a, b, c}) < 3 or not (_ok_bond(x, a, b) and _ok_bond(x, c, b)):
        return False
    u, v = x[:, a] - x[:, b], x[:, c] - x[:, b]
    cs = (u * v).sum(1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))
    return float(np.abs(cs).max()) < MAX_COS


def _ok_dihedral(x, a, b, c, d):
    return len({a, b, c, d}) == 4 and _ok_angle(x, a, b, c) and _ok_angle(x, b, c, d)


def rows_counts(case):
    """(n_bond, n_angle, n_dihedral, coverage bonds, hub bonds) of a rows case: n_pos + b + a + d = n_mrec records and
    n_pos + 2 b + 3 a + 4 d = n_ref rows, with enough bonds to touch every pool atom and to give the hubs their records."""
    p, hub = case.n_pos, sum(c for _, c in case.hubs)
    cover = (case.n_slot - len(case.hubs) - p + 1) // 2
    M, R = case.n_mrec - p, case.n_ref - p
    Q = R - 2 * M                       # = a + 2 d
    assert Q >= 0 and cover >= 0, case.id
    a = Q // 3
    a += (a - Q) % 2                    # (a and Q of one parity)
    while a >= 0:
        d = (Q - a) // 2
        b = M - a - d
        if b >= hub + cover:
            return b, a, d, cover, hub
        a -= 2
    raise AssertionError(f"{case.id}: no feature list with these counts")


@functools.lru_cache(maxsize=None)
def rows_features(case):
    """(features, pool): position records on the first n_pos free pool atoms, bonds that pair up the other free atoms, hub bonds,
    then bonds, angles and dihedrals drawn over the free atoms, each accepted by _ok_* on all 130 frames."""
    x = frames(case.n, case.seed)[0].astype(np.float64)
    rs = np.random.RandomState(1000 + case.n_mrec + case.n_ref + case.seed)
    pool = list(range(case.n_slot)) if case.align == "all" else sorted(int(i) for i in rs.choice(case.n, case.n_slot, replace=False))
    hubs = {pool[i]: c for i, c in case.hubs}
    free = [p for p in pool if p not in hubs]
    n_bond, n_ang, n_dih, cover, _ = rows_counts(case)
    feats = [("position", tuple(free[:case.n_pos]))] if case.n_pos else []
    rest = free[case.n_pos:]
    bonds = []
    for _ in range(200):                                  # a pairing of the uncovered atoms whose bonds are all acceptable
        order = [rest[i] for i in rs.permutation(len(rest))]
        if len(order) % 2:
            order.append(free[int(rs.randint(len(free)))])
        pairs = list(zip(order[0::2], order[1::2]))
        if all(_ok_bond(x, a, b) for a, b in pairs):
            bonds = pairs
            break
    assert len(bonds) == cover, case.id

    def draw(m, ok):
        for _ in range(10000):
            atoms = tuple(int(free[i]) for i in rs.choice(len(free), m, replace=False))
            if ok(x, *atoms):
                return atoms
        raise AssertionError(case.id)

    for h, c in hubs.items():
        for j in range(c):
            while True:
                o = int(free[int(rs.randint(len(free)))])
                if _ok_bond(x, h, o):
                    break
            bonds.append((h, o) if j % 2 else (o, h))
    bonds += [draw(2, _ok_bond) for _ in range(n_bond - len(bonds))]
    feats += [("bond", b) for b in bonds]
    feats += [("angle", draw(3, _ok_angle)) for _ in range(n_ang)]
    feats += [("dihedral", draw(4, _ok_dihedral)) for _ in range(n_dih)]
    return tuple(feats), tuple(pool)


@functools.lru_cache(maxsize=None)
def build(case):
    """Everything about a case that does not depend on the device: features, align set, weights, frames, a, g."""
    s = types.SimpleNamespace(case=case)
    traj, s.w_frames, s.ref = frames(case.n, case.seed)
    s.traj = traj[:case.B] if case.B <= len(traj) else None
    rs = np.random.RandomState(77 + case.n + case.seed)
    if case.kind == "rows":
        s.feats, s.pool = rows_features(case)
        s.feats = list(s.feats)
        s.align = list(range(case.n)) if case.align == "all" else sorted(int(i) for i in rs.choice(case.n, 2 * case.n // 3, replace=False))
    elif case.kind == "pure":
        s.feats, s.align = [("position", tuple(range(case.n_slot)))], list(range(case.align))
    else:
        s.feats = MIXED
        s.align = [0, 1, 2, 4, 5, 8] if case.n == 10 else sorted({0, 1, 2, 4, 5, 8} | {int(i) for i in rs.choice(case.n, case.n // 2, replace=False)})
    s.aw = rs.uniform(0.2, 3.0, size=len(s.align)) if case.weighted else None
    used = {a for _, atoms in s.feats for a in atoms}
    s.unused = [a for a in range(case.n) if a not in used and a not in set(s.align)]
    s.a = diag_coeff_for(case.n, 3 + case.seed).astype(np.float32)
    return s


def layer_of(case, dev=None):
    from colvarsfinder import pp
    s = build(case)
    layer = pp.AlignFeatureLayer(case.n, s.align, s.ref[s.align], s.feats, case.angle, align_weights=s.aw, weights_any_size=True)
    return layer if dev is None else layer.to(dev)


def host_desc(case):
    """cvf_pp_desc with the counts and flags of the case's layer and NULL tables (align_w: a non-NULL token when weighted) - all that
    cvf_metric_route reads."""
    from colvarsfinder import _hip
    layer = layer_of(case)
    d = _hip.PPDesc()
    d.mode, d.n_coord, d.n_align, d.n_rec = _hip.PP_ALIGN, 3 * layer.n_atoms, layer.align_idx.numel(), layer.rec.shape[0]
    d.d_r, d.use_angle_value, d.flags = layer.d_r, int(layer.use_angle_value), layer._flags
    d.has_position = int(any(t == "position" for t, _ in layer.features))
    d.n_slot, d.n_rec_slot, d.n_mrec, d.n_ref = layer._n_slot, layer._n_rec_slot, layer.mrec.shape[0], layer._n_ref
    d.align_w = 64 if layer.align_w is not None else None
    return d, layer


def cotangent(case, d_r, B=None, k=None):
    """g [B, k, d_r] fp32."""
    B, k = B or case.B, k or case.k
    gen = torch.Generator().manual_seed(31 * B + 7 * k + case.n_ref)
    return torch.randn(B, k, d_r, generator=gen, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ references
def _oracle_metric(case, dtype):
    from oracle.pp import AlignFeature
    s = build(case)
    torch.set_default_dtype(dtype)   # (the oracle's buffers take the default type when it is built)
    try:
        f = AlignFeature(s.align, s.ref[s.align], s.feats, case.angle, align_weights=s.aw, compact=case.n > 64)
        B, k, n = case.B, case.k, case.n
        x = torch.tensor(s.traj, dtype=dtype).repeat_interleave(k, dim=0)            # [B k, n, 3]: frame b, net i at row b k + i
        xr = x.clone().requires_grad_(True)
        y = f(xr)
        g = cotangent(case, y.shape[1]).to(dtype).reshape(B * k, -1)
        (u,) = torch.autograd.grad(y, xr, g)
        au = torch.tensor(s.a, dtype=dtype).reshape(1, n, 3) * u
        E = (au * u).sum(dim=(1, 2))
        with fwAD.dual_level():
            q = fwAD.unpack_dual(f(fwAD.make_dual(x, au.detach()))).tangent.clone()
    finally:
        torch.set_default_dtype(torch.float32)
    return q.double().reshape(B, k, -1).numpy(), E.double().reshape(B, k).numpy()


def q_errors(q, q_ref):
    """e_f of every (frame, net): [B, k]."""
    return np.abs(np.asarray(q, dtype=np.float64) - q_ref).max(axis=2) / np.abs(q_ref).max(axis=2)


def e_errors(E, E_ref):
    return np.abs(np.asarray(E, dtype=np.float64) - E_ref) / E_ref


Ref = namedtuple("Ref", "q E twin_q twin_E bar_q bar_E")


@functools.lru_cache(maxsize=None)
def reference(case):
    """(q_ref [B, k, d_r], E_ref [B, k] in fp64; the fp32 twin's worst errors; the bars of the case)."""
    q, E = _oracle_metric(case, torch.float64)
    assert np.isfinite(q).all() and np.isfinite(E).all() and (E > 0).all() and (np.abs(q).max(axis=2) > 0).all(), case.id
    q32, E32 = _oracle_metric(case, torch.float32)
    tq, tE = float(q_errors(q32, q).max()), float(e_errors(E32, E).max())
    q.setflags(write=False)
    E.setflags(write=False)
    return Ref(q, E, tq, tE, max(FLOOR, TWIN_MARGIN * tq), max(FLOOR, TWIN_MARGIN * tE))


# ------------------------------------------------------------------------------------------------ tiled buffers
def to_tiled(rows, B):
    """[B, k, d] -> fp32 [T, k, d, 64], padded lanes 0."""
    rows = np.asarray(rows, dtype=np.float32)
    k, d = rows.shape[1], rows.shape[2]
    T = n_tiles(B)
    out = np.zeros((T * TILE, k, d), dtype=np.float32)
    out[:B] = rows
    return np.ascontiguousarray(out.reshape(T, TILE, k, d).transpose(0, 2, 3, 1))


def from_tiled(tiled, B):
    """fp32 [T, k, d, 64] -> [B, k, d]."""
    T, k, d, _ = tiled.shape
    return np.ascontiguousarray(np.asarray(tiled).transpose(0, 3, 1, 2)).reshape(T * TILE, k, d)[:B]


def garbage(shape, seed):
    """Finite values of magnitude ~1e3 and mixed sign (tests/stats_tail_cases.py: tiled)."""
    rs = np.random.RandomState(900 + seed)
    return (rs.uniform(500.0, 2000.0, shape) * rs.choice([-1.0, 1.0], shape)).astype(np.float32)


def stats_terms(w, y, E):
    """[ns][B] fp64: the term of every generator-mode statistic for every frame, [W | S1(k) | S2(i <= j) | E(k)] (include/cvf.h),
    from fp32 w [B], y [B, k], E [B, k]."""
    w, y, E = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (w, y, E))
    k = y.shape[1]
    rows = [w] + [w * y[:, i] for i in range(k)] + [w * y[:, i] * y[:, j] for i in range(k) for j in range(i, k)]
    rows += [w * E[:, i] for i in range(k)]
    return np.stack(rows)


def exact_sums(terms):
    return (np.array([math.fsum(r) for r in terms.tolist()]), np.array([math.fsum(r) for r in np.abs(terms).tolist()]))


# ------------------------------------------------------------------------------------------------ the C ABI
class _npb_env:
    """CVF_METRIC_NPB for the calls inside (None: unset); the library reads it on every call."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        import os
        self.old = os.environ.pop("CVF_METRIC_NPB", None)
        if self.value is not None:
            os.environ["CVF_METRIC_NPB"] = str(self.value)

    def __exit__(self, *exc):
        import os
        os.environ.pop("CVF_METRIC_NPB", None)
        if self.old is not None:
            os.environ["CVF_METRIC_NPB"] = self.old


def abi_route(desc, B, k, with_stats, npb=None):
    """The fields of cvf_metric_route's plan as a dict."""
    import ctypes as C
    from colvarsfinder import _hip
    plan = _hip.MetricPlan()
    with _npb_env(npb):
        _hip.check(_hip.lib().cvf_metric_route(C.byref(desc), B, k, int(with_stats), C.byref(plan)), "cvf_metric_route")
    return {name: getattr(plan, name) for name, _ in plan._fields_ if name != "reserved"}


def abi_prepare(case, dev, B=None):
    """cvf_align_feature_fwd with aux and scratch on the case's first B frames (its 130 repeated when B is larger), then
    cvf_metric_dense_tensors: everything cvf_metric_apply reads besides g."""
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    B = B or case.B
    s = build(case)
    p = types.SimpleNamespace(case=case, B=B, T=n_tiles(B), layer=layer_of(case, dev))
    traj = frames(case.n, case.seed)[0]
    p.x = torch.tensor(np.resize(traj, (B,) + traj.shape[1:]) if B > len(traj) else traj[:B]).to(dev).contiguous()
    p.desc = p.layer.pp_desc()
    rows = torch.empty(B, p.layer.d_r, device=dev)
    p.aux = torch.zeros(p.T, _hip.AUX_ROWS, TILE, device=dev)
    p.slot = _hip.align_scratch(p.desc, B, dev)
    _hip.check(lib.cvf_align_feature_fwd(p.desc, P(p.x), B, None, P(rows), P(p.aux), P(p.slot), _hip.stream()), "cvf_align_feature_fwd")
    p.a = torch.tensor(s.a, device=dev)
    p.dense = None
    if case.kind == "rows":
        assert p.slot is not None, case.id
        p.dense = torch.full((lib.cvf_metric_dense_doubles(p.desc),), float("nan"), device=dev, dtype=torch.float64)
        _hip.check(lib.cvf_metric_dense_tensors(p.desc, P(p.a), P(p.dense), _hip.stream()), "cvf_metric_dense_tensors")
    torch.cuda.synchronize()
    return p


def padded(p, g, how, seed=0, g_only=False):
    """(g_tiled [T, k, d_r, 64], aux, slot_xyz) with the lanes of the padded frames filled with zeros (how = 'zero') or with finite
    garbage of magnitude ~1e3 ('garbage'); how = None: g padded with zeros, aux and slot_xyz as the forward call left them (its
    padded lanes repeat the last frame); g_only: the garbage goes into g alone."""
    dev = p.x.device
    gt = torch.tensor(to_tiled(g, p.B)).to(dev)
    n_pad = p.T * TILE - p.B
    if how is None or n_pad == 0:
        return gt, p.aux, p.slot
    fr = torch.arange(p.B, p.T * TILE, device=dev)

    def fill(shape, i):
        return torch.zeros(shape, device=dev) if how == "zero" else torch.tensor(garbage(shape, seed + i)).to(dev)

    gt[fr // TILE, :, :, fr % TILE] = fill((n_pad,) + tuple(gt.shape[1:3]), 0)
    if g_only:
        return gt, p.aux, p.slot
    aux = p.aux.clone()
    aux[fr // TILE, :, fr % TILE] = fill((n_pad, aux.shape[1]), 1)
    slot = None
    if p.slot is not None:
        slot = p.slot.clone()
        ns3 = 3 * p.desc.n_slot
        v = slot.view(torch.float32)[:p.T * TILE * ns3].view(p.T * 8, ns3, 8)      # [frame group of 8][n_slot * 3][8]
        v[fr // 8, :, fr % 8] = fill((n_pad, ns3), 2)
    return gt, aux, slot


def abi_apply(p, gt, k, aux, slot, npb=None, stats=None):
    """cvf_metric_apply, or with stats = (w [B] fp32, y_tiled [T k 64] fp32) cvf_metric_apply_stats: (q [B, k, d_r], E [B, k]) of the
    valid frames (and stats [ns] fp64).  Every output starts as NaN."""
    import ctypes as C
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    dev, nan = p.x.device, float("nan")
    q = torch.full(tuple(gt.shape), nan, device=dev)
    e = torch.full((p.T, k, TILE), nan, device=dev)
    st = None
    with _npb_env(npb):
        if stats is None:
            _hip.check(lib.cvf_metric_apply(p.desc, P(p.x), p.B, P(aux), P(p.a), k, P(gt), P(q), P(e), P(slot), P(p.dense), _hip.stream()),
                       "cvf_metric_apply")
        else:
            cfg = _hip.EFCfg()
            cfg.k, cfg.lag_idx, cfg.sort_eigvals, cfg.alpha, cfg.beta, cfg.dt = k, 0, 1, 10.0, 1.0, 1.0
            for i in range(k):
                cfg.eig_w[i] = 1.0
            w, yt = stats
            scratch = torch.full((lib.cvf_metric_stats_scratch_doubles(p.B, k),), nan, device=dev, dtype=torch.float64)
            st = torch.full((lib.cvf_ef_nstats(k, 0),), nan, device=dev, dtype=torch.float64)
            _hip.check(lib.cvf_metric_apply_stats(p.desc, P(p.x), p.B, P(aux), P(p.a), k, P(gt), P(q), P(e), P(slot), P(p.dense),
                                                  C.byref(cfg), P(w), P(yt), P(scratch), P(st), None, None, _hip.stream()),
                       "cvf_metric_apply_stats")
    torch.cuda.synchronize()
    qv = from_tiled(q.cpu().numpy(), p.B)
    ev = from_tiled(e.cpu().numpy()[:, :, None, :], p.B)[:, :, 0]
    return (qv, ev) if stats is None else (qv, ev, st.cpu().numpy())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run_and_check(case, dev):
    """One case through the C ABI: the instance the route names, q and E against the fp64 oracle at the case's bars, every valid
    lane written, the same bits on a repeated call and under garbage in the padded lanes.  Returns (plan, q error, E error)."""
    p = abi_prepare(case, dev)
    plan = abi_route(p.desc, case.B, case.k, False, case.npb)
    assert plan == expected_plan(case), (case.id, plan, expected_plan(case))
    ref = reference(case)
    g = cotangent(case, p.layer.d_r).numpy()
    gt, aux, slot = padded(p, g, "zero")
    q, E = abi_apply(p, gt, case.k, aux, slot, case.npb)
    assert q.shape == ref.q.shape and np.isfinite(q).all() and np.isfinite(E).all(), f"{case.id}: a valid output lane was not written"
    eq, eE = float(q_errors(q, ref.q).max()), float(e_errors(E, ref.E).max())
    what = f"rows<{plan['F']}, {plan['waves']}, {plan['geo_pre']}, {plan['multi']}> npb {plan['npb']}" if case.kind == "rows" else \
        f"{case.kind} nets/wg {plan['nets_per_wg']}"
    print(f"[metric] {case.id:26s} {what:32s} lds {plan['lds_bytes']:6d} records {case.n_mrec:4d} q {eq:.2e} (bar {ref.bar_q:.2e}) "
          f"E {eE:.2e} (bar {ref.bar_E:.2e})", flush=True)
    assert eq <= ref.bar_q, (case.id, eq, ref.bar_q)
    assert eE <= ref.bar_E, (case.id, eE, ref.bar_E)
    q2, E2 = abi_apply(p, gt, case.k, aux, slot, case.npb)
    assert same_bits(q, q2) and same_bits(E, E2), f"{case.id}: a repeated call gives other bits"
    if case.B % TILE:
        gt, aux, slot = padded(p, g, "garbage", seed=case.B)
        q3, E3 = abi_apply(p, gt, case.k, aux, slot, case.npb)
        assert same_bits(q, q3) and same_bits(E, E3), f"{case.id}: the padded lanes reach the valid frames"
    return plan, eq, eE
