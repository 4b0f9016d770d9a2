"""The eigenfunction step's kernel-instance sweep: its cases and, for each case, the kernel instances the host will launch.

Plain Python (no torch, no GPU).  `tests/test_ef_instances.py` (CPU) reads the instances compiled into the code objects and
checks that every one is claimed by a case here or listed in `UNREACHABLE`; `tests/test_ef_sweep_gpu.py` runs every case on
the GPU against the fp64 oracle and checks that the launches are the ones `route()` predicts.

The rules below mirror the host dispatch; the comments name the functions they copy.  If those change, change them too: the
GPU sweep's checks (`route()` against the task's own route record, `launches()` against its calls) fail when the mirror and
the host disagree.
"""

from collections import namedtuple

# ---------------------------------------------------------------------------------------------------- shapes and limits
# ef16_dispatch (csrc/ef16_common.hpp) - the 16-frames-per-wave step (ef16_front.hip, ef16_back.hip)
EF16_SHAPES = ((8, 1), (8, 2), (8, 3), (12, 1), (12, 2), (12, 3), (16, 1), (16, 2), (16, 3), (20, 1), (20, 2), (20, 3),
               (24, 2), (24, 3), (32, 2), (32, 3))
# ef_dispatch (csrc/ef_mfma.hip) - the 64-frame kernels
EF_SHAPES = EF16_SHAPES + ((48, 2), (48, 3), (64, 2), (64, 3), (20, 4), (20, 5), (32, 4), (32, 5))
FUSED_MAX_H = 32     # kFusedMaxH (ef_mfma.hip): the fused launches are instantiated up to 32 units
MAX_NETS = 8         # CVF_MAX_NETS
TILE, UNIT = 64, 16  # CVF_TILE (include/cvf.h), kU (ef16_common.hpp)
IMG_PITCH, AUX_PITCH = 76, 21   # kImgP, kAuxP (ef16_common.hpp)
SLAB_ROWS = 1024     # cvf_ef16_backward_slab_rows (ef16_back.hip)

# MIXED features of tests/test_gpu_parity.py: positions, bonds, angles and dihedrals of a 10-atom molecule (d_r = 22)
MIXED = [("position", (0, 2, 3, 5)), ("bond", (0, 1)), ("bond", (2, 7)), ("angle", (1, 2, 3)),
         ("dihedral", (0, 1, 2, 3)), ("dihedral", (4, 5, 6, 7)), ("angle", (6, 8, 9))]
MIXED_D = 22

# Instances no case of the step can reach, each with the reason; keys as in `instances()`.  Empty: every compiled instance
# of the three families is reachable from EigenFunctionTask.
UNREACHABLE = {}

# ---------------------------------------------------------------------------------------------------- cases
# mode: "gen" (lag_tau = 0) or "tr" (transfer operator, lag_tau > 0).  layout: "pos" (the first n_rec of n_atoms frame atoms as
# positions, aligned on the first n_align) or "mixed" (MIXED on n_atoms atoms, aligned on all of them).  hidden: the nets' hidden
# widths (tanh).  no_ef16: CVF_NO_EF16=1 is set.  dup: the batch is also run as two copies of itself (more than 1024 backward
# tiles: the MULTI backward instance) and must give the same loss and gradient.
Case = namedtuple("Case", "id mode n_atoms n_rec n_align layout hidden k B no_ef16 dup")

RAGGED_B = (5, 63, 65, 100, 130, 190, 257, 333, 401)   # batches that leave the last 64-frame tile (and 16-frame unit) part empty


def _nrec_options(nit):
    return [n for n in range(4 * nit - 3, 4 * nit + 1) if n >= 3]


def front16_lds_bytes(n_coord, n_align, k):
    """front16_lds(nc, nal, k).total * 4 (ef16_common.hpp; the stride: x_tile_stride, cvf_common.hpp)."""
    stride = n_coord if n_coord & 3 == 2 else n_coord | 1
    ref = UNIT * stride
    a = ref + 3 * n_align
    aux = (a + n_coord + 3) & ~3
    w = aux + ((UNIT * AUX_PITCH + 3) & ~3)
    feat = w + UNIT + 4 + 2 * k * UNIT
    return 4 * (feat + UNIT * IMG_PITCH + k * UNIT * IMG_PITCH)


def _gen_ef16_cases():
    """Generator mode on the fast layout: every (H, NH) x NIT 1..6 x ALLAL.  n_rec, n_align, trailing atoms, k and B rotate;
    NIT = 6 with ALLAL carries each shape's launch above 48 KiB of LDS (k = 7 or 8 and 21-24 recorded atoms)."""
    big = ((22, 22, 8), (24, 24, 8), (21, 26, 8), (23, 23, 8), (21, 40, 7))   # (n_rec, n_atoms, k) above 48 KiB
    out = []
    for s, (H, NH) in enumerate(EF16_SHAPES):
        for nit in range(1, 7):
            for allal in (True, False):
                j = 2 * nit + int(allal)
                opts = [n for n in _nrec_options(nit) if allal or n >= 4]
                n_rec = opts[(s + j) % len(opts)]
                n_align = n_rec if allal else 3 + (3 * s + nit) % (n_rec - 3)
                n_atoms = n_rec + (0, 0, 2, 5)[(s + nit) % 4]
                k = 1 + (5 * s + j) % MAX_NETS
                if nit == 6 and allal:
                    n_rec, n_atoms, k = big[s % len(big)]
                    n_align = n_rec
                B = RAGGED_B[(3 * s + j) % len(RAGGED_B)]
                out.append(Case(f"gen-ef16-h{H}x{NH}-nit{nit}-{'allal' if allal else 'prefix'}", "gen", n_atoms, n_rec, n_align,
                                "pos", (H,) * NH, k, B, False, False))
    return out


def _tr_ef16_cases():
    """Transfer mode on the fast layout, every (H, NH); alternately on all / a prefix of the recorded atoms."""
    out = []
    for s, (H, NH) in enumerate(EF16_SHAPES):
        n_rec = (4, 9, 14, 19, 24)[s % 5]
        n_align = n_rec if s % 2 == 0 else 3 + s % (n_rec - 3)
        out.append(Case(f"tr-ef16-h{H}x{NH}", "tr", n_rec + s % 3, n_rec, n_align, "pos", (H,) * NH, 1 + (3 * s) % MAX_NETS,
                        RAGGED_B[s % len(RAGGED_B)], False, False))
    return out


def _multi_cases():
    """The MULTI backward instances, every (H, NH) in both modes: a batch just past half of 1024 backward tiles, checked
    against the oracle, then as two copies of itself (gen: T > 1024 is B > 65 536 frames; tr: 2 T > 1024 is B > 32 768)."""
    out = []
    for s, (H, NH) in enumerate(EF16_SHAPES):
        n_rec = (9, 16, 22, 6)[s % 4]
        n_align = n_rec if s % 3 else n_rec - 2
        k = 1 + (3 * s + 1) % 4
        out.append(Case(f"gen-multi-h{H}x{NH}", "gen", n_rec, n_rec, n_align, "pos", (H,) * NH, k, 32_768 + 1 + 97 * s, False, True))
        out.append(Case(f"tr-multi-h{H}x{NH}", "tr", n_rec + 1, n_rec, n_align, "pos", (H,) * NH, k, 16_384 + 5 + 61 * s, False, True))
    return out


def _plain_cases():
    """The 64-frame kernels on the plain layout (mixed features: align + features, forward, [metric,] backward launches), every
    (H, NH) of ef_dispatch in both modes."""
    out = []
    for s, (H, NH) in enumerate(EF_SHAPES):
        for mode in ("gen", "tr"):
            j = 2 * s + (mode == "tr")
            out.append(Case(f"{mode}-mixed-h{H}x{NH}", mode, 10 + s % 3, 0, 0, "mixed", (H,) * NH, 1 + j % MAX_NETS,
                            RAGGED_B[j % len(RAGGED_B)], False, False))
    return out


def _fused_cases():
    """The fused 64-frame launches (CVF_NO_EF16=1, what CVF_PIPELINE=1 runs on): every (H <= 32, NH) of ef_dispatch through
    ef_fwd_metric_kernel (gen; with the alignment folded in from 10 atoms) and ef_align_fwd_kernel (tr)."""
    out = []
    for s, (H, NH) in enumerate(sh for sh in EF_SHAPES if sh[0] <= FUSED_MAX_H):
        for mode in ("gen", "tr"):
            n_rec = (7, 10, 16, 22)[s % 4] if mode == "gen" else (10, 13, 18, 24)[s % 4]
            n_align = n_rec if s % 2 else max(3, n_rec - 4)
            n_atoms = n_rec + (0, 3)[s % 2]
            k = 1 + (s + 3 * (mode == "tr")) % 4
            while fwd_metric_lds_bytes(3 * n_atoms, n_align, k) > 80 * 1024:   # (else the step takes the plain launches)
                k -= 1
            out.append(Case(f"{mode}-fused-h{H}x{NH}", mode, n_atoms, n_rec, n_align, "pos", (H,) * NH, k,
                            RAGGED_B[(s + 4) % len(RAGGED_B)], True, False))
    return out


# ---------------------------------------------------------------------------------------------------- the host's rules


def d_r(case):
    return MIXED_D if case.layout == "mixed" else 3 * case.n_rec


def shape(case):
    """(H, NH) of the nets; the cases use kernel widths only (no zero padding: _FlatParams._init_padded)."""
    H = case.hidden[0]
    assert all(h == H for h in case.hidden), case
    return H, len(case.hidden)


def _pos_fast(case):
    # CVF_PP_ALIGN_CONTIG | CVF_PP_PURE_POSITION (AlignFeatureLayer.pp_desc): aligned on atoms 0..n_align-1, positions of atoms 0..n_rec-1
    return case.layout == "pos"


def ef16_supported(case):
    """cvf_ef16_supported (ef16_front.hip) and the ef16 row of EigenFunctionTask._route."""
    H, NH = shape(case)
    nc = 3 * case.n_atoms
    return (not case.no_ef16 and NH <= 3 and (H, NH) in EF16_SHAPES and _pos_fast(case)
            and 3 <= case.n_align <= case.n_rec and d_r(case) <= 72 and d_r(case) <= nc <= 192 and 1 <= case.k <= MAX_NETS
            and front16_lds_bytes(nc, case.n_align, case.k) <= 64 * 1024)


def fwd_metric_lds_bytes(n_coord, n_align, k):
    """fwd_metric_lds (ef_mfma.hip)."""
    stride = n_coord if n_coord & 3 == 2 else n_coord | 1
    head = (TILE * stride + 3 * n_align + n_coord + 3) & ~3
    return 4 * (head + k * n_coord * TILE + k * TILE)


def _saved_floats_ok(case):
    """cvf_ef_saved_floats(mlp, 1) > 0 for H <= 32 (ef_mfma.hip): fwd_wg_ok (ef_mfma.hip; pack_layout: cvf_pack.hpp) or a first
    layer wider than kWideD = 128."""
    H, NH = shape(case)
    D = d_r(case)
    ng, s1, ct = (H + 3) // 4, (D + 3) // 4, (D + 15) // 16
    rt = (ng + 3) // 4
    return (s1 * rt + 2 * (NH - 1) * ng * rt + ct * ng) * 64 * 4 <= 64 * 1024 or D > 128


def fwd_metric_supported(case):
    """cvf_ef_fwd_metric_supported (ef_mfma.hip)."""
    H, NH = shape(case)
    nc = 3 * case.n_atoms
    return (H <= FUSED_MAX_H and _pos_fast(case) and case.n_align <= case.n_rec and d_r(case) <= 72 and nc <= 192
            and fwd_metric_lds_bytes(nc, case.n_align, case.k) <= 80 * 1024 and _saved_floats_ok(case))


def route(case):
    """'ef16', 'fused' (gen: cvf_ef_[align_]fwd_metric_stats; tr: cvf_ef_align_fwd) or 'plain': `kind` of the task's route record
    (EigenFunctionTask._route), which the GPU sweep compares with this."""
    if ef16_supported(case):
        return "ef16"
    if fwd_metric_supported(case) and (case.mode == "gen" or 3 * case.n_atoms >= 30):   # tr: cvf_ef_align_fwd_metric_supported
        return "fused"
    return "plain"


def launches(case):
    """The C-ABI calls (EigenFunctionTask._call names) of one loss_func + backward: the _fwd_* method of the route, the rule at the
    end of EigenFunctionTask._forward, and _backward (tests/test_ef_routes_gpu.py pins their order and counts)."""
    r, gen = route(case), case.mode == "gen"
    if r == "ef16":
        return {"cvf_ef16_front", "cvf_ef16_finish", "cvf_ef16_backward", "cvf_slab_reduce"} if gen else \
               {"cvf_ef16_front_transfer", "cvf_ef16_finish", "cvf_ef16_backward_transfer", "cvf_slab_reduce"}
    if r == "fused" and gen:
        k1 = 3 * case.n_atoms >= 30   # cvf_ef_align_fwd_metric_supported
        return {"cvf_ef_align_fwd_metric_stats" if k1 else "cvf_ef_fwd_metric_stats", "cvf_ef_stats_finish_rows", "cvf_ef_backward",
                "cvf_slab_reduce"} | (set() if k1 else {"cvf_align_feature_fwd"})
    if r == "fused":
        return {"cvf_ef_align_fwd", "cvf_ef_stats", "cvf_ef_backward", "cvf_slab_reduce"}
    return {"cvf_align_feature_fwd", "cvf_ef_mlp_fwd", "cvf_metric_apply" if gen else "cvf_ef_stats", "cvf_ef_backward",
            "cvf_slab_reduce"}


def n_tiles(B):
    return (B + TILE - 1) // TILE


def instances(case, B=None):
    """The instances of the three families one step of `case` (at batch B, default case.B) launches:
    ("ef16_front_kernel", H, NH, NIT, ALLAL), ("ef16_back_kernel", H, NH, MULTI, GEN) and (family, H, NH) of the 64-frame kernels
    ef_bwd_mfma_kernel, ef_fwd_metric_kernel and ef_align_fwd_kernel."""
    B = case.B if B is None else B
    H, NH = shape(case)
    gen, r = case.mode == "gen", route(case)
    if r == "ef16":
        # front: NIT = ceil(n_rec / 4), ALLAL = (n_align == n_rec) (cvf_ef16_front); transfer: <H, NH, 0, true> (ef16_front_transfer_impl)
        front = ("ef16_front_kernel", H, NH, (case.n_rec + 3) // 4, int(case.n_align == case.n_rec)) if gen else \
                ("ef16_front_kernel", H, NH, 0, 1)
        # back: MULTI when the backward tiles (T, or 2 T with the lagged partners) outnumber the 1024 slab rows (cvf_ef16_backward[_transfer])
        tiles = n_tiles(B) if gen else 2 * n_tiles(B)
        return {front, ("ef16_back_kernel", H, NH, int(tiles > SLAB_ROWS), int(gen))}
    out = {("ef_bwd_mfma_kernel", H, NH)}                       # cvf_ef_backward
    if r == "fused":
        out.add(("ef_fwd_metric_kernel", H, NH) if gen else ("ef_align_fwd_kernel", H, NH))   # fwd_metric_launch, cvf_ef_align_fwd
    return out


def claimed():
    """Every instance some case launches (dup cases: at B and at 2 B)."""
    out = set()
    for c in CASES:
        out |= instances(c)
        if c.dup:
            out |= instances(c, 2 * c.B)
    return out


CASES = _gen_ef16_cases() + _tr_ef16_cases() + _multi_cases() + _plain_cases() + _fused_cases()
