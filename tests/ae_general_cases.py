"""The per-layer autoencoder step (csrc/ae_general.hip, cvf_ae_general_step): its cases, the Python mirror of its workspace
formula and the error bars the GPU module holds it to.

Plain Python at import (no torch, no GPU).  `tests/test_ae_general_host.py` (CPU) checks the mirror against the library and ties
the bars to the fp32 CPU oracle; `tests/test_ae_general_gpu.py` runs every case through the C entry against the fp64 oracle.

The C entry takes any chain, small ones too, so the edges of its kernels - the 64-row output block and the 32-deep K stage of
aeg_layer_kernel, the 64 x 64 blocks of aeg_wgrad_kernel, the last tile's padding, the slab-row wrap - are met at the smallest
shapes that reach them.  A case with a gradient is either a chain cvf_ae_step refuses (the route's reason to exist) or is
listed in SMALL with the reason a small shape is used.
"""
from tests import ae_cases as A

Case = A.Case
TILE = A.TILE
MAX_ROWS = 256                # kMaxRows
SLAB_BYTES = 128 << 20        # kSlabBytes
MAX_WIDTH, MAX_D0 = 4096, 65536


def _case(id, e_dims, d_dims, B, act="tanh", idx=False, grad=True, misaligned=False, dup=False, adam=False):
    return Case(id, tuple(e_dims), tuple(d_dims), act, B, idx, grad, False, misaligned, dup, adam)


BIG_E, BIG_D = [384, 256, 64, 2], [2, 64, 256, 384]          # an autoencoder on the 384 features of the large-molecule shape
DIP_E, DIP_D = [66, 128, 128, 2], [2, 128, 128, 66]          # the dipeptide autoencoder: 200 KB of parameters
HUGE_E, HUGE_D = [120, 56, 24, 3], [3, 24, 56, 120]          # ae_cases' "mfma-tanh-refused": 164 144 B of LDS with its gradient
CAP_E, CAP_D = [384, 170, 2], [2, 170, 384]                  # 131 966 parameters: 254 slab rows fit 128 MiB, not 256
MANY_B = 64 * MAX_ROWS + 37                                  # 257 tiles on 256 slab rows: row 0 sums tiles 0 and 256
CAP_B = 64 * 254 + 64 + 5                                    # 256 tiles on 254 slab rows: rows 0 and 1 sum two tiles each

CASES = [
    # ---- hidden widths at the edges of the 64-row block and the 32-deep K stage, d0 in {1, 3, 67, 384}, every activation,
    #      batches 1, 63, 64, 65, 130, 257, with and without the gather
    _case("width-1", [3, 1, 2], [2, 1, 3], 1),
    _case("width-31-sigmoid", [67, 31, 2], [2, 31, 67], 63, act="sigmoid", idx=True),
    _case("width-32-relu", [67, 32, 3], [3, 32, 67], 64, act="relu"),
    _case("width-33-elu", [3, 33, 2], [2, 33, 3], 65, act="elu", idx=True),
    _case("width-63-leaky", [67, 63, 2], [2, 63, 67], 130, act="leaky_relu"),
    _case("width-64-softplus", [67, 64, 2], [2, 64, 67], 257, act="softplus", idx=True),
    _case("width-65-d0-1", [1, 65, 1], [1, 65, 1], 130),
    _case("width-65-d0-1-B-64", [1, 65, 1], [1, 33, 1], 64, idx=True),
    _case("width-130", [67, 130, 3], [3, 130, 67], 257, idx=True, adam=True),
    _case("d0-384", [384, 65, 2], [2, 33, 384], 65),
    _case("d0-384-B-1", [384, 65, 2], [2, 33, 384], 1, idx=True),
    # ---- depth
    _case("one-hidden-layer", [3, 5], [5, 3], 63),
    _case("one-hidden-layer-wide", [384, 130], [130, 384], 65, idx=True),
    _case("twelve-layers", [30, 17, 13, 9, 5, 3, 2], [2, 3, 5, 9, 13, 17, 30], 130, idx=True, adam=True),
    # ---- more tiles than slab rows
    _case("many-tiles", [3, 5, 2], [2, 5, 3], MANY_B, idx=True, dup=True),
    _case("slab-capped", CAP_E, CAP_D, CAP_B),
    # ---- the chains the route exists for
    _case("large-molecule", BIG_E, BIG_D, 130, idx=True),
    _case("large-molecule-softplus", BIG_E, BIG_D, 65, act="softplus"),
    _case("dipeptide", DIP_E, DIP_D, 257),
    _case("dipeptide-elu-B-1001", DIP_E, DIP_D, 1001, act="elu", idx=True),
    _case("refused-by-the-fused-step", HUGE_E, HUGE_D, 65),
    _case("refused-relu", HUGE_E, HUGE_D, 190, act="relu", idx=True),
    _case("misaligned", HUGE_E, HUGE_D, 63, idx=True, misaligned=True),
    _case("misaligned-dipeptide", DIP_E, DIP_D, 64, misaligned=True),
    # ---- loss only
    _case("loss-large-molecule", BIG_E, BIG_D, 130, grad=False),
    _case("loss-width-33", [3, 33, 2], [2, 33, 3], 65, act="sigmoid", idx=True, grad=False),
    _case("loss-B-1001", [67, 31, 2], [2, 31, 67], 1001, idx=True, grad=False),
    _case("loss-B-1", DIP_E, DIP_D, 1, grad=False),
]

# The `adam` cases (three fused Adam steps against the fp64 oracle's, at the sweep's ADAM_TOL = 2e-6) are cases whose fp32 CPU
# oracle itself stays within ADAM_TOL / 8 of the fp64 oracle after those steps (tests/test_ae_general_host.py recomputes it).
# That excludes chains with gradient entries next to zero: Adam's first updates are lr g / (|g| + eps), so an entry whose
# gradient is of the size of Adam's eps = 1e-8 or of fp32 rounding moves by a different fraction of lr = 1e-3 in ANY fp32
# evaluation - on "large-molecule" (230 658 parameters, entries down to 1e-9 of the largest) torch's own fp32 steps on the
# CPU end 1.3e-4 from the fp64 ones, sixty times the bar, so that chain's update is covered by its gradient check instead.
ADAM_SOURCE_MAX = 2e-6 / 8

# Cases with a gradient that cvf_ae_step would take too, and why the small shape is used
_EDGE = "a hidden width at an edge of aeg_layer_kernel's 64-row block / 32-deep K stage, at the smallest chain that has it"
SMALL = {
    "width-1": _EDGE, "width-31-sigmoid": _EDGE, "width-32-relu": _EDGE, "width-33-elu": _EDGE, "width-63-leaky": _EDGE,
    "width-64-softplus": _EDGE, "width-65-d0-1": _EDGE + " (d0 = 1: one-column operands)", "width-65-d0-1-B-64": _EDGE,
    "one-hidden-layer": "the shallowest chain: one forward pair, one backward product",
    "twelve-layers": "CVF_MAX_LAYERS layers; narrow, so that the fp64 oracle of twelve layers stays cheap",
    "many-tiles": "257 tiles on 256 slab rows needs 16 421 frames: the chain is tiny so that the case takes no time",
}


def dims(case):
    return A.dims(case)


def group(case):
    """The group whose error bar the case is held to, as ae_cases.group: the route x (B < 1000 | B >= 1000)."""
    return "general", "small" if case.B < 1000 else "large"


# ---------------------------------------------------------------------------------------------------- the host's rules
def n_tiles(B):
    return (B + TILE - 1) // TILE


def slab_rows(d, B):
    """g64_rows (csrc/cvf_gemm64.hpp): min(tiles, 256, 128 MiB / (4 n_params)), at least 1."""
    return max(1, min(n_tiles(B), MAX_ROWS, SLAB_BYTES // (4 * A.n_params(d))))


def scratch_floats(d, B):
    """aeg_layout: the tiled input and the saved activations a_1..a_{L-1}, two adjoint images as wide as the widest of
    dims[1..L], the slab rows, (rounded up to even) two doubles per tile."""
    T = n_tiles(B)
    images = T * TILE * (sum(d[:-1]) + 2 * max(d[1:]))
    return ((images + slab_rows(d, B) * A.n_params(d) + 1) & ~1) + 4 * T


def supported(d):
    """aeg_why for a chain built by ae_inputs.mlp_desc (one net, valid activation codes, parameters filling the buffer)."""
    L = len(d) - 1
    blocks = lambda l: ((d[l + 1] + 63) // 64) * ((d[l] + 1 + 63) // 64)   # aeg_wgrad_kernel's grid.y for layer l
    return (1 <= L <= A.MAX_LAYERS and d[0] == d[L] and 1 <= d[0] <= MAX_D0 and all(1 <= h <= MAX_WIDTH for h in d[1:L])
            and all(blocks(l) <= 65535 for l in range(L)))


# ---------------------------------------------------------------------------------------------------- error bars
def group_e32(cases=None):
    """{group: [worst loss e32, worst gradient e32]}: ae_inputs.group_e32's rule (a loss-only case enters with its loss alone)
    under this module's groups - ae_inputs.group_e32 itself keys by cvf_ae_step's route and skips the chains that route
    refuses, which are the ones this table is about."""
    from tests import ae_inputs as I
    worst = {}
    for c in CASES if cases is None else cases:
        e = I.e32(c)
        w = worst.setdefault(group(c), [0.0, 0.0])
        w[0] = max(w[0], e[0])
        if c.grad:
            w[1] = max(w[1], e[1])
    return worst


# group -> (loss, relative; gradient, largest entry error over the largest entry): EIGHT TIMES the worst distance of the fp32 CPU
# oracle (ae_inputs.oracle_fp32, tile by tile) from the fp64 oracle over the group's cases, rounded up to two digits - the rule of
# ae_cases.BARS, measured against the oracle, never against the kernels.  tests/test_ae_general_host.py recomputes the maxima
# and holds every bar between 4 and 16 times its source.
BARS = {("general", "small"): (7.1e-7, 2.9e-6), ("general", "large"): (1.4e-7, 4.8e-7)}
