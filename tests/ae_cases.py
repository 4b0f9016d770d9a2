"""The autoencoder step's kernel-instance sweep: its cases and, for each case, the kernel and LDS layout the host will launch.

Plain Python (no torch, no GPU).  `tests/test_ae_instances.py` (CPU) reads the instances compiled into ae.o and checks that
every one is claimed by a case here or listed in `UNREACHABLE`, and compares `route()` with the library's own
cvf_ae_step_route(); `tests/test_ae_sweep_gpu.py` runs every case on the GPU against the fp64 oracle.

The rules below mirror the host code of csrc/ae.hip; the comments cite the functions they copy.  If the C++ changes, change
them too: the comparison with cvf_ae_step_route() fails when the mirror and the host disagree.
"""

from collections import namedtuple

# ---------------------------------------------------------------------------------------------------- limits
TILE = 64            # CVF_TILE (include/cvf.h)
MAX_LAYERS = 12      # CVF_MAX_LAYERS
AP = 68              # image pitch of both kernels (ae.hip: AP)
AE16_PAD = 576       # kAe16Pad: the zero pad behind theta's LDS copy
MAX_BLOCKS = 2048    # kAeMaxBlocks: ae_grid / regae_grid
AE16_LDS_MAX = 80 * 1024     # ae16_shape: two workgroups per CU
MFMA_HALF = 80 * 1024 - 1024   # ae_mlayout: kHalf
MFMA_LDS_MAX = 160 * 1024    # cvf_ae_step_route: refused above
OPT_IN_LDS = 48 * 1024       # above: the hipFuncSetAttribute branch
# ae16_dispatch: (RTD, RTH) = (ceil(d0 / 16), ceil(hmax / 16))
AE16_INSTANCES = tuple((d, h) for h in (1, 2) for d in (1, 2, 3, 4, 5))
ACTS = ("tanh", "sigmoid", "relu", "elu", "leaky_relu", "softplus")   # CVF_ACT_* 1..6, colvarsfinder/nn.py:_act_code

# Instances no case can reach, each with the reason; keys as in `instances()`.  Empty: all ten ae16_kernel<RTD, RTH> and both
# ae_mfma_kernel<TANH> are reachable from cvf_ae_step.
UNREACHABLE = {}

# ---------------------------------------------------------------------------------------------------- cases
# e_dims / d_dims: encoder and decoder widths (e_dims[-1] == d_dims[0]; the chain is e_dims + d_dims[1:], no activation after
# the encoder's and the decoder's last layer, nn.py:46-62).  act: name in ACTS.  B: frames.  idx: the frames are gathered from
# a longer feature trajectory through an index vector (train()), else idx = NULL (weighted_MSE_loss()).  grad: the gradient is
# asked for (else the loss-only launch of a test epoch).  no_ae16: CVF_NO_AE16=1 is set.  misaligned: theta starts 4 bytes
# into a 16-byte line.  dup: the batch is also run as two copies of itself (a loss-only case: the loss alone).  adam: three fused Adam steps are run too.
Case = namedtuple("Case", "id e_dims d_dims act B idx grad no_ae16 misaligned dup adam")


def _case(id, e_dims, d_dims, B, act="tanh", idx=False, grad=True, no_ae16=False, misaligned=False, dup=False, adam=False):
    return Case(id, tuple(e_dims), tuple(d_dims), act, B, idx, grad, no_ae16, misaligned, dup, adam)


RAGGED_B = (5, 63, 65, 130, 190, 257, 333, 401, 1001, 1500)   # batches whose last 64-frame tile is part empty
BIG_B = 140_001      # 2188 tiles on 2048 blocks: blocks 0..139 walk two tiles, the last tile holds 33 frames


def _instance_cases():
    """Every ae16_kernel<RTD, RTH> twice: [d0, h, 2, h, d0] with d0 = 16 RTD - 3, h = 16 RTH - 5 (no width a multiple of 4) on a
    ragged batch, and an asymmetric chain of full tiles' widths (d0 = 16 RTD, a 16 RTH-wide and narrower layers; one layer
    fewer where five would pass 80 KiB)."""
    full = {(4, 2): ([64, 32, 9, 3], [3, 30, 64]), (5, 2): ([80, 32, 3], [3, 30, 80])}   # 79 104 B and 81 408 B
    out = []
    for s, (rtd, rth) in enumerate(AE16_INSTANCES):
        d0, h = 16 * rtd - 3, 16 * rth - 5
        out.append(_case(f"ae16-inst-{rtd}x{rth}-odd", [d0, h, 2], [2, h, d0], RAGGED_B[s], idx=bool(s % 2)))
        d0, h = 16 * rtd, 16 * rth
        e, d = full.get((rtd, rth), ([d0, h, h - 7, 3], [3, h - 2, d0]))
        out.append(_case(f"ae16-inst-{rtd}x{rth}-full", e, d, RAGGED_B[(s + 3) % len(RAGGED_B)] + 1000 * (s % 2),
                         idx=not s % 2, grad=s % 5 != 4))
    return out


def _edge_cases():
    """Widths, depths, LDS sizes and batches at the edges of ae16_kernel."""
    c2e, c2d = [66, 20, 20, 20, 2], [2, 10, 10, 66]   # BASELINE config 2: 78 848 B of LDS, 3 KiB under the 80 KiB line
    return [
        _case("ae16-edge-d0-1", [1, 3, 1], [1, 3, 1], 63),
        _case("ae16-edge-d0-2", [2, 7, 1], [1, 5, 2], 64, idx=True),
        _case("ae16-edge-d0-16", [16, 9, 2], [2, 16, 16], 65),
        _case("ae16-edge-d0-17", [17, 17, 2], [2, 17, 17], 130, idx=True),
        _case("ae16-edge-d0-77", [77, 31, 3], [3, 30, 77], 401),
        _case("ae16-edge-d0-80", [80, 20, 4], [4, 17, 80], 257, idx=True),
        _case("ae16-edge-hidden-1", [30, 1, 1], [1, 1, 30], 130),
        _case("ae16-edge-hidden-31", [33, 31, 2], [2, 31, 33], 333, idx=True),
        _case("ae16-edge-hidden-32", [20, 32, 32, 2], [2, 32, 20], 190),
        _case("ae16-edge-2-layers", [45, 1], [1, 45], 65, idx=True),
        _case("ae16-edge-2-layers-wide", [80, 32], [32, 80], 1500),
        _case("ae16-edge-12-layers", [30, 17, 13, 9, 5, 3, 2], [2, 3, 5, 9, 13, 17, 30], 333, adam=True),
        _case("ae16-edge-12-layers-66", [66, 12, 10, 8, 6, 4, 1], [1, 4, 6, 8, 10, 12, 66], 257, idx=True),
        _case("ae16-edge-config2", c2e, c2d, 20_000 - 37, idx=True, dup=True, adam=True),
        _case("ae16-edge-config2-loss", c2e, c2d, 1001, grad=False),
        _case("ae16-edge-over-80k", [80, 32, 4], [4, 32, 80], 401),                          # 83 968 B as ae16: mfma_tanh
        _case("ae16-edge-B-1", [9, 8, 8, 1], [1, 8, 9], 1),
        _case("ae16-edge-B-1-idx", [30, 32, 3], [3, 32, 30], 1, idx=True),
        _case("ae16-edge-B-5", [30, 32, 3], [3, 32, 30], 5, idx=True, dup=True),
        _case("ae16-edge-B-63-loss", [9, 8, 8, 1], [1, 8, 9], 63, idx=True, grad=False),
        _case("ae16-edge-B-64", [66, 20, 2], [2, 20, 66], 64),
        _case("ae16-edge-B-65-loss", [66, 20, 2], [2, 20, 66], 65, grad=False),
        _case("ae16-edge-B-130", [13, 5, 2], [2, 6, 13], 130, idx=True, adam=True),
        _case("ae16-edge-B-big", [13, 10, 2], [2, 10, 13], BIG_B, dup=True),
        _case("ae16-edge-B-big-idx-loss", [21, 8, 1], [1, 8, 21], BIG_B + 7, idx=True, grad=False, dup=True),
    ]


def _mfma_cases():
    """ae_mfma_kernel<TANH = true / false> x {roomy, tight} x {with gradient, loss only}, its LDS edges and the fallbacks
    of cvf_ae_step that lead to it."""
    wide_e, wide_d = [80, 32, 32, 3], [3, 32, 32, 80]   # 126 976 B as ae16: leaves it; 97 744 B roomy / 87 504 B tight -> roomy
    tight_e, tight_d = [100, 24, 24, 3], [3, 24, 24, 100]
    huge_e, huge_d = [120, 56, 24, 3], [3, 24, 56, 120]
    out = [
        # fallbacks from an ae16 shape
        _case("mfma-tanh-misaligned", [30, 32, 3], [3, 32, 30], 130, misaligned=True),
        _case("mfma-tanh-misaligned-config2", [66, 20, 20, 20, 2], [2, 10, 10, 66], 1001, idx=True, misaligned=True),
        _case("mfma-tanh-no-ae16", [13, 11, 2], [2, 11, 13], 65, no_ae16=True),               # theta < 32 AP floats: zero tail
        _case("mfma-tanh-no-ae16-loss", [66, 20, 2], [2, 20, 66], 63, idx=True, grad=False, no_ae16=True),
        _case("mfma-tanh-hidden-33", [30, 33, 2], [2, 33, 30], 5),
        _case("mfma-tanh-d0-81", [81, 20, 2], [2, 20, 81], 190, idx=True),
        # layouts
        _case("mfma-tanh-roomy-old40", [66, 20, 2], [2, 40, 66], 20_000, idx=True, dup=True, adam=True),
        _case("mfma-tanh-roomy-wide", wide_e, wide_d, 333),
        _case("mfma-tanh-roomy-loss", [66, 20, 2], [2, 40, 66], 257, idx=True, grad=False),
        _case("mfma-tanh-tight", tight_e, tight_d, 401, idx=True, adam=True),                  # 77 600 B tight (roomy: over 79 KiB)
        _case("mfma-tanh-tight-B-64", tight_e, tight_d, 64),
        _case("mfma-tanh-tight-loss", wide_e, wide_d, 130, grad=False),                        # 78 800 B tight
        _case("mfma-tanh-roomy-max-loss", huge_e, huge_d, 63, grad=False),                     # 146 736 B
        _case("mfma-tanh-B-1", [40, 33, 1], [1, 33, 40], 1, idx=True),
        _case("mfma-tanh-B-big", [36, 6, 2], [2, 6, 36], BIG_B + 20, idx=True, dup=True, no_ae16=True),
        _case("mfma-tanh-hidden-40-B-1001", [30, 40, 3], [3, 40, 30], 1001, idx=True),
        _case("mfma-tanh-d0-96-B-2049", [96, 48, 2], [2, 48, 96], 2049),
        _case("mfma-tanh-no-ae16-B-4097-loss", [45, 16, 4], [4, 16, 45], 4097, idx=True, grad=False, no_ae16=True),
        _case("mfma-tanh-refused", huge_e, huge_d, 65),                                        # 164 144 B with its gradient
    ]
    for s, act in enumerate(ACTS[1:]):
        out.append(_case(f"mfma-any-{act}", [30, 20, 12, 2], [2, 10, 30], RAGGED_B[s + 2], act=act, idx=bool(s % 2)))
    out += [
        _case("mfma-any-small-loss", [9, 8, 1], [1, 8, 9], 63, act="relu", grad=False),         # zero tail, under 48 KiB
        _case("mfma-any-roomy-wide", wide_e, wide_d, 190, act="elu", idx=True),
        _case("mfma-any-roomy-loss", [66, 20, 2], [2, 40, 66], 65, act="softplus", grad=False),
        _case("mfma-any-tight", tight_e, tight_d, 257, act="sigmoid"),
        _case("mfma-any-tight-loss", wide_e, wide_d, 333, act="leaky_relu", idx=True, grad=False),
        _case("mfma-any-B-1500", [66, 20, 20, 20, 2], [2, 10, 10, 66], 1500, act="elu", idx=True, adam=True),
        _case("mfma-any-B-64", [17, 5, 2], [2, 5, 17], 64, act="softplus"),
        _case("mfma-any-relu-B-1001", [30, 20, 12, 2], [2, 10, 30], 1001, act="relu"),
        _case("mfma-any-softplus-B-2049", [66, 20, 2], [2, 40, 66], 2049, act="softplus", idx=True),
        _case("mfma-any-sigmoid-B-5000-loss", [12, 40, 1], [1, 40, 12], 5000, act="sigmoid", grad=False),
        _case("mfma-any-B-big-loss", [10, 6, 2], [2, 6, 10], BIG_B + 3, act="sigmoid", grad=False, dup=True),
        _case("mfma-any-B-big", [10, 6, 2], [2, 6, 10], BIG_B + 11, act="elu", idx=True, dup=True),
    ]
    return out


CASES = _instance_cases() + _edge_cases() + _mfma_cases()

# ---------------------------------------------------------------------------------------------------- the host's rules


def dims(case):
    assert case.e_dims[-1] == case.d_dims[0], case
    return list(case.e_dims) + list(case.d_dims[1:])


def acts(case):
    """cvf_mlp_desc.act: the activation's code after every layer but the encoder's and the decoder's last."""
    d, code = dims(case), ACTS.index(case.act) + 1
    return [0 if l in (len(case.e_dims) - 2, len(d) - 2) else code for l in range(len(d) - 1)]


def n_params(d):
    return sum(d[l] * d[l + 1] + d[l + 1] for l in range(len(d) - 1))


def _up16(n):
    return (n + 15) & ~15


def ae16_lds_bytes(d):
    """ae16_layout(m).total * 4: images a_1..a_{L-1} (d_l + 1 rows), zbar_1..zbar_L (d_l rows), theta + the zero pad."""
    L = len(d) - 1
    rows = sum(d[l] + 1 for l in range(1, L)) + sum(d[l] for l in range(1, L + 1))
    wfl = ((n_params(d) + 3) & ~3) + AE16_PAD
    return 4 * (rows * AP + max(wfl, 16 * AP))


def ae16_shape(d, act):
    """ae16_shape: one tanh chain of 2..12 layers, d0 = dL <= 80, hidden widths 1..32, at most 80 KiB of LDS."""
    L = len(d) - 1
    return (2 <= L <= MAX_LAYERS and d[0] <= 80 and d[0] == d[L] and all(1 <= h <= 32 for h in d[1:L]) and act == "tanh"
            and ae16_lds_bytes(d) <= AE16_LDS_MAX)


def ae16_instance(d):
    """ae16_dispatch: (RTD, RTH), or None when that pair is not compiled."""
    key = ((d[0] + 15) // 16, (max(d[1:-1], default=1) + 15) // 16)
    return key if key in AE16_INSTANCES else None


def _mfma_layout_of(d, with_grad, tight):
    """ae_mlayout_of: (total floats, skip0, has_zero_tail)."""
    L = len(d) - 1
    rows = sum(d[l] + 1 for l in range(1, L))
    dh = max([1] + d[1:L])
    dall = max([1] + d[1:L + 1])
    zb_rows = dall if tight else _up16(dall)
    ab_rows = (dh if tight else _up16(dh)) if with_grad else 0
    skip0 = d[0] * d[1] if tight else 0           # (the flat buffer starts with the first layer's weights: w_off[0][0] == 0)
    np4 = (n_params(d) - skip0 + 3) & ~3
    w_off = (rows + zb_rows + ab_rows) * AP
    return w_off + max(np4, 32 * AP), skip0, np4 < 32 * AP


def mfma_layout(d, with_grad):
    """ae_mlayout: ("roomy" | "tight", lds_bytes, skip0, has_zero_tail) - roomy unless only the tight one fits 79 KiB."""
    roomy = _mfma_layout_of(d, with_grad, False)
    if 4 * roomy[0] <= MFMA_HALF:
        return ("roomy", 4 * roomy[0]) + roomy[1:]
    tight = _mfma_layout_of(d, with_grad, True)
    return ("tight", 4 * tight[0]) + tight[1:] if 4 * tight[0] <= MFMA_HALF else ("roomy", 4 * roomy[0]) + roomy[1:]


def n_tiles(B):
    return (B + TILE - 1) // TILE


def grid(B):
    """ae_grid (regae_grid takes the tile count: T or 2 T): (blocks, most tiles one block walks)."""
    T = n_tiles(B)
    G = min(T, MAX_BLOCKS)
    return G, (T + G - 1) // G


def scratch_floats(d, B):
    """cvf_ae_scratch_floats: slab rows + two doubles per block."""
    G = grid(B)[0]
    return G * n_params(d) + 4 * G + 4


def uses_ae16(case):
    """cvf_ae_step_route's first branch."""
    d = dims(case)
    return not case.no_ae16 and ae16_shape(d, case.act) and not case.misaligned and ae16_instance(d) is not None


def lds_bytes(case):
    return ae16_lds_bytes(dims(case)) if uses_ae16(case) else mfma_layout(dims(case), case.grad)[1]


def route(case):
    """cvf_ae_step_route: 'ae16', 'mfma_tanh' / 'mfma_any' (chain_is_tanh picks the template value) or 'refused'."""
    if uses_ae16(case):
        return "ae16"
    if lds_bytes(case) > MFMA_LDS_MAX:
        return "refused"
    return "mfma_tanh" if case.act == "tanh" else "mfma_any"


def route_code(case):
    """What cvf_ae_step_route returns: 0 ae16, 1 / 2 ae_mfma_kernel roomy / tight, -1 refused."""
    r = route(case)
    return 0 if r == "ae16" else -1 if r == "refused" else 1 + (mfma_layout(dims(case), case.grad)[0] == "tight")


def group(case):
    """The group whose error bar the case is held to: route x (B < 1000 | B >= 1000)."""
    return route(case), "small" if case.B < 1000 else "large"


def instances(case):
    """{("ae16_kernel", RTD, RTH)} or {("ae_mfma_kernel", TANH)}; nothing for a refused chain."""
    r = route(case)
    if r == "ae16":
        return {("ae16_kernel",) + ae16_instance(dims(case))}
    return set() if r == "refused" else {("ae_mfma_kernel", int(r == "mfma_tanh"))}


def claimed():
    out = set()
    for c in CASES:
        out |= instances(c)
    return out


# ---------------------------------------------------------------------------------------------------- error bars
# group -> (loss, relative; gradient, largest entry error over the largest entry).  EIGHT TIMES the worst distance of the fp32
# CPU oracle (evaluated tile by tile, tests/ae_inputs.py: oracle_fp32) from the fp64 oracle over the group's cases
# (group_e32), rounded up to two digits - derived
# from the reference, never from what the kernels achieve.  tests/test_ae_instances.py recomputes the maxima and holds every
# bar between 4 and 16 times its source.  The margin covers what separates the kernels from that reference: the summation
# order (64-frame tiles, slab rows, a fixed-order sum), cvf_tanh against libm's tanh, fp32 accumulation in the MFMA chains.
BARS = {("ae16", "small"): (6.9e-7, 1.7e-6), ("ae16", "large"): (3.2e-7, 5.2e-7),
        ("mfma_tanh", "small"): (7.3e-7, 1.7e-6), ("mfma_tanh", "large"): (4.3e-8, 4.3e-7),
        ("mfma_any", "small"): (4.6e-7, 1.1e-6), ("mfma_any", "large"): (1.7e-7, 6.8e-7)}


# ---------------------------------------------------------------------------------------------------- RegAutoEncoderTask
# The launch modes of ae_mfma_kernel that only RegAutoEncoderTask reaches (K regulariser heads, lagged targets and inputs, the
# second pass over the lagged rows: 2 T tiles), first step only.  d: feature width; enc / dec / reg: hidden widths of the encoder,
# the decoder and each of the K regulariser nets (decoder and regularisers of one depth: block-structured layers,
# core.py:_RegFlatParams); k: latent width; lag_ae / lag_reg: target and input lags in rows; layout: the LDS layout the
# gradient pass must take; handoff: forward_keep / backward_reuse are also compared with the plain pair, bit for bit.
RegCase = namedtuple("RegCase", "id d enc k dec reg K B lag_ae lag_reg idx layout dup handoff")
REGAE_BIG_B = 66_001    # T = 1032 tiles: 2 T = 2064 > 2048 blocks, a ragged last tile

REGAE_CASES = [
    RegCase("regae-K1-B5", 6, (8,), 2, (8,), (6,), 1, 5, 1, 2, False, "roomy", False, False),
    RegCase("regae-K4-B5", 6, (8,), 3, (8,), (6,), 4, 5, 2, 1, True, "roomy", False, False),
    RegCase("regae-K4-B63", 9, (12, 7), 3, (7, 12), (5, 4), 4, 63, 2, 3, True, "roomy", False, True),
    RegCase("regae-K8-B65", 6, (8,), 2, (8,), (6,), 8, 65, 1, 1, False, "roomy", False, False),
    RegCase("regae-K1-B63-lag-input-only", 7, (9,), 2, (9,), (3,), 1, 63, 0, 5, False, "roomy", False, False),
    RegCase("regae-K4-B130-lags-cross-tiles", 6, (8,), 2, (8,), (6,), 4, 130, 70, 67, False, "roomy", False, False),
    RegCase("regae-K8-B130-idx", 10, (16, 8), 3, (8, 16), (4, 3), 8, 130, 3, 64, True, "roomy", False, False),
    RegCase("regae-K1-B65-idx", 6, (5,), 1, (5,), (2,), 1, 65, 1, 2, True, "roomy", False, False),
    RegCase("regae-K4-B130-tight", 100, (24, 20), 3, (16, 20), (2, 1), 4, 130, 1, 2, True, "tight", False, True),
    RegCase("regae-K1-B-big", 6, (8,), 2, (8,), (4,), 1, REGAE_BIG_B, 1, 2, False, "roomy", True, False),
]


def regae_dims(c):
    """(e_dims, d_dims, r_dims, the chain's widths: encoder, then decoder and K regulariser nets side by side)."""
    e, d, r = [c.d] + list(c.enc) + [c.k], [c.k] + list(c.dec) + [c.d], [c.k] + list(c.reg) + [1]
    assert len(d) == len(r), c
    return e, d, r, e + [dw + c.K * rw for dw, rw in zip(d[1:], r[1:])]


def regae_grid(c, copies=1):
    """regae_grid over the 2 T tiles of both passes: (blocks, most tiles one block walks)."""
    T2 = 2 * n_tiles(copies * c.B)
    G = min(T2, MAX_BLOCKS)
    return G, (T2 + G - 1) // G


# term -> bar: 8 x the worst distance of the fp32 CPU oracle from the fp64 oracle over REGAE_CASES (ae_inputs.regae_group_e32),
# rounded up to two digits, as BARS above; relative for the loss terms, of the largest entry for the gradient.  That oracle is
# the fp64 one on fp32 tensors with every rounding pinned (ae_inputs.regae_e32: Linear sums in a fixed order, tanh rounded from
# fp64, batch statistics in fp64), so the figures recompute to the digit on another CPU; tests/test_ae_instances.py holds every
# bar, "loss" included, between 4 x and 16 x of them.
# One group for all of RegAE: on randomly initialised heads npl, eig and the gradient amplify the chain's rounding (sums of
# squared lagged differences over variances far smaller than the squared means), most with K = 8 - regae-K8-B65 and
# regae-K8-B130-idx set the worst e32 of loss, npl, eig and grad, five to forty times the other cases'.  So the tight-layout case
# (regae-K4-B130-tight: e32 4.3e-6 on the gradient) is checked at 65 x its own fp32-oracle error, not 8 x.
REGAE_TERMS = ("loss", "ae", "npl", "pen", "eig", "norm", "orth", "grad")
REGAE_BARS = dict(loss=2.0e-5, ae=4.1e-7, npl=1.2e-4, pen=4.5e-8, eig=1.7e-4, norm=1.5e-7, orth=3.8e-6, grad=2.8e-4)
