"""Form C of the CV evaluation kernels - k scalar chains on one trunk (cvf_cv_nets_shared_*, cvf_cv_frame_shared_*,
cvf_cv_frame_large_shared_*, cvf_cv_file_n_shared): the nets, the cases, the Python mirrors of the LDS and
scratch totals, and a reader of the file's n_shared word.  `tests/test_cv_shared_host.py` (CPU) and `tests/test_cv_shared_gpu.py`
(GPU) share it.

The layers, frames, fp64 / fp32 CPU evaluations and the file reader are those of tests/cv_frame_cases.py (wave kernel, cv_nets)
and tests/cv_frame_large_cases.py (workgroup kernel), reused unchanged.  Shapes are the smallest at which form C can go wrong:
B = 6 frames per accuracy case, B = 65 for the independence of frames and the tile tail of cv_nets; trunk widths 63 / 64 / 65 / 256
sit on either side of one lane pass now that the trunk is counted once, head width 9 under k = 8 gives 72 head units (two passes).
"""
import copy
import struct

import torch

from tests import cv_frame_cases as F
from tests import cv_frame_large_cases as G

N_FRAMES = 6
COND_TOL = F.COND_TOL
PAD_FRONT, PAD_BACK = 37, 11

# (net id, trunk dims behind d_r, head dims, k, activation, pad floats in front of the parameters); "reg": a RegModel
NETS = ([("C-k%d" % k, [20, 20], [20, 1], k, "tanh", 0) for k in (1, 3, 6, 8)]
        + [("C-head2", [12], [12, 6, 1], 2, "tanh", 0), ("C-deep", [10, 10, 10], [10, 1], 2, "tanh", 0)]
        + [("C-w%d" % w, [w, w], [w, 1], 3, "tanh", 0) for w in (63, 64, 65, 256)]
        + [("C-head9-k8", [12], [12, 9, 1], 8, "tanh", 0)]
        + [("C-act-%s" % a, [12], [12, 12, 1], 3, a, 0) for a in F.ACTS]
        + [("C-offset", [20, 20], [20, 1], 3, "tanh", PAD_FRONT)]
        + [("C-reg", "reg", [3, 12, 1], 2, "tanh", 0)])
NET = {n[0]: n for n in NETS}
REG_CVEC = {2: [1, 0], 3: [2, 0, 1]}

WAVE_LAYERS = ["mixed10", "weighted12_mixed-angle", "pos22", "dih10", "mixed64", "identity2d"]
ACCURACY = [(lid, "C-k3") for lid in WAVE_LAYERS] + [("mixed10", n[0]) for n in NETS if n[0] not in ("C-k3", "C-k6")]
COEF = [(lid, "C-k%d" % k) for lid in dict.fromkeys(l for l, _ in F.COEF) for k in (3, 8)]   # the layers of F.COEF, once each
LARGE_ACCURACY = [("mixed65", "C-k3"), ("mixed65-angle", "C-k3"), ("mixed300w", "C-k3"), ("mixed1000", "C-k3"), ("dih300", "C-k3"),
                  ("dih300-rows", "C-k8"), ("c5", "C-k6"), ("mixed65", "C-head2"), ("mixed65", "C-reg"), ("mixed65", "C-w256")]
LARGE_COEF = [("mixed65", "C-k3"), ("mixed65", "C-k8"), ("mixed300w", "C-k3"), ("dih300-rows", "C-k8")]

# seeds of the nets, for cases that seed 0 leaves past COND_TOL on the CPU: none so far (tests/test_cv_shared_host.py prints the
# figures; the closest are mixed64 C-k3 at 1.9e-6 and c5 C-k6 at 1.7e-6)
NET_SEED = {}


def is_large(lid):
    return lid in G.LAYERS


def d_r_of(lid):
    return G.d_r_of(lid) if is_large(lid) else F.d_r_of(lid)


def frames(lid, B=N_FRAMES):
    """traj [B, ...] fp32 of a layer id of either case file."""
    return G.frames(lid, B)[0] if is_large(lid) else F.hip_layer(lid, B=B)[1]


def hip_layer(lid, dev=None):
    return G.hip_layer(lid, dev) if is_large(lid) else F.hip_layer(lid, dev, B=1)[0]


def cpu_eval(lid, nets, traj, dtype):
    return (G if is_large(lid) else F).cpu_eval(lid, nets, traj, dtype)


def build_nets(nid, d_r, seed=0):
    """The torch module of a net id for d_r features (CPU, fp32), seeded: a SharedEigenFunctions, or a RegModel ("reg")."""
    from colvarsfinder import nn
    _, trunk, head, k, act, _ = NET[nid]
    torch.manual_seed(2000 + seed + sum(map(ord, nid)))
    if trunk == "reg":
        return nn.RegModel(nn.RegAutoEncoder([d_r, 16, 3], [3, 16, d_r], head, k), REG_CVEC[k])
    A = F.ACTS[act]
    if A is not None:
        return nn.SharedEigenFunctions([d_r] + trunk, head, k, activation=A())
    m = nn.SharedEigenFunctions([d_r] + trunk, head, k)   # Linear layers only: the chains keep sharing the trunk's modules
    m.eigen_funcs = torch.nn.ModuleList([torch.nn.Sequential(*[c for c in net._modules.values() if isinstance(c, torch.nn.Linear)])
                                         for net in m.eigen_funcs])
    return m


def nets_for(lid, nid):
    return build_nets(nid, d_r_of(lid), NET_SEED.get((lid, nid), 0))


def plan_of(nets, pad=0):
    """(MLPDesc, n_layers, k, theta fp32 CPU, n_shared) of core._CVModel._nets_plan_shared - every tensor once - the parameters
    `pad` NaN floats into a larger theta with 11 NaN floats behind them (tests/cv_frame_cases.plan_of)."""
    from colvarsfinder import core
    d, L, k, params, ns = core._CVModel._nets_plan_shared(nets)
    theta = torch.cat([p.detach().reshape(-1).float() for p in params])
    if pad:
        d = copy.deepcopy(d)
        for i in range(d.n_nets):
            for l in range(d.n_layers):
                d.w_off[i][l] += pad
                d.b_off[i][l] += pad
        theta = torch.cat([torch.full((pad,), float("nan")), theta, torch.full((PAD_BACK,), float("nan"))])
        d.n_params = theta.numel()
    return d, L, k, theta, ns


# ------------------------------------------------------------------------------------------------ descriptions by hand
def shared_mlp(trunk, head, k, act=1):
    """A form-C MLPDesc over dims = trunk + head[1:] (trunk[-1] == head[0]): the trunk once, then head 0, head 1, .."""
    from colvarsfinder import _hip
    dims, ns = list(trunk) + list(head[1:]), len(trunk) - 1
    m, pos = _hip.MLPDesc(), 0
    m.n_nets, m.n_layers = k, len(dims) - 1
    for l, d in enumerate(dims):
        m.dims[l] = d
    for l in range(len(dims) - 1):
        m.act[l] = act if l + 1 < len(dims) - 1 else 0
    for l in range(ns):
        for i in range(k):
            m.w_off[i][l], m.b_off[i][l] = pos, pos + dims[l] * dims[l + 1]
        pos += (dims[l] + 1) * dims[l + 1]
    for i in range(k):
        for l in range(ns, len(dims) - 1):
            m.w_off[i][l], m.b_off[i][l] = pos, pos + dims[l] * dims[l + 1]
            pos += (dims[l] + 1) * dims[l + 1]
    m.n_params = pos
    return m, ns


# ------------------------------------------------------------------------------------------------ mirrors of the C totals
def lds_floats(m, ns, pp):
    """Python mirror of the wave kernel's LDS total for form C (csrc/cv_frame.hip: cvfr_why with ns > 0), in floats."""
    from colvarsfinder import _hip as H
    k = m.n_nets
    identity = pp.mode == H.PP_IDENTITY
    tot = pp.n_coord + (0 if identity else m.dims[0])
    tot += nets_lds_floats(m, ns)
    if not identity:
        tot += k * pp.n_rec * 12 + k * pp.n_coord + k * 12
    return tot


def nets_lds_floats(m, ns):
    """The nets' share of both kernels' LDS: the trunk's activations once, the heads' k times, two sweep vectors of a head, two
    images [k][widest trunk layer] of the trunk's sweep, k rows of d xi / d r."""
    L, k = m.n_layers, m.n_nets
    trunk, heads = [m.dims[l] for l in range(1, ns + 1)], [m.dims[l] for l in range(ns + 1, L + 1)]
    return sum(trunk) + k * sum(heads) + 2 * max([1] + heads) + 2 * k * max(trunk) + k * m.dims[0]


def large_lds_layout(m, ns, pp):
    """Mirror of the workgroup kernel's layout for form C (csrc/cv_frame_large.hip: cvfl_why with ns > 0):
    (bytes of LDS or None, rows_per_pass)."""
    k = m.n_nets
    pos = m.dims[0] + nets_lds_floats(m, ns)
    pos = (pos + 1) // 2 * 2 + G.RED_FLOATS
    pos = (pos + 3) // 4 * 4
    row = 3 * pp.n_ref
    rpp = min(k, (G.LDS_LIMIT // 4 - pos) // row) if G.LDS_LIMIT // 4 - pos >= row else 0
    return (4 * (pos + rpp * row) if rpp >= 1 else None), rpp


def scratch_floats(m, ns, B, want_g=True):
    """Mirror of cvf_cv_nets_shared_scratch_floats (csrc/cv_nets.hip: cvn_layout): the trunk's images once."""
    L, k, per = m.n_layers, m.n_nets, (B + 63) // 64 * 64
    tot = m.dims[0] + sum(m.dims[l] for l in range(1, ns + 1)) + k * sum(m.dims[l] for l in range(ns + 1, L + 1))
    if want_g:
        tot += 2 * k * max([0] + [m.dims[l] for l in range(1, L - 1)])
    return per * tot


# ------------------------------------------------------------------------------------------------ the file
def file_n_shared(blob):
    """The word at byte 956 (tests/cv_frame_cases.read_cv_file asserts 0 there: it reads files of forms A and B)."""
    return struct.unpack_from("<i", blob, F.TAIL_OFFSET + 12)[0]


def read_cv_file(blob):
    """tests/cv_frame_cases.read_cv_file of a file of any form, plus "n_shared"."""
    got = F.read_cv_file(F.patched(blob, F.TAIL_OFFSET + 12, "<i", 0))
    got["n_shared"] = file_n_shared(blob)
    return got
