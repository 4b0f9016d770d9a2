"""One-launch CV evaluation for frames of any size (csrc/cv_frame_large.hip, cvf_cv_frame_large_*): the cases, the descriptors of
the predicate table, the Python mirror of the LDS layout and the CPU evaluations (fp64 / fp32) that the conditioning test ties
the accuracy cases to.  `tests/test_cv_frame_large_host.py` (CPU) and `tests/test_cv_frame_large_gpu.py` (GPU) share it.

A workgroup of 256 threads owns one frame; align atoms, records, slots, units and coordinates are strided over its threads.
Shapes are the smallest at which that can go wrong (B = 3 frames per accuracy case, 2 for c5):

  mixed65       one atom past the wave kernel; 32 align atoms (one partial wave), both angle modes
  mixed300w     300 atoms, per-atom weights on 257 align atoms (one past one sweep of the threads), more than 256 records and more
                than 256 slots (both stride twice, ragged)
  mixed1000     600 align atoms (three sweeps, ragged), 400 atoms not aligned, most of them never read
  dih300        CVF_PP_FEATURES: bonds and dihedrals of the raw coordinates, no alignment
  dih300-rows   the same with 80 bonds and 420 dihedrals in angle-value mode under eight chains: 1840 contribution rows, the row
                table of all eight cotangent rows is past the LDS - rows_per_pass < k
  c5            the config-5 layer (5000 atoms, d_r = 384) under six [384, 20, 20, 1] chains: past 48 KiB of dynamic LDS

The helpers of tests/cv_frame_cases.py that do not look a layer up in its own LAYERS table are reused unchanged (mlp, pp_desc,
plan_of, ACTS, COND_TOL); layers_of / build_nets / cpu_eval here are their twins for this file's layer ids and net shapes.
"""
import copy

import numpy as np
import torch

from tests import cv_frame_cases as F
from tests.synth import make_molecule_traj

COND_TOL = F.COND_TOL
LDS_LIMIT = 160 * 1024
RED_FLOATS = 2 * 4 * 16 + F.MAX_NETS * 4 * 12 + F.MAX_NETS * 12   # the moments' doubles, [row][wave][12], [row][12]

# layer id -> (case name or None, use_angle_value, frames per accuracy case)
LAYERS = {"mixed65": ("mixed65", False, 3), "mixed65-angle": ("mixed65", True, 3), "mixed300w": (None, False, 3),
          "mixed1000": ("mixed1000", False, 3), "dih300": (None, False, 3), "dih300-rows": (None, True, 3), "c5": ("c5", False, 2)}


def parts(lid):
    """(n_atoms, align or None, features, weights or None) of a layer id."""
    from tests.test_align_vjp_gpu import case, random_features
    name = LAYERS[lid][0]
    if name is not None:
        return case(name)
    rs = np.random.RandomState(300)
    if lid == "mixed300w":
        align = sorted(rs.choice(300, 257, replace=False).tolist())
        return 300, align, random_features(300, 301, n_pos=60, n_bond=70, n_angle=70, n_dih=60), rs.uniform(0.2, 3.0, size=257)

    def pick(m):
        return tuple(int(i) for i in rs.choice(300, m, replace=False))

    nb, nd = (80, 420) if lid == "dih300-rows" else (60, 100)
    return 300, None, [("bond", pick(2)) for _ in range(nb)] + [("dihedral", pick(4)) for _ in range(nd)], None


def frames(lid, B=None, seed=0):
    """(traj [B, N, 3] fp32, ref [N, 3])."""
    n = parts(lid)[0]
    traj, _, ref = make_molecule_traj(n, LAYERS[lid][2] if B is None else B, seed=300 + n + seed)
    return traj, ref


def hip_layer(lid, dev=None):
    from colvarsfinder import pp
    n, align, feats, w = parts(lid)
    _, ref = frames(lid, 1)
    layer = pp.AlignFeatureLayer(n, align, None if align is None else ref[align], feats, LAYERS[lid][1], align_weights=w,
                                 weights_any_size=w is not None)
    return layer if dev is None else layer.to(dev)


def torch_layer(lid, dtype):
    """The layer in plain torch at `dtype` on the CPU (oracle.pp.AlignFeature or the raw features)."""
    from oracle.pp import AlignFeature
    n, align, feats, w = parts(lid)
    if align is None:
        return F.RawFeatures(feats, LAYERS[lid][1])
    _, ref = frames(lid, 1)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return AlignFeature(align, ref[align], feats, LAYERS[lid][1], align_weights=w)
    finally:
        torch.set_default_dtype(old)


# (net id, form, dims behind d_r, k, activation, activation after the last layer, pad floats in front of the parameters)
NETS = [("A-k1", "A", [20, 20, 1], 1, "tanh", False, 0), ("A-k3", "A", [20, 20, 1], 3, "tanh", False, 0),
        ("A-k6", "A", [20, 20, 1], 6, "tanh", False, 0), ("A-k8", "A", [20, 20, 1], 8, "tanh", False, 0),
        ("B-encoder-offset", "B", [20, 2], 2, "tanh", False, 37), ("B-one-layer", "B", [3], 3, "tanh", False, 0),
        ("B-act-after-last", "B", [20, 2], 2, "tanh", True, 0), ("A-w255", "A", [255, 255, 1], 3, "tanh", False, 0),
        ("A-w256", "A", [256, 256, 1], 3, "tanh", False, 0), ("A-act-softplus", "A", [12, 12, 1], 3, "softplus", False, 0)]
NET = {n[0]: n for n in NETS}

LAYER_CASES = [("mixed65", "A-k3"), ("mixed65-angle", "A-k3"), ("mixed300w", "A-k3"), ("mixed1000", "A-k3"), ("dih300", "A-k3"),
               ("dih300-rows", "A-k8"), ("c5", "A-k6")]
ACCURACY = LAYER_CASES + [("mixed65", n[0]) for n in NETS if n[0] not in ("A-k3", "A-k6")]
COEF = [("mixed65", "A-k3"), ("mixed65", "A-k8"), ("mixed65", "B-encoder-offset"), ("mixed300w", "A-k3"), ("dih300-rows", "A-k8"),
        ("c5", "A-k6")]

# seeds of the nets, chosen on the CPU where seed 0 leaves a case past COND_TOL (c5: the fp32 evaluation itself is at 1.4e-6 ..
# 3.3e-6 of fp64 over seeds 0..7, only seed 2 below the bar; tests/test_cv_frame_large_host.py prints the figures)
NET_SEED = {("c5", "A-k6"): 2}


def d_r_of(lid):
    return hip_layer(lid).d_r


def build_nets(nid, d_r, seed=0):
    """The torch module of a net id for d_r features (CPU, fp32), seeded (tests/cv_frame_cases.build_nets for this file's NETS)."""
    from colvarsfinder import nn
    _, form, dims, k, act, act_last, _ = NET[nid]
    torch.manual_seed(1000 + seed + sum(map(ord, nid)))
    A = F.ACTS[act]
    if form == "A":
        return nn.EigenFunctions([d_r] + dims, k, activation=A())
    widths = [d_r] + dims
    mods = []
    for l, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        mods.append(torch.nn.Linear(a, b))
        if l + 1 < len(widths) - 1 or act_last:
            mods.append(A())
    return torch.nn.Sequential(*mods)


def nets_for(lid, nid):
    return build_nets(nid, d_r_of(lid), NET_SEED.get((lid, nid), 0))


def cpu_eval(lid, nets, traj, dtype):
    """(xi [B, k], J [B, k, N, 3]) by torch.func.jacrev through the torch layer and a copy of the nets at `dtype`, on the CPU."""
    pp = torch_layer(lid, dtype)
    net = copy.deepcopy(nets).to(device="cpu", dtype=dtype)
    X = torch.tensor(np.asarray(traj), dtype=dtype)

    def f(x):
        y = net(pp(x.unsqueeze(0))).reshape(-1)
        return y, y

    J, xi = torch.func.vmap(torch.func.jacrev(f, has_aux=True))(X)
    return xi.detach().numpy(), J.detach().numpy()


# ------------------------------------------------------------------------------------------------ the predicate table
def pp_large(mode, n_coord, d_r, n_align=3, n_slot=8, n_ref=16, n_mrec=4, **missing):
    """tests/cv_frame_cases.pp_desc plus the large-frame tables (host arithmetic: the pointers are only compared with NULL);
    `name=None` leaves a table out."""
    from colvarsfinder import _hip
    d = F.pp_desc(mode, n_coord, d_r, n_rec=n_mrec, n_align=n_align)
    if mode in (_hip.PP_ALIGN, _hip.PP_FEATURES):
        d.n_slot, d.n_ref, d.n_mrec, d.n_rec_slot = n_slot, n_ref, n_mrec, n_mrec
        d.mrec = d.slot_row = d.slot_atom = d.atom_slot = d.rec_slot = 16
        if mode == _hip.PP_ALIGN:
            d.atom_align = 16
        for name, v in missing.items():
            assert v is None
            setattr(d, name, None)
            if name == "mrec":
                d.n_mrec = 0
    return d


def predicate_table():
    """[(id, MLPDesc, upto_layer, PPDesc, expected answer, words the reason must contain)]"""
    from colvarsfinder import _hip as H
    A, Fm, I, X = H.PP_ALIGN, H.PP_FEATURES, H.PP_IDENTITY, H.PP_FACTORED
    chain = lambda d_r, k=3: F.mlp([d_r, 20, 20, 1], k)
    deep = lambda n: [6] + [4] * (n - 1) + [1]
    return [
        ("align-195", chain(66), 3, pp_large(A, 195, 66), 1, ""),
        ("align-192", chain(66), 3, pp_large(A, 192, 66), 1, ""),
        ("align-15000", chain(384, 6), 3, pp_large(A, 15000, 384, n_align=5000, n_slot=600, n_ref=608, n_mrec=224), 1, ""),
        ("align-194", chain(66), 3, pp_large(A, 194, 66), 0, "n_coord = 194"),
        ("features-3", chain(8), 3, pp_large(Fm, 3, 8), 1, ""),
        ("features-0", chain(8), 3, pp_large(Fm, 0, 8), 0, "n_coord = 0"),
        ("features-195", chain(8), 3, pp_large(Fm, 195, 8), 1, ""),
        ("features-no-atom_align", chain(8), 3, pp_large(Fm, 195, 8, atom_align=None), 1, ""),
        ("identity", chain(30), 3, F.pp_desc(I, 30, 30), 0, "CVF_PP_IDENTITY"),
        ("factored", chain(4), 3, F.pp_desc(X, 12, 4), 0, "CVF_PP_FACTORED"),
        ("no-mrec", chain(66), 3, pp_large(A, 195, 66, mrec=None), 0, "no mrec table"),
        ("no-atom_align", chain(66), 3, pp_large(A, 195, 66, atom_align=None), 0, "no atom_align table"),
        ("no-slot_row", chain(66), 3, pp_large(A, 195, 66, slot_row=None), 0, "no slot_row table"),
        ("no-slot_atom", chain(66), 3, pp_large(A, 195, 66, slot_atom=None), 0, "no slot_atom table"),
        ("no-atom_slot", chain(66), 3, pp_large(A, 195, 66, atom_slot=None), 0, "no atom_slot table"),
        ("n_align-2", chain(66), 3, pp_large(A, 195, 66, n_align=2), 0, "n_align=2"),
        ("n_slot-4096", chain(66), 3, pp_large(A, 15000, 66, n_slot=4096), 1, ""),
        ("n_slot-4097", chain(66), 3, pp_large(A, 15000, 66, n_slot=4097), 0, "n_slot = 4097"),
        ("n_ref-6144", chain(66), 3, pp_large(A, 15000, 66, n_ref=6144), 1, ""),
        ("n_ref-6145", chain(66), 3, pp_large(A, 15000, 66, n_ref=6145), 0, "n_ref = 6145"),
        ("in-512", chain(512), 3, pp_large(A, 195, 512), 1, ""),
        ("in-513", chain(513), 3, pp_large(A, 195, 513), 0, "dims[0] = 513"),
        ("inner-256", F.mlp([30, 256, 256, 1], 3), 3, pp_large(A, 195, 30), 1, ""),
        ("inner-257", F.mlp([30, 256, 257, 1], 3), 3, pp_large(A, 195, 30), 0, "257 wide"),
        ("k-8", chain(30, 8), 3, pp_large(A, 195, 30), 1, ""),
        ("k-9-nets", chain(30, 9), 3, pp_large(A, 195, 30), 0, "9 nets"),
        ("k-8-encoder", F.mlp([30, 20, 8]), 2, pp_large(A, 195, 30), 1, ""),
        ("k-9-encoder", F.mlp([30, 20, 9]), 2, pp_large(A, 195, 30), 0, "k = 9"),
        ("layers-1", F.mlp([6, 2]), 1, pp_large(Fm, 195, 6), 1, ""),
        ("layers-12", F.mlp(deep(12), 3), 12, pp_large(Fm, 195, 6), 1, ""),
        ("layers-13", F.mlp(deep(13), 3), 13, pp_large(Fm, 195, 6), 0, "13 layers"),
        # 8 chains x 12 layers x 256 units of activations (96 KiB) and 8 x 512 of d xi / d r leave no room for one 72 KiB row
        ("lds-over", F.mlp([512] + [256] * 11 + [1], 8), 12, pp_large(A, 195, 512, n_ref=6144), 0, "bytes of LDS"),
        ("d_r-mismatch", chain(30), 3, pp_large(A, 195, 29), 0, "features"),
    ]


def lds_layout(m, upto, pp):
    """Python mirror of the predicate's layout (csrc/cv_frame_large.hip: cvfl_why): (bytes of LDS or None, rows_per_pass)."""
    form_a = m.n_nets > 1
    k, nn = (m.n_nets, m.n_nets) if form_a else (m.dims[upto], 1)
    inner = [m.dims[l] for l in range(1, upto + 1)]
    pos = m.dims[0] + nn * sum(inner) + 2 * max([1] + inner) + k * m.dims[0]
    pos = (pos + 1) // 2 * 2 + RED_FLOATS
    pos = (pos + 3) // 4 * 4
    row = 3 * pp.n_ref
    rpp = min(k, (LDS_LIMIT // 4 - pos) // row) if LDS_LIMIT // 4 - pos >= row else 0
    return (4 * (pos + rpp * row) if rpp >= 1 else None), rpp
