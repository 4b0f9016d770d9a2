"""One-launch CV evaluation (csrc/cv_frame.hip, cvf_cv_frame_*) and the CV model file (csrc/cv_file.hip, cvf_cv_file_*): the
cases, the descriptors of the predicate table, a pure-Python reader of the file, and the CPU evaluations (fp64 / fp32) that the
conditioning test ties the accuracy cases to.

`tests/test_cv_frame_host.py` and `tests/test_cv_file_host.py` (CPU) and `tests/test_cv_frame_gpu.py` (GPU) share it.

Shapes are the smallest at which the kernel can still go wrong: a wave owns one frame; units, records and atoms are strided over
its 64 lanes (widths 63 / 64 / 65 sit on either side of one pass, 256 is four passes, mixed64 has more than 64 records and
exactly 64 atoms); B = 6 frames per accuracy case, B = 65 for the independence of frames.
"""
import copy
import struct

import numpy as np
import torch

from tests.synth import make_2d_traj, make_molecule_traj

DIR_OFFSET, ENTRY_BYTES, MLP_OFFSET, PP_OFFSET, TAIL_OFFSET = 960, 24, 16, 896, 944
MAX_NETS, MAX_LAYERS = 8, 12
TABLE_IDS = {"align_idx": 1, "ref_c": 2, "rec": 3, "align_w": 4, "atom_align": 5, "atom_slot": 6, "rec_slot": 7, "slot_atom": 8,
             "mrec": 9, "slot_row": 10, "theta": 11}
FLOAT_TABLES = ("ref_c", "align_w", "theta")
PP_SCALARS = ("mode", "n_coord", "n_align", "n_rec", "d_r", "use_angle_value", "has_position", "flags", "n_slot", "n_rec_slot",
              "n_mrec", "n_ref")
N_FRAMES = 6
COND_TOL = 2e-6     # fp32 CPU evaluation against fp64, the condition every accuracy case has to meet (issue: not loosened)

DIH10 = [("dihedral", (0, 1, 2, 3)), ("dihedral", (1, 2, 3, 4)), ("dihedral", (2, 4, 5, 6)), ("dihedral", (3, 5, 7, 8)),
         ("dihedral", (4, 6, 8, 9)), ("dihedral", (0, 3, 6, 9))]

# (layer id, case name of tests/test_align_vjp_gpu.case or None, use_angle_value)
LAYERS = [("mixed10", "mixed10", False), ("mixed10-angle", "mixed10", True), ("weighted12_mixed-angle", "weighted12_mixed", True),
          ("pos22", "pos22", False), ("mixed64", "mixed64", False), ("mixed64-angle", "mixed64", True), ("dih10", None, False),
          ("identity2d", None, False)]


# ------------------------------------------------------------------------------------------------ the file, read in Python
def read_cv_file(blob):
    """{"mlp": {...}, "pp": {...}, "upto_layer", "k", "tables": {name: array}, "offsets": {name: (offset, count)}} of a CV file."""
    assert blob[:4] == b"CVF1"
    version, max_nets, max_layers = struct.unpack_from("<3i", blob, 4)
    assert (version, max_nets, max_layers) == (1, MAX_NETS, MAX_LAYERS)
    ints = np.frombuffer(blob, dtype="<i4", count=(PP_OFFSET - MLP_OFFSET) // 4, offset=MLP_OFFSET)
    L1 = MAX_LAYERS + 1
    mlp = {"n_nets": int(ints[0]), "n_layers": int(ints[1]), "dims": ints[2:2 + L1].tolist(),
           "act": ints[2 + L1:2 + L1 + MAX_LAYERS].tolist(),
           "w_off": ints[2 + L1 + MAX_LAYERS:2 + L1 + MAX_LAYERS + MAX_NETS * MAX_LAYERS].reshape(MAX_NETS, MAX_LAYERS).tolist(),
           "b_off": ints[2 + L1 + MAX_LAYERS + MAX_NETS * MAX_LAYERS:-1].reshape(MAX_NETS, MAX_LAYERS).tolist(), "n_params": int(ints[-1])}
    pp = dict(zip(PP_SCALARS, struct.unpack_from("<12i", blob, PP_OFFSET)))
    upto, k, n_entries, zero = struct.unpack_from("<4i", blob, TAIL_OFFSET)
    assert zero == 0 and n_entries == len(TABLE_IDS)
    names = {v: n for n, v in TABLE_IDS.items()}
    tables, offsets = {}, {}
    for e in range(n_entries):
        tid, ty, count, off = struct.unpack_from("<2i2q", blob, DIR_OFFSET + ENTRY_BYTES * e)
        name = names[tid]
        assert ty == (1 if name in FLOAT_TABLES else 0)
        assert count == 0 or (off % 16 == 0 and off + 4 * count <= len(blob))
        tables[name] = np.frombuffer(blob, dtype="<f4" if ty else "<i4", count=count, offset=off if count else 0).copy()
        offsets[name] = (off, count)
    return {"mlp": mlp, "pp": pp, "upto_layer": upto, "k": k, "tables": tables, "offsets": offsets}


def patched(blob, offset, fmt, *values):
    b = bytearray(blob)
    struct.pack_into(fmt, b, offset, *values)
    return bytes(b)


def dir_entry_offset(name):
    return DIR_OFFSET + ENTRY_BYTES * (TABLE_IDS[name] - 1)   # save_cv_file lists the tables in id order


# ------------------------------------------------------------------------------------------------ layers and nets
def layer_parts(lid, B=N_FRAMES, seed=0):
    """(n_atoms or None, align, features, weights, traj [B, ...] fp32, ref) of a layer id of LAYERS."""
    from tests.test_align_vjp_gpu import case
    _, name, _ = next(l for l in LAYERS if l[0] == lid)
    if lid == "identity2d":
        return None, None, None, None, make_2d_traj(B, seed=4 + seed)[0].astype(np.float32), None
    if lid == "dih10":
        traj, _, ref = make_molecule_traj(10, B, seed=310 + seed)
        return 10, None, DIH10, None, traj, ref
    n, align, feats, w = case(name)
    traj, _, ref = make_molecule_traj(n, B, seed=300 + n + seed)
    return n, align, feats, w, traj, ref


def hip_layer(lid, dev=None, B=N_FRAMES, seed=0):
    """(AlignFeatureLayer or Identity, traj, ref)."""
    from colvarsfinder import pp
    n, align, feats, w, traj, ref = layer_parts(lid, B, seed)
    angle = next(l for l in LAYERS if l[0] == lid)[2]
    if n is None:
        return torch.nn.Identity(), traj, ref
    layer = pp.AlignFeatureLayer(n, align, None if align is None else ref[align], feats, angle, align_weights=w)
    return (layer if dev is None else layer.to(dev)), traj, ref


def d_r_of(lid):
    layer, traj, _ = hip_layer(lid, B=1)
    return 2 if isinstance(layer, torch.nn.Identity) else layer.d_r


class RawFeatures(torch.nn.Module):
    """oracle.pp.features_of on the raw coordinates: the fp64 / fp32 twin of a layer without alignment."""

    def __init__(self, feats, angle):
        super().__init__()
        self.feats, self.angle = feats, angle

    def forward(self, x):
        from oracle.pp import features_of
        return features_of(x, self.feats, self.angle)


def torch_layer(lid, dtype):
    """The layer in plain torch at `dtype` on the CPU (oracle.pp.AlignFeature, the raw features, or Identity)."""
    from oracle.pp import AlignFeature
    n, align, feats, w, _, ref = layer_parts(lid, 1)
    angle = next(l for l in LAYERS if l[0] == lid)[2]
    if n is None:
        return torch.nn.Identity()
    if align is None:
        return RawFeatures(feats, angle)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return AlignFeature(align, ref[align], feats, angle, align_weights=w)
    finally:
        torch.set_default_dtype(old)


ACTS = {"none": None, "tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid, "relu": torch.nn.ReLU, "elu": torch.nn.ELU,
        "leaky_relu": torch.nn.LeakyReLU, "softplus": torch.nn.Softplus}

# (net id, form, dims behind d_r, k, activation, activation after the last layer, pad floats in front of the parameters)
NETS = ([("A-k%d" % k, "A", [20, 20, 1], k, "tanh", False, 0) for k in (1, 3, 8)]
        + [("B-encoder-offset", "B", [20, 2], 2, "tanh", False, 37), ("B-one-layer", "B", [3], 3, "tanh", False, 0),
           ("B-act-after-last", "B", [20, 2], 2, "tanh", True, 0)]
        + [("A-w%d" % w, "A", [w, w, 1], 3, "tanh", False, 0) for w in (63, 64, 65, 256)]
        + [("A-act-%s" % a, "A", [12, 12, 1], 3, a, False, 0) for a in ACTS]
        # eight chains of six 256-wide layers on mixed10: about 56 KiB of LDS per frame, past the 48 KiB a launch gets by default
        + [("A-lds-over-48k", "A", [256] * 6 + [1], 8, "tanh", False, 0)])
NET = {n[0]: n for n in NETS}

# every layer under the k = 3 nets of the conditioning figures; every net shape on mixed10
ACCURACY = [(lid, "A-k3") for lid, _, _ in LAYERS] + [("mixed10", n[0]) for n in NETS if n[0] != "A-k3"]
COEF = [("mixed10", "A-k3"), ("mixed10", "A-k8"), ("pos22", "A-k3"), ("identity2d", "A-k3"), ("mixed10", "B-encoder-offset")]


# seeds of the nets, chosen on the CPU where seed 0 leaves a case past COND_TOL (mixed64: the fp32 evaluation itself is at
# 1.2e-6 .. 2.3e-6 of fp64 over seeds 0..5; the frames are those of make_molecule_traj(n, B, seed=300 + n) throughout)
NET_SEED = {"mixed64": 2, "mixed64-angle": 5}


def nets_for(lid, nid):
    return build_nets(nid, d_r_of(lid), NET_SEED.get(lid, 0))


def build_nets(nid, d_r, seed=0):
    """The torch module of a net id for d_r features (CPU, fp32), seeded."""
    from colvarsfinder import nn
    _, form, dims, k, act, act_last, _ = NET[nid]
    torch.manual_seed(1000 + seed + sum(map(ord, nid)))
    A = ACTS[act]
    if form == "A":
        if A is None:   # k chains of Linear layers without activations
            m = nn.EigenFunctions([d_r] + dims, k)
            m.eigen_funcs = torch.nn.ModuleList([torch.nn.Sequential(*[c for c in net._modules.values() if isinstance(c, torch.nn.Linear)])
                                                 for net in m.eigen_funcs])
            return m
        return nn.EigenFunctions([d_r] + dims, k, activation=A())
    widths = [d_r] + dims
    mods = []
    for l, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        mods.append(torch.nn.Linear(a, b))
        if l + 1 < len(widths) - 1 or act_last:
            mods.append(A())
    return torch.nn.Sequential(*mods)


def plan_of(nets, pad=0):
    """(MLPDesc, upto_layer, k, theta fp32 CPU) of core._CVModel._nets_plan, the parameters `pad` floats into a larger theta."""
    from colvarsfinder import core
    d, upto, k, params = core._CVModel._nets_plan(nets)
    theta = torch.cat([p.detach().reshape(-1).float() for p in params])
    if pad:
        d = copy.deepcopy(d)
        for i in range(d.n_nets):
            for l in range(d.n_layers):
                d.w_off[i][l] += pad
                d.b_off[i][l] += pad
        theta = torch.cat([torch.full((pad,), float("nan")), theta, torch.full((11,), float("nan"))])
        d.n_params = theta.numel()
    return d, upto, k, theta


def cpu_eval(lid, nets, traj, dtype):
    """(xi [B, k], J [B, k, *frame]) by torch.func.jacrev through the torch layer and a copy of the nets at `dtype`, on the CPU."""
    pp = torch_layer(lid, dtype)
    net = copy.deepcopy(nets).to(device="cpu", dtype=dtype)
    X = torch.tensor(np.asarray(traj), dtype=dtype)

    def f(x):
        y = net(pp(x.unsqueeze(0))).reshape(-1)
        return y, y

    J, xi = torch.func.vmap(torch.func.jacrev(f, has_aux=True))(X)
    return xi.detach().numpy(), J.detach().numpy()


# ------------------------------------------------------------------------------------------------ the predicate table
def mlp(dims, nets=1, act=1):
    from colvarsfinder import _hip
    m, pos = _hip.MLPDesc(), 0
    m.n_nets, m.n_layers = nets, len(dims) - 1
    for l, d in enumerate(dims[:MAX_LAYERS + 1]):
        m.dims[l] = d
    for i in range(min(nets, MAX_NETS)):
        for l in range(min(len(dims) - 1, MAX_LAYERS)):
            m.act[l] = act if l + 1 < len(dims) - 1 else 0
            m.w_off[i][l], m.b_off[i][l] = pos, pos + dims[l] * dims[l + 1]
            pos += (dims[l] + 1) * dims[l + 1]
    m.n_params = pos
    return m


def pp_desc(mode, n_coord, d_r, n_rec=4, n_align=3, fake_tables=True):
    """A descriptor for the predicate (host arithmetic: the table pointers are only compared with NULL)."""
    from colvarsfinder import _hip
    d = _hip.PPDesc()
    d.mode, d.n_coord, d.d_r = mode, n_coord, d_r
    if mode in (_hip.PP_ALIGN, _hip.PP_FEATURES):
        d.n_rec, d.rec = n_rec, 16 if fake_tables else None
        if mode == _hip.PP_ALIGN:
            d.n_align, d.align_idx, d.ref_c = n_align, 16, 16
    return d


def predicate_table():
    """[(id, MLPDesc, upto_layer, PPDesc, expected answer, words the reason must contain)]"""
    from colvarsfinder import _hip as H
    A, F, I, X = H.PP_ALIGN, H.PP_FEATURES, H.PP_IDENTITY, H.PP_FACTORED
    chain = lambda d_r, k=3: mlp([d_r, 20, 20, 1], k)
    deep = lambda n: [6] + [4] * (n - 1) + [1]
    return [
        ("align-192", chain(66), 3, pp_desc(A, 192, 66), 1, ""),
        ("align-195", chain(66), 3, pp_desc(A, 195, 66), 0, "n_coord = 195"),
        ("features-192", chain(8), 3, pp_desc(F, 192, 8), 1, ""),
        ("features-195", chain(8), 3, pp_desc(F, 195, 8), 0, "n_coord = 195"),
        ("identity-512", chain(512), 3, pp_desc(I, 512, 512), 1, ""),
        ("identity-513", chain(513), 3, pp_desc(I, 513, 513), 0, "dims[0] = 513"),
        ("identity-513-coord", mlp([512, 20, 1], 3), 2, pp_desc(I, 513, 512), 0, "n_coord = 513"),
        ("inner-256", mlp([30, 256, 256, 1], 3), 3, pp_desc(A, 30, 30), 1, ""),
        ("inner-257", mlp([30, 256, 257, 1], 3), 3, pp_desc(A, 30, 30), 0, "257 wide"),
        ("k-8", chain(30, 8), 3, pp_desc(A, 30, 30), 1, ""),
        ("k-9-nets", chain(30, 9), 3, pp_desc(A, 30, 30), 0, "9 nets"),
        ("k-8-encoder", mlp([30, 20, 8]), 2, pp_desc(A, 30, 30), 1, ""),
        ("k-9-encoder", mlp([30, 20, 9]), 2, pp_desc(A, 30, 30), 0, "k = 9"),
        ("layers-12", mlp(deep(12), 3), 12, pp_desc(I, 6, 6), 1, ""),
        ("layers-13", mlp(deep(13), 3), 13, pp_desc(I, 6, 6), 0, "13 layers"),
        ("factored", chain(4), 3, pp_desc(X, 12, 4), 0, "CVF_PP_FACTORED"),
        # 8 chains x 11 layers x 256 units of activations alone are 88 KiB
        ("lds-over", mlp([30] + [256] * 11 + [1], 8), 12, pp_desc(A, 30, 30), 0, "bytes of LDS"),
        ("d_r-mismatch", chain(30), 3, pp_desc(A, 30, 29), 0, "features"),
    ]


def lds_floats(m, upto, pp):
    """Python mirror of the predicate's LDS total (csrc/cv_frame.hip: cvfr_why), in floats."""
    from colvarsfinder import _hip as H
    form_a = m.n_nets > 1
    k, nn = (m.n_nets, m.n_nets) if form_a else (m.dims[upto], 1)
    identity = pp.mode == H.PP_IDENTITY
    tot = pp.n_coord + (0 if identity else m.dims[0])
    tot += nn * sum(m.dims[l] for l in range(1, upto + 1)) + 2 * max([1] + [m.dims[l] for l in range(1, upto + 1)]) + k * m.dims[0]
    if not identity:
        tot += k * pp.n_rec * 12 + k * pp.n_coord + k * 12
    return tot
