"""RegAutoEncoderTask with decoder and regulariser nets of different depths (csrc/regae_general.hip, cvf_regae_ragged_*): its
cases, the Python mirrors of core._RegRaggedFlatParams' chain, of cvf_regae_ragged_supported and of the workspace formula, the
oracle of the cases and the error bars the GPU module holds the route to.

Plain Python at import (no torch, no GPU).  `tests/test_regae_ragged_host.py` (CPU) checks the mirrors against the library and
the layout class and ties the bars to the fp32 CPU oracle; `tests/test_regae_ragged_gpu.py` runs every case through
RegAutoEncoderTask._step against the fp64 oracle.  The cases are ae_cases.RegCase tuples with hidden widths of different counts
in `dec` and `reg`; the hyper-parameters are ae_inputs.REGAE_HYPER.  Every case takes the per-layer route by itself (`layout` is
"ragged"): there is no other one for these models.

The chain (include/cvf.h): behind the encoder, merged layer m holds the rows of the groups alive at depth m, the deeper group's
first; the shallower group's outputs (`fin` rows: K heads, or d reconstruction rows) end image ls = n_enc + min(Ld, Lr), and layer
ls reads the rows before them.
"""
from tests import ae_cases as A
from tests import regae_general_cases as G

RegCase = A.RegCase
TILE = A.TILE
DIP = dict(d=66, enc=(128, 128), k=2, dec=(128, 128), reg=(20,), K=2)       # [66,128,128,2 | 2,128,128,66] + 2 x [2,20,1]


def _case(id, d, enc, k, dec, reg, K, B, lag_ae, lag_reg, idx=False, handoff=True):
    return RegCase(id, d, tuple(enc), k, tuple(dec), tuple(reg), K, B, lag_ae, lag_reg, idx, "ragged", False, handoff)


# The inputs of a case are seeded by its id (ae_inputs.regae_inputs' rule: zlib.crc32).  The trailing "-sN" / "-dN" tags pick, among
# the first forty seeds, one at which the fp32 CPU oracle itself stays within an eighth of BAR_CAP: behind ReLU or Sigmoid layers, and
# with a frozen encoder, a head's variance is at many seeds so much smaller than its squared mean that the fp32 oracle ends 1e-4 to
# 1e-3 from the fp64 one (regae_general_cases.ACT) - no measure of a kernel.  Two sigmoid layers under K = 2 heads of widths (6, 5)
# are like that at every seed tried: that case has one head behind widths (16, 2).
CASES = [
    # ---- the decoder is the deeper group: the heads end early, in the last rows of an inner image
    _case("decoder-one-deeper", 6, (8,), 2, (8, 7), (6,), 2, 70, 1, 2),                                   # two ragged tiles
    _case("decoder-two-deeper-heads-astride-a-block", 6, (8,), 2, (9, 63, 12), (5,), 2, 130, 70, 67, idx=True),   # 63 + 2 rows; lags cross tiles
    _case("regularisers-without-hidden-layer-s1", 5, (7,), 2, (8, 6), (), 1, 65, 1, 2),                   # heads end where the latent vector is read
    # ---- the regulariser nets are the deeper group: the reconstruction ends early, its seed enters at an inner layer
    _case("regularisers-one-deeper", 6, (8,), 2, (8,), (6, 5), 2, 70, 1, 2),
    _case("regularisers-two-deeper-d65", 65, (9,), 2, (12,), (6, 5, 4), 2, 130, 2, 1),                    # finished rows cross a 64-row block
    _case("decoder-without-hidden-layer", 5, (7,), 2, (), (6, 4), 2, 65, 1, 2),
    # ---- the chain the route is for: real widths, the K stage and the row blocks of the product core
    _case("dipeptide-small-regularisers", B=130, lag_ae=1, lag_reg=2, idx=True, **DIP),
    # ---- ReLU and Sigmoid (act(0) != 0: an activation applied to finished or structural rows shows), one per direction each;
    #      frozen encoder; loss only
    _case("decoder-one-deeper-relu-s9", 6, (8,), 2, (8, 7), (6,), 2, 70, 1, 2, handoff=False),
    _case("regularisers-one-deeper-relu-s1", 6, (8,), 2, (8,), (6, 5), 2, 70, 1, 2, handoff=False),
    _case("decoder-one-deeper-sigmoid-s29", 6, (8,), 2, (8, 7), (6,), 2, 70, 1, 2, handoff=False),
    _case("regularisers-one-deeper-sigmoid-d32", 6, (8,), 2, (8,), (16, 2), 1, 70, 1, 2, handoff=False),
    _case("regularisers-one-deeper-frozen-encoder-s2", 6, (8,), 2, (8,), (6, 5), 2, 70, 1, 2, idx=True, handoff=False),
    _case("loss-decoder-one-deeper", 6, (8,), 2, (8, 7), (6,), 2, 70, 1, 2, handoff=False),
]
ACT = {"decoder-one-deeper-relu-s9": "relu", "regularisers-one-deeper-relu-s1": "relu", "decoder-one-deeper-sigmoid-s29": "sigmoid",
       "regularisers-one-deeper-sigmoid-d32": "sigmoid"}
FROZEN = {"regularisers-one-deeper-frozen-encoder-s2"}
LOSS_ONLY = {"loss-decoder-one-deeper"}
# three fused Adam steps against the fp64 oracle's, under the rule of regae_general_cases.ADAM: cases whose fp32 CPU oracle itself
# stays within ADAM_SOURCE_MAX of the fp64 one after those steps (tests/test_regae_ragged_host.py recomputes it), one per direction.
# That table's only case has K = 0; every model here has regulariser nets, and the gradient at a net's last bias is exactly 0 (the
# regulariser does not change when a constant is added to a head), so that Adam turns its rounding noise into steps of +-lr in any
# precision: those K entries are left out of the comparison (adam_compared), as tests/test_gpu_parity.py leaves them out.
ADAM = {"decoder-one-deeper", "regularisers-one-deeper"}
ADAM_SOURCE_MAX = G.ADAM_SOURCE_MAX


def act(c):
    return ACT.get(c.id, "tanh")


def grad(c):
    return c.id not in LOSS_ONLY


def hyper(c):
    from tests import ae_inputs as I
    return dict(I.REGAE_HYPER)


def adam_compared(c, sd0):
    """Boolean mask over the flat parameters (state-dict order): False at the last bias of every regulariser net."""
    import numpy as np
    last = f".{len(c.reg) + 1}.bias"
    return np.concatenate([np.full(p.numel(), not (k.startswith("reg.") and k.endswith(last))) for k, p in sd0.items()])


# ---------------------------------------------------------------------------------------------------- the chain
def model_dims(c):
    """(e_layer_dims, d_layer_dims, reg_layer_dims) of nn.RegAutoEncoder."""
    return [c.d] + list(c.enc) + [c.k], [c.k] + list(c.dec) + [c.d], [c.k] + list(c.reg) + [1]


def depths(c):
    """(n_enc_layers, n_dec_layers, n_reg_layers)."""
    return len(c.enc) + 1, len(c.dec) + 1, len(c.reg) + 1


def shape(c):
    """(image widths dims[0..L], columns of W_0..W_{L-1}, ls, fin, dec_deep)."""
    e, dd, r = model_dims(c)
    ne, Ld, Lr = depths(c)
    dec_deep = Ld > Lr
    dw, rw = dd[1:], [c.K * v for v in r[1:]]
    deep, shallow = (dw, rw) if dec_deep else (rw, dw)
    dims = e + [deep[m] + (shallow[m] if m < len(shallow) else 0) for m in range(len(deep))]
    ls, fin = ne + len(shallow), shallow[-1]
    cols = [dims[l] - (fin if l == ls else 0) for l in range(len(dims) - 1)]
    return dims, cols, ls, fin, dec_deep


def n_params(c):
    dims, cols, *_ = shape(c)
    return sum(dims[l + 1] * (cols[l] + 1) for l in range(len(cols)))


def acts(c):
    """cvf_mlp_desc.act: the activation's code after every layer but the encoder's and the chain's last (the finished rows take
    none, whatever their layer's code)."""
    L, ne, code = len(shape(c)[0]) - 1, depths(c)[0], A.ACTS.index(act(c)) + 1
    return [0 if l in (ne - 1, L - 1) else code for l in range(L)]


def mlp_desc(c):
    """cvf_mlp_desc of the chain as core._RegRaggedFlatParams lays it out (dense layers, W then b, in chain order)."""
    from colvarsfinder import _hip
    m, (dims, cols, *_), ac, pos = _hip.MLPDesc(), shape(c), acts(c), 0
    m.n_nets, m.n_layers = 1, len(cols)
    m.dims[0] = dims[0]
    for l in range(len(cols)):
        m.dims[l + 1], m.act[l] = dims[l + 1], ac[l]
        m.w_off[0][l], pos = pos, pos + cols[l] * dims[l + 1]
        m.b_off[0][l], pos = pos, pos + dims[l + 1]
    m.n_params = pos
    return m


# ---------------------------------------------------------------------------------------------------- the host's rules
def scratch_floats(c, B):
    """regaeg_layout with this chain's parameter count: images for 2 T tiles, two adjoint images, slab rows, the loss pairs."""
    dims, T, n = shape(c)[0], G.n_tiles(B), n_params(c)
    rows = max(1, min(2 * T, G.MAX_ROWS, G.SLAB_BYTES // (4 * n)))
    return ((2 * T * TILE * (sum(dims[:-1]) + 2 * max(dims[1:])) + rows * n + 1) & ~1) + 4 * T


def supported(dims, K, n_enc, n_dec, n_reg, acts_, n_par):
    """rag_why (csrc/regae_general.hip) for one net with valid activation codes and in-range offsets: `dims` the image widths,
    `n_par` the flat buffer's length."""
    L = len(dims) - 1
    blocks = lambda l: ((dims[l + 1] + 63) // 64) * ((dims[l] + 1 + 63) // 64)
    if not (2 <= L <= A.MAX_LAYERS and 1 <= dims[0] <= G.MAX_D0 and all(1 <= h <= G.MAX_WIDTH for h in dims[1:L])
            and all(blocks(l) <= 65535 for l in range(L)) and 1 <= K <= G.MAX_NETS):
        return False
    if n_dec < 1 or n_reg < 1 or n_dec == n_reg or n_enc < 1 or n_enc + max(n_dec, n_reg) != L:
        return False
    if acts_[n_enc - 1] != 0 or dims[n_enc] > G.MAX_NETS:
        return False
    ls, fin, last = n_enc + min(n_dec, n_reg), (K if n_dec > n_reg else dims[0]), (dims[0] if n_dec > n_reg else K)
    if dims[L] != last or dims[ls] <= fin:
        return False
    return n_par == sum(dims[l + 1] * (dims[l] - (fin if l == ls else 0) + 1) for l in range(L))


# ---------------------------------------------------------------------------------------------------- oracles
TERMS = A.REGAE_TERMS
errors = G.errors


def inputs(c):
    """ae_inputs.regae_inputs' rule (seeded by the case's id) for a model of any depths."""
    import zlib
    import numpy as np
    import torch
    from oracle import nnref
    from tests import ae_inputs as I
    seed = zlib.crc32(c.id.encode()) % 100_000
    rs = np.random.RandomState(seed)
    lag = max(c.lag_ae, c.lag_reg)
    n = c.B + lag + (I.EXTRA_ROWS if c.idx else 0)
    traj = rs.normal(size=(n, c.d))
    for t in range(1, n):
        traj[t] = 0.7 * traj[t - 1] + 0.714 * traj[t]
    traj = (traj - traj.mean(0)).astype(np.float32)
    w = rs.uniform(0.5, 1.5, size=n)
    w /= w.mean()
    idx = (np.sort(rs.permutation(n - lag)[:c.B]) if c.idx else np.arange(c.B)).astype(np.int64)
    e, d, r = model_dims(c)
    sd0 = nnref.init_regautoencoder(e, d, r, c.K, torch.Generator().manual_seed(seed), torch.float32)
    return traj, w, idx, [1.0 - 0.1 * i for i in range(c.K)], sd0


def oracle(c, inp, dtype, adam_steps=0, lr=1e-3):
    """regae_general_cases.oracle for these cases (oracle.losses takes nets of any depths): the first step's loss row [loss, ae, npl,
    pen, eig_1..K, 0, norm, orth], the flat gradient (state-dict order) and the ordering, float64; with adam_steps > 0 also the
    flat parameters after that many torch.optim.Adam steps on the batch."""
    import numpy as np
    import torch
    from oracle import losses
    from tests import ae_inputs as I
    traj, w, idx, eig_w, sd0 = inp
    h, K = hyper(c), c.K
    F, W = torch.as_tensor(traj).to(dtype), torch.as_tensor(w.astype(np.float32)).double()
    frozen = c.id in FROZEN
    sd = {k: p.to(dtype).clone().requires_grad_(not (frozen and k.startswith("encoder."))) for k, p in sd0.items()}
    fn = I._rounded_tanh if act(c) == "tanh" else G._rounded(I.ACT_FN[act(c)])

    def terms():
        ae = losses.regae_mse(sd, F[idx], F[idx + c.lag_ae], W[idx], activation=fn)
        eig, npl, pen, cvec = losses.regae_eigen_loss(sd, K, F[idx], W[idx], F[idx + c.lag_reg], W[idx + c.lag_reg], eig_w=eig_w,
                                                      lag_idx=c.lag_reg, dt=h["dt"], activation=fn)
        en, eo = losses.regae_enc_norm(sd, F[idx], W[idx], activation=fn), losses.regae_enc_orth(sd, F[idx], W[idx], activation=fn)
        lo = h["alpha"] * ae + h["gamma"][0] * npl + h["gamma"][1] * pen + h["eta"][1] * en + h["eta"][2] * eo
        return lo, ae, npl, pen, eig, en, eo, cvec

    flat_grad = lambda: torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in sd.values()]).double().numpy()
    lo, ae, npl, pen, eig, en, eo, cvec = terms()
    lo.backward()
    row = np.asarray([float(v.detach()) for v in (lo, ae, npl, pen)] + [float(v) for v in eig] + [0.0, float(en.detach()), float(eo.detach())])
    out = [row, flat_grad(), list(cvec)]
    if adam_steps:
        opt = torch.optim.Adam([p for p in sd.values() if p.requires_grad], lr=lr)
        for step in range(adam_steps):
            if step:
                opt.zero_grad()
                terms()[0].backward()
            opt.step()
        out.append(torch.cat([p.detach().reshape(-1) for p in sd.values()]).double().numpy())
    return out


_REF = {}


def reference(c, adam_steps=0, lr=1e-3):
    """(inputs, fp64 oracle) of a case, computed once and shared by the tests of a process; nobody writes to them."""
    key = (c.id, adam_steps, lr)
    if key not in _REF:
        import torch
        inp = inputs(c)
        _REF[key] = (inp, oracle(c, inp, torch.float64, adam_steps, lr))
    return _REF[key]


def e32(c):
    """{term: distance of the fp32 CPU oracle from the fp64 oracle}, the fp32 one under regae_general_cases._fixed_order_fp32."""
    import torch
    inp, ref = reference(c)
    with G._fixed_order_fp32():
        row, g, _ = oracle(c, inp, torch.float32)
    return errors(c, row, g if grad(c) else None, ref[0], ref[1])


def group_e32(cases=None):
    """({term: worst e32 over the cases}, {term: the case that has it})."""
    worst, where = dict.fromkeys(TERMS, 0.0), {}
    for c in CASES if cases is None else cases:
        for term, e in e32(c).items():
            if e > worst[term]:
                worst[term], where[term] = e, c.id
    return worst, where


# term -> largest bar this route may be given: the larger of regae_general_cases.BARS and ae_cases.REGAE_BARS
BAR_CAP = {t: max(G.BARS[t], A.REGAE_BARS[t]) for t in TERMS}

# term -> bar: EIGHT TIMES the worst distance of the fp32 CPU oracle from the fp64 oracle over CASES (group_e32), rounded up to two
# digits - the rule of regae_general_cases.BARS, measured against the oracle, never against the kernels.
# tests/test_regae_ragged_host.py recomputes the maxima, holds every bar between 4 and 16 times its source and below BAR_CAP.
# Worst e32 per term (and its case): loss 4.5e-07 (decoder-without-hidden-layer), ae 1.2e-08 (decoder-one-deeper), npl 1.7e-06
# (decoder-without-hidden-layer), pen 2.7e-09 (loss-decoder-one-deeper), eig 1.5e-06 (regularisers-one-deeper-frozen-encoder-s2), norm
# 6.1e-09 (regularisers-two-deeper-d65), orth 2.1e-06 (decoder-without-hidden-layer), grad 4.5e-06 (decoder-without-hidden-layer).
BARS = dict(loss=3.7e-6, ae=9.5e-8, npl=1.4e-5, pen=2.2e-8, eig=1.3e-5, norm=4.9e-8, orth=1.7e-5, grad=3.6e-5)
