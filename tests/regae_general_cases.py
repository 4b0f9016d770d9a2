"""RegAutoEncoderTask's per-layer route (csrc/regae_general.hip, cvf_regae_general_*): its cases, the Python mirrors of its
workspace formula and of cvf_regae_general_supported, the oracles of the cases and the error bars the GPU module holds it to.

Plain Python at import (no torch, no GPU).  `tests/test_regae_general_host.py` (CPU) checks the mirrors against the library and
ties the bars to the fp32 CPU oracle; `tests/test_regae_general_gpu.py` runs every case through RegAutoEncoderTask._step against
the fp64 oracle.  The hyper-parameters are ae_inputs.REGAE_HYPER (K = 0: no regulariser, gamma = [0, 0]).

The cases are ae_cases.RegCase tuples; what a RegCase cannot say sits in the tables beside them (ACT, LOSS_ONLY, ADAM, FROZEN).
`layout` is "refused" for a chain the fused route refuses (ae_cases.mfma_layout(chain, True)[1] > MFMA_LDS_MAX: the route's
reason to exist) and "small" for a chain it would take, listed in SMALL with the reason a small shape is used - the GPU module
forces the per-layer route on those.  `handoff`: the re-running backward call is also compared with the _reuse one, bit for bit.
"""
import contextlib

from tests import ae_cases as A

RegCase = A.RegCase
TILE = A.TILE
MAX_ROWS = 256                # kMaxRows
SLAB_BYTES = 128 << 20        # kSlabBytes
MAX_WIDTH, MAX_D0, MAX_NETS = 4096, 65536, 8

DIP = dict(d=66, enc=(128, 128), k=2, dec=(128, 128), reg=(128, 128), K=2)       # [66,128,128,2 | 2,128,128,66] + 2 x [2,128,128,1]
BIG = dict(d=384, enc=(256, 64), k=2, dec=(64, 256), reg=(64, 256), K=2)         # [384,256,64,2 | 2,64,256,384] + 2 x [2,64,256,1]
CAP = dict(d=384, enc=(1024,), k=2, dec=(1024,), reg=(8,), K=1)                  # 797 091 parameters: 42 slab rows fit 128 MiB
MANY_B = 64 * 128 + 37        # 129 tiles per half: 258 tiles on 256 slab rows
CAP_B = 64 * 22 + 5           # 23 tiles per half: 46 tiles on 42 slab rows


def _case(id, d, enc, k, dec, reg, K, B, lag_ae, lag_reg, idx=False, layout="small", dup=False, handoff=True):
    return RegCase(id, d, tuple(enc), k, tuple(dec), tuple(reg), K, B, lag_ae, lag_reg, idx, layout, dup, handoff)


CASES = [
    # ---- heads: one, CVF_MAX_NETS with three latents, none (the T-tile form, latent penalties on)
    _case("K1-B5", 6, (8,), 2, (8,), (6,), 1, 5, 1, 2),
    _case("K8-k3-width-31-B65", 7, (9,), 3, (7,), (3,), 8, 65, 2, 1, idx=True),
    _case("K0-width-1-B63", 3, (5,), 2, (1,), (1,), 0, 63, 1, 0),
    # ---- lags: none on the target with a lagged input; both crossing tiles; each with and without the gather
    _case("width-32-lag-input-only", 7, (9,), 2, (24,), (2,), 4, 63, 0, 5),
    _case("width-33-lag-input-only-idx", 7, (9,), 2, (25,), (2,), 4, 64, 0, 3, idx=True),
    _case("width-63-lags-cross-tiles", 6, (8,), 2, (60,), (3,), 1, 130, 70, 67),
    _case("width-64-lags-cross-tiles-idx", 6, (8,), 2, (60,), (2,), 2, 130, 70, 67, idx=True),
    # ---- merged widths past one 64-row block
    _case("width-65", 5, (7,), 1, (64,), (1,), 1, 130, 1, 2),
    _case("width-130", 9, (12,), 2, (100,), (15,), 2, 257, 3, 64, idx=True),
    # ---- depth, frozen encoder
    _case("twelve-layers-K0", 10, (9, 8, 7, 6, 5), 2, (5, 6, 7, 8, 9), (1, 1, 1, 1, 1), 0, 130, 2, 0, idx=True),
    _case("frozen-encoder", 9, (12, 7), 3, (7, 12), (5, 4), 4, 63, 2, 3, idx=True),
    # ---- more tiles than slab rows
    _case("many-tiles", 3, (4,), 1, (4,), (2,), 1, MANY_B, 1, 2, dup=True, handoff=False),
    _case("slab-capped", B=CAP_B, lag_ae=1, lag_reg=2, layout="refused", handoff=False, **CAP),
    # ---- the chains the route exists for
    _case("dipeptide-B130", B=130, lag_ae=1, lag_reg=2, idx=True, layout="refused", **DIP),
    _case("dipeptide-B1001", B=1001, lag_ae=2, lag_reg=1, layout="refused", handoff=False, **DIP),
    _case("large-molecule-B65", B=65, lag_ae=1, lag_reg=2, idx=True, layout="refused", **BIG),
    # ---- loss only
    _case("loss-dipeptide-K0-B1", B=1, lag_ae=1, lag_reg=0, layout="refused", handoff=False, **dict(DIP, K=0)),
    _case("loss-width-31-B1001", 7, (9,), 3, (7,), (3,), 8, 1001, 2, 1, idx=True, handoff=False),
]
LOSS_ONLY = {"loss-dipeptide-K0-B1", "loss-width-31-B1001"}
FROZEN = {"frozen-encoder"}
# activation other than tanh (each of the six codes once over the table).  Sigmoid and the twelve-layer chain go with K = 0: behind
# randomly initialised sigmoid layers, or six narrow layers deep, a head's variance is so much smaller than its squared mean that
# the fp32 CPU oracle itself ends 1e-3 to 1e-1 from the fp64 one in npl, eig and the gradient - no measure of a kernel.
ACT = {"K0-width-1-B63": "sigmoid", "width-32-lag-input-only": "relu", "width-33-lag-input-only-idx": "elu",
       "width-63-lags-cross-tiles": "leaky_relu", "width-64-lags-cross-tiles-idx": "softplus"}
# Three fused Adam steps against the fp64 oracle's, at the sweep's ADAM_TOL = 2e-6: cases whose fp32 CPU oracle itself stays
# within ADAM_TOL / 8 of the fp64 one after those steps (tests/test_regae_general_host.py recomputes it; see
# ae_general_cases.ADAM_SOURCE_MAX for why chains with gradient entries next to zero are excluded).  Every case with a gradient
# runs the three steps for the structural zeros and the frozen entries; these are compared with the oracle's parameters too.
ADAM = {"K0-width-1-B63"}
ADAM_SOURCE_MAX = 2e-6 / 8

_EDGE = "a merged width at an edge of aeg_layer_kernel's 64-row block / 32-deep K stage, at the smallest chain that has it"
SMALL = {
    "K1-B5": "one head on a batch of five frames: the smallest 2 T-tile launch",
    "K8-k3-width-31-B65": _EDGE + "; CVF_MAX_NETS heads on three latents",
    "K0-width-1-B63": _EDGE + "; no heads: the T-tile form with the latent penalties",
    "width-32-lag-input-only": _EDGE, "width-33-lag-input-only-idx": _EDGE, "width-63-lags-cross-tiles": _EDGE,
    "width-64-lags-cross-tiles-idx": _EDGE, "width-65": _EDGE, "width-130": _EDGE,
    "twelve-layers-K0": "CVF_MAX_LAYERS layers; narrow, so that the fp64 oracle of twelve layers stays cheap",
    "frozen-encoder": "the mask on a frozen encoder, at ae_cases' regae-K4-B63 chain",
    "many-tiles": "258 tiles on 256 slab rows needs 8 229 frames: the chain is tiny so that the case takes no time",
}


def act(c):
    return ACT.get(c.id, "tanh")


def grad(c):
    return c.id not in LOSS_ONLY


def hyper(c):
    from tests import ae_inputs as I
    h = dict(I.REGAE_HYPER)
    if c.K == 0:
        h["gamma"] = [0.0, 0.0]
    return h


def chain(c):
    return A.regae_dims(c)[3]


def n_enc_layers(c):
    return len(c.enc) + 1


def acts(c):
    """cvf_mlp_desc.act of the merged chain: the activation's code after every layer but the encoder's and the chain's last."""
    d, code = chain(c), A.ACTS.index(act(c)) + 1
    return [0 if l in (n_enc_layers(c) - 1, len(d) - 2) else code for l in range(len(d) - 1)]


def mlp_desc(c):
    """cvf_mlp_desc of the merged chain as core._RegFlatParams lays it out (dense layers, W then b, in chain order)."""
    from colvarsfinder import _hip
    m, d, ac, pos = _hip.MLPDesc(), chain(c), acts(c), 0
    m.n_nets, m.n_layers = 1, len(d) - 1
    for l in range(len(d) - 1):
        m.dims[l], m.dims[l + 1], m.act[l] = d[l], d[l + 1], ac[l]
        m.w_off[0][l], pos = pos, pos + d[l] * d[l + 1]
        m.b_off[0][l], pos = pos, pos + d[l + 1]
    m.n_params = pos
    return m


# ---------------------------------------------------------------------------------------------------- the host's rules
def n_tiles(B):
    return (B + TILE - 1) // TILE


def slab_rows(d, tiles):
    """g64_rows (csrc/cvf_gemm64.hpp): min(tiles, 256, 128 MiB / (4 n_params)), at least 1."""
    return max(1, min(tiles, MAX_ROWS, SLAB_BYTES // (4 * A.n_params(d))))


def scratch_floats(d, B):
    """regaeg_layout, always for 2 T tiles: the tiled input and the saved activations a_1..a_{L-1}, two adjoint images as wide as
    the widest of dims[1..L], the slab rows, (rounded up to even) two doubles per base tile."""
    T = n_tiles(B)
    images = 2 * T * TILE * (sum(d[:-1]) + 2 * max(d[1:]))
    return ((images + slab_rows(d, 2 * T) * A.n_params(d) + 1) & ~1) + 4 * T


def supported(d, K, n_enc, acts_):
    """regaeg_why for a chain built by mlp_desc (one net, valid activation codes, parameters filling the buffer)."""
    L = len(d) - 1
    blocks = lambda l: ((d[l + 1] + 63) // 64) * ((d[l] + 1 + 63) // 64)   # aeg_wgrad_kernel's grid.y for layer l
    return (2 <= L <= A.MAX_LAYERS and 0 <= K <= MAX_NETS and d[L] == d[0] + K and 1 <= d[0] <= MAX_D0
            and all(1 <= h <= MAX_WIDTH for h in d[1:L]) and all(blocks(l) <= 65535 for l in range(L))
            and 1 <= n_enc < L and acts_[n_enc - 1] == 0 and d[n_enc] <= MAX_NETS)


def fused_refuses(c):
    return A.mfma_layout(chain(c), True)[1] > A.MFMA_LDS_MAX


# ---------------------------------------------------------------------------------------------------- oracles
TERMS = A.REGAE_TERMS


def _rounded(fn):
    """An activation evaluated in fp64 and rounded to its argument's precision, as ae_inputs._rounded_tanh: torch's fp32 vector
    functions differ in their last digit between instruction sets."""
    return lambda x: fn(x.double()).to(x.dtype)


def oracle(c, inp, dtype, adam_steps=0, lr=1e-3):
    """ae_inputs.regae_oracle for these cases: the first step's loss row [loss, ae, npl, pen, eig_1..K, 0, norm, orth] and flat
    gradient (state-dict order), float64 - with the case's activation, K = 0 (no regulariser terms) and a frozen encoder (zero
    gradient, no update); with adam_steps > 0 also the flat parameters after that many torch.optim.Adam steps on the batch."""
    import numpy as np
    import torch
    from oracle import losses
    from tests import ae_inputs as I
    traj, w, idx, eig_w, sd0 = inp
    h, K = hyper(c), c.K
    F, W = torch.as_tensor(traj).to(dtype), torch.as_tensor(w.astype(np.float32)).double()
    frozen = c.id in FROZEN
    sd = {k: p.to(dtype).clone().requires_grad_(not (frozen and k.startswith("encoder."))) for k, p in sd0.items()}
    fn = I._rounded_tanh if act(c) == "tanh" else _rounded(I.ACT_FN[act(c)])

    def terms():
        ae = losses.regae_mse(sd, F[idx], F[idx + c.lag_ae], W[idx], activation=fn)
        if K > 0:
            eig, npl, pen, cvec = losses.regae_eigen_loss(sd, K, F[idx], W[idx], F[idx + c.lag_reg], W[idx + c.lag_reg], eig_w=eig_w,
                                                          lag_idx=c.lag_reg, dt=h["dt"], activation=fn)
        else:
            eig, npl, pen, cvec = [], torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64), []
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


def errors(c, row, grad_, ref_row, ref_grad):
    """ae_inputs.regae_errors for these cases: {term: error}, relative (eig: the worst eigenvalue), the gradient's of its
    largest entry; K = 0 has no npl / pen / eig, a loss-only case no grad."""
    import numpy as np
    K = c.K
    # (a term whose fp64 value is the rounding noise of an exact zero - the covariance penalty of a one-frame batch - is held to
    #  its absolute error)
    rel = lambda i: abs(row[i] - ref_row[i]) / (abs(ref_row[i]) if abs(ref_row[i]) > 1e-25 else 1.0)
    out = dict(loss=rel(0), ae=rel(1), norm=rel(5 + K), orth=rel(6 + K))
    if K > 0:
        out.update(npl=rel(2), pen=rel(3), eig=max(rel(4 + i) for i in range(K)))
    if grad_ is not None:
        out["grad"] = float(np.abs(grad_ - ref_grad).max() / np.abs(ref_grad).max())
    return out


@contextlib.contextmanager
def _fixed_order_fp32():
    """ae_inputs.regae_e32's setting: one thread, the Linear layers' sums in a fixed order."""
    import torch
    from tests import ae_inputs as I
    n, linear = torch.get_num_threads(), torch.nn.functional.linear
    torch.set_num_threads(1)
    torch.nn.functional.linear = I._FixedOrderLinear.apply
    try:
        yield
    finally:
        torch.nn.functional.linear = linear
        torch.set_num_threads(n)


def e32(c, inp=None, ref=None):
    """{term: distance of the fp32 CPU oracle from the fp64 oracle} (ae_inputs.regae_e32's rule, on `oracle` above)."""
    import torch
    from tests import ae_inputs as I
    inp = I.regae_inputs(c) if inp is None else inp
    ref = oracle(c, inp, torch.float64) if ref is None else ref
    with _fixed_order_fp32():
        row, g, _ = oracle(c, inp, torch.float32)
    return errors(c, row, g if grad(c) else None, ref[0], ref[1])


def group_e32(cases=None):
    """{term: worst e32 over the cases}; a loss-only case enters without its gradient, a K = 0 case without the head terms."""
    worst = dict.fromkeys(TERMS, 0.0)
    for c in CASES if cases is None else cases:
        for term, e in e32(c).items():
            worst[term] = max(worst[term], e)
    return worst


# term -> bar: EIGHT TIMES the worst distance of the fp32 CPU oracle from the fp64 oracle over CASES (group_e32), rounded up to
# two digits - the rule of ae_cases.REGAE_BARS, measured against the oracle, never against the kernels.
# tests/test_regae_general_host.py recomputes the maxima and holds every bar between 4 and 16 times its source.
# Worst e32 per term (and its case): loss 2.3e-07 (frozen-encoder), ae 3.4e-08 (K1-B5), npl 1.8e-06 (width-63-lags-cross-tiles), pen
# 2.4e-09 (width-63-lags-cross-tiles), eig 3.3e-06 (frozen-encoder), norm 5.6e-09 (large-molecule-B65), orth 4.9e-06 (slab-capped),
# grad 3.2e-05 (K1-B5).
BARS = dict(loss=1.8e-6, ae=2.8e-7, npl=1.5e-5, pen=1.9e-8, eig=2.7e-5, norm=4.5e-8, orth=4.0e-5, grad=2.5e-4)
