"""The fp64 end of every eigenfunction route, tested on its own: cases, input builders, references and the mirrored host rules
for tests/test_stats_tail_cases.py (CPU) and tests/test_stats_tail_gpu.py (GPU).

Under test: the batch sums (ef_stats_partial_kernel<K, LAG>, csrc/stats.hip), the fixed-order row reduction
(ef_stats_finish_kernel, three pass shapes, rows [row][ns] and [ns][row]), the one-wave loss tail with its partial derivatives
(ef_loss_tail_wave, csrc/cvf_loss_tail.hpp) and RegAutoEncoderTask's two scalar kernels (regae_enc_loss_kernel,
regae_loss_row_kernel, csrc/ae.hip).  Plain Python: numpy, torch on the CPU, mpmath.  No GPU.

The rules below mirror the host dispatch; the comments name the functions they copy.  If those change, change them too.

References.  Sums: the terms from the fp32 inputs, upcast (one rounding each), added exactly (math.fsum).  Tail: oracle/stats.py
(loss_from_stats) in torch fp64 with autograd in the sums, mapped to the `coef` layout of include/cvf.h (ref_tail); and the same
loss in mpmath at 50 digits with every `coef` entry a central difference in the one sum include/cvf.h names for it, ordering
held fixed (hp_tail), so that the check of the map and of the kernels does not repeat the kernel's closed forms; the 50-digit
side finds the sums by walking the layout (stat_names) and shares no index code with the fp64 side.

Bars.  Sums: |got - ref| <= (B + 3) 2^-53 sum_b |t_b| per statistic (at most three roundings per term, B - 1 additions in some
order, one rounding in the reference's term); rows: n_rows 2^-53 sum |rows|.  Tail and encoder terms, per output group:
8 e_ref + 16 2^-53 s with e_ref = max |ref_tail - hp_tail| over the group (the fp64 oracle's own error) and s the group's largest
magnitude (tail_bars).  Nothing here is taken from what a kernel returns.
"""
import functools
import math
from collections import namedtuple

import mpmath
import numpy as np
import torch

from oracle import stats as ostats

MAX_NETS = 8            # CVF_MAX_NETS (include/cvf.h)
TILE = 64               # CVF_TILE
STAT_BLOCKS = 128       # kStatBlocks (csrc/stats.hip)
MAX_ROWS16 = 16384      # kMaxRows16 (csrc/ef16_common.hpp)
MODES = ("gen", "tr")
EPS = 2.0 ** -53
MARGIN, FLOOR = 8.0, 16.0 * EPS   # tail bar: MARGIN e_ref + FLOOR s


# ------------------------------------------------------------------------------------------------ mirrored rules
def npair(k):
    return k * (k + 1) // 2     # CVF_NPAIR


def nstats(k, lag):
    """cvf_ef_nstats (csrc/stats.hip)."""
    base = 1 + k + npair(k)
    return base + k if lag == 0 else base + 1 + 2 * k + k


def loss_len(k):
    return 3 + 2 * k            # CVF_LOSS_LEN


def coef_len(k):
    return 4 * k + k * k        # CVF_COEF_LEN


def finish_pass(ns):
    """(kSt, kR) of the pass ef_stats_finish_kernel takes; nw: the launch's waves (cvf_ef_stats_finish_ll, csrc/stats.hip)."""
    nw = min(ns, 16)
    if ns <= nw:
        return (1, 24)
    if ns <= 2 * nw:
        return (2, 20)
    return (4, 6)


def ef16_rows(B):
    """cvf_ef16_rows (csrc/ef16_front.hip): four 16-frame units per 64-frame tile; 0 above the cap kMaxRows16."""
    units = 4 * ((B + TILE - 1) // TILE)
    return units if units <= MAX_ROWS16 else 0


def stat_grid(B):
    """Blocks (= rows of partial sums) of ef_stats_partial_kernel (ef_stats_impl, csrc/stats.hip)."""
    return min((B + TILE - 1) // TILE, STAT_BLOCKS)


def partial_instance(k, mode):
    """ef_stats_partial_kernel<K, LAG> that ef_stats_impl launches (k_dispatch, csrc/stats.hip)."""
    return ("ef_stats_partial_kernel", k, int(mode == "tr"))


def pidx(k, a, b):
    """Index of S2(a, b) among the pairs i <= j, row-major (include/cvf.h)."""
    lo, hi = min(a, b), max(a, b)
    return lo * k - lo * (lo - 1) // 2 + (hi - lo)


# ------------------------------------------------------------------------------------------------ cases
KM = [(k, mode) for k in range(1, MAX_NETS + 1) for mode in MODES]
SMALL_B = (1, 63, 64, 65)
BIG_B = (64 * 127 + 1, 64 * 128, 64 * 128 + 1, 2 * 64 * 128 + 1)   # (128 blocks, ragged) (128, full) (block 0 walks two tiles) (all walk two+)


def stats_batches(k, mode):
    """Batches of the (k, mode) instance: the small four and two of BIG_B, one of them above 8192."""
    r = k + 2 * (mode == "tr")      # (mixes k and mode: over k = 1..8 each mode meets all four of BIG_B)
    return SMALL_B + (BIG_B[r % 4], BIG_B[(r + 2) % 4])


def claimed():
    return {partial_instance(k, mode) for k, mode in KM}


def row_counts(k, mode):
    """Row counts of cvf_ef_stats_finish_rows for this (k, mode): around one lane sweep and around R = 64 kR rows, the most
    one wave loads per statistic and trip of its row loop."""
    R = 64 * finish_pass(nstats(k, lag_of(k, mode)))[1]
    return (1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 5)


def ef16_batches(k, mode):
    """Batches B of cvf_ef16_finish: their rows (4 ceil(B / 64)) are the multiples of 4 on either side of row_counts(), the rows
    of B = 20 000 and the cap."""
    rows = sorted({4 * ((n + 3) // 4) for n in row_counts(k, mode)} | {4 * (n // 4) for n in row_counts(k, mode) if n >= 4})
    return tuple(16 * r for r in rows) + (20000, 64 * MAX_ROWS16 // 4)


ALPHA, BETA, DT = 7.5, 1.3, 0.4
EIG_W = ((1.0, 0.8, 0.64, 0.512, 0.4096, 0.32768, 0.262144, 0.2097152),    # decreasing
         (0.6, 1.0, 0.3, 0.9, 0.2, 0.7, 0.5, 0.4))                         # non-monotone
EIG_W_PAD = 777.0   # cfg.eig_w past k: never read (ef_loss_tail_wave selects by the clamped net index)


def lag_of(k, mode, wsel=0):
    return 0 if mode == "gen" else (1, 3)[(k + wsel) % 2]


TailCase = namedtuple("TailCase", "id k mode sort wsel tie")
TIE_PAIRS = {2: (0, 1), 4: (1, 3), 8: (2, 6)}
TAIL_CASES = [TailCase(f"{mode}-k{k}-sort{sort}-w{wsel}", k, mode, sort, wsel, None)
              for k, mode in KM for sort in (0, 1) for wsel in (0, 1)]
TIE_CASES = [TailCase(f"{mode}-k{k}-tie", k, mode, 1, 0, TIE_PAIRS[k]) for k in (2, 4, 8) for mode in MODES]


def cfg_of(case):
    """The scalars of cvf_ef_cfg for a tail case."""
    return make_cfg(case.k, case.mode, case.sort, case.wsel)


def make_cfg(k, mode, sort=1, wsel=0):
    return dict(k=k, lag_idx=lag_of(k, mode, wsel), sort_eigvals=sort, alpha=ALPHA, beta=BETA, dt=DT,
                eig_w=tuple(EIG_W[wsel][:k]) + (EIG_W_PAD,) * (MAX_NETS - k))


# ------------------------------------------------------------------------------------------------ input builders
VARIANCES = (0.45, 1.9, 0.7, 1.35, 2.2, 0.55, 1.6, 0.8)   # of y: in 0.3 .. 2.5, none at 1


def _perm(k):
    """A fixed order of the nets that is not the identity for k >= 2: the rank of (5 i + 3) mod 8."""
    key = [(5 * i + 3) % 8 for i in range(k)]
    return [sorted(key).index(v) for v in key]


@functools.lru_cache(maxsize=None)
def sample(k, mode, n, seed=0, tie=None, f32=False):
    """Deterministic frames: w in [0.5, 1.5]; y = z A + m with a fixed mixing matrix A (a common factor with loadings of mixed
    sign: covariances far from 0, variances VARIANCES) and non-zero means; generator: e >= 0 with prescribed ratios
    sum w e_i / var_i = 1.35^p_i; transfer: y_lag = y + noise whose variance sets the eigenvalues to 0.08 * 1.35^p_i, and
    w_lag; p = _perm(k), so the unsorted order is not the identity and the relative gaps are ~0.3.  tie = (a, b): column b is a
    bit-copy of column a everywhere.  f32: every array rounded to fp32 (returned as fp64)."""
    rs = np.random.RandomState(1000 * k + 100 * (mode == "tr") + seed)
    sig = np.sqrt(np.array(VARIANCES[:k]))
    rho = np.array([(0.35 + 0.2 * (i % 3)) * (-1) ** i for i in range(k)])
    A = np.vstack([np.diag(sig * np.sqrt(1 - rho ** 2)), sig * rho])         # [k + 1, k]
    m = np.array([(0.5 + 0.25 * i) * (-1) ** (i // 2) for i in range(k)])
    z = rs.standard_normal((n, k + 1))
    y = z @ A + m
    w = rs.uniform(0.5, 1.5, n)
    p = np.array(_perm(k), dtype=np.float64)
    out = dict(w=w, y=y)
    if mode == "gen":
        out["e"] = (1.35 ** p) * sig ** 2 * rs.uniform(0.5, 1.5, (n, k))
    else:
        t = 0.08 * 1.35 ** p
        q = 2 * t / (1 - t)                                                  # noise variance / var: eig ~ q / (2 + q) = t
        out["y_lag"] = y + rs.standard_normal((n, k)) * sig * np.sqrt(q)
        out["w_lag"] = rs.uniform(0.5, 1.5, n)
    if tie is not None:
        for name in ("y", "e", "y_lag"):
            if name in out:
                out[name][:, tie[1]] = out[name][:, tie[0]]
    if f32:
        out = {name: a.astype(np.float32).astype(np.float64) for name, a in out.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


def tiled(a, B, garbage=None):
    """[B][k] -> fp32 [T][k][64]; the padded lanes of the last tile are 0, or with garbage = seed finite values of magnitude
    ~1e3 and mixed sign that copy no frame (the header's promise: padding weight is forced to 0)."""
    k = a.shape[1]
    T = (B + TILE - 1) // TILE
    out = np.zeros((T * TILE, k), dtype=np.float32)
    out[:B] = a[:B]
    if garbage is not None:
        rs = np.random.RandomState(77 + garbage)
        out[B:] = (rs.uniform(500.0, 2000.0, (T * TILE - B, k)) * rs.choice([-1.0, 1.0], (T * TILE - B, k))).astype(np.float32)
    return np.ascontiguousarray(out.reshape(T, TILE, k).transpose(0, 2, 1)).reshape(-1)


def stat_terms(s, B, k, mode):
    """[ns][B] fp64: the term of every statistic for every frame (layout of include/cvf.h), from the (fp32-valued) inputs."""
    w, y = s["w"][:B], s["y"][:B]
    rows = [w] + [w * y[:, i] for i in range(k)] + [w * y[:, i] * y[:, j] for i in range(k) for j in range(i, k)]
    if mode == "gen":
        rows += [w * s["e"][:B, i] for i in range(k)]
    else:
        wl, yl = s["w_lag"][:B], s["y_lag"][:B]
        rows += [wl] + [wl * yl[:, i] for i in range(k)] + [wl * yl[:, i] * yl[:, i] for i in range(k)]
        rows += [w * (yl[:, i] - y[:, i]) * (yl[:, i] - y[:, i]) for i in range(k)]
    return np.stack(rows)


def ref_sums(s, B, k, mode):
    """(sums, sum of |terms|) per statistic, exact summation of the fp64 terms."""
    t = stat_terms(s, B, k, mode)
    return (np.array([math.fsum(r) for r in t.tolist()]), np.array([math.fsum(r) for r in np.abs(t).tolist()]))


def sums_bar(B, abs_sums):
    return (B + 3) * EPS * abs_sums


def ref_rowsum(partial):
    """partial [n_rows][ns] -> (sums, sum of |rows|) per statistic, exact."""
    t = np.asarray(partial).T
    return (np.array([math.fsum(r) for r in t.tolist()]), np.array([math.fsum(r) for r in np.abs(t).tolist()]))


def rows_bar(n_rows, abs_sums):
    return n_rows * EPS * abs_sums


@functools.lru_cache(maxsize=None)
def _row_pool(k, mode):
    ns = nstats(k, lag_of(k, mode))
    rs = np.random.RandomState(5000 + 10 * k + (mode == "tr"))
    a = 10.0 ** rs.uniform(-3.0, 3.0, (MAX_ROWS16, ns)) * rs.choice([-1.0, 1.0], (MAX_ROWS16, ns))
    a.setflags(write=False)
    return a


def synth_rows(k, mode, n_rows):
    """[n_rows][ns] fp64 rows of mixed sign, magnitudes 1e-3 .. 1e3, whose sum is the sums vector of the (k, mode) tail sample
    up to one rounding: the last row is that vector minus the exact sum of the others (so it can be larger), and the tail of
    the reduced sums is a well-posed loss.  Every |entry| >= 1e-3 stays above rows_bar: a dropped or doubled row is seen."""
    target = tail_sums(k, mode).numpy()
    rows = np.array(_row_pool(k, mode)[:n_rows])
    if n_rows == 1:
        rows[0] = target
    else:
        rows[-1] = target - ref_rowsum(rows[:-1])[0]
    return rows


# ------------------------------------------------------------------------------------------------ tail references
@functools.lru_cache(maxsize=None)
def tail_sums(k, mode, tie=None, n=512):
    """The batch sums (oracle.stats.batch_stats, fp64) of the 512-frame fp64 sample: consistent by construction."""
    s = {name: torch.tensor(a) for name, a in sample(k, mode, n, 0, tie).items()}
    if mode == "gen":
        return ostats.batch_stats(s["y"], s["w"], dirichlet=s["e"])
    return ostats.batch_stats(s["y"], s["w"], y_lag=s["y_lag"], w_lag=s["w_lag"])


def case_sums(case):
    return tail_sums(case.k, case.mode, case.tie)


COEF_GROUPS = ("gS1", "gS2", "gET", "gS1l", "gS2l")
GROUPS = ("loss", "eig") + COEF_GROUPS


def coef_groups_from_grad(g, k, lag):
    """d loss / d sums -> the groups of `coef` (include/cvf.h): gS1 = d/dS1; gS2[i][j] = gS2[j][i] = d/dS2(min, max) (the full
    symmetric matrix holds the derivative with respect to the ONE stored sum in both places); gE_or_gT; gS1', gS2'_ii (zero in
    generator mode)."""
    o = 1 + k + npair(k)
    out = {"gS1": [g[1 + i] for i in range(k)],
           "gS2": [g[1 + k + pidx(k, i, j)] for i in range(k) for j in range(k)]}
    if lag == 0:
        out.update(gET=[g[o + i] for i in range(k)], gS1l=[0.0] * k, gS2l=[0.0] * k)
    else:
        out.update(gET=[g[o + 1 + 2 * k + i] for i in range(k)], gS1l=[g[o + 1 + i] for i in range(k)],
                   gS2l=[g[o + 1 + k + i] for i in range(k)])
    return out


def coef_vector(groups):
    """[gS1(k), gS2(k*k), gE_or_gT(k), gS1'(k), gS2'_ii(k)] as cvf_ef_loss writes it."""
    return np.concatenate([np.asarray(groups[g], dtype=np.float64) for g in COEF_GROUPS])


def ref_tail(sums, cfg):
    """oracle.stats.loss_from_stats in torch fp64, autograd in the sums -> {group: fp64 array} + "cvec" (ints)."""
    k, lag = cfg["k"], cfg["lag_idx"]
    s = torch.as_tensor(sums, dtype=torch.float64).clone().requires_grad_(True)
    loss, eig, npl, pen, cvec = ostats.loss_from_stats(s, k, alpha=cfg["alpha"], eig_w=list(cfg["eig_w"][:k]), beta=cfg["beta"],
                                                       lag_idx=lag, dt=cfg["dt"], sort_eigvals=bool(cfg["sort_eigvals"]))
    (g,) = torch.autograd.grad(loss, s)
    out = {name: np.array([float(v) for v in vals]) for name, vals in coef_groups_from_grad(g, k, lag).items()}
    out["loss"] = np.array([float(loss.detach()), float(npl.detach()), float(pen.detach())])
    out["eig"] = eig.detach().numpy().copy()
    out["cvec"] = np.array(cvec, dtype=np.int64)
    return out


def stat_names(k, lag):
    """{name: position} of the statistics vector, written out from the comment in include/cvf.h by walking it once - no index
    formula: generator [W, S1(k), S2(i <= j, row-major), E(k)], transfer [W, S1(k), S2(..), W', S1'(k), S2'_ii(k), T(k)].  The
    50-digit side (_hp_loss, hp_tail, hp_enc) reads and perturbs the sums through this table only, so that it shares neither
    pidx nor coef_groups_from_grad with the fp64 side it checks."""
    names = ["W"] + [("S1", i) for i in range(k)]
    for i in range(k):
        for j in range(i, k):
            names.append(("S2", i, j))
    if lag == 0:
        names += [("E", i) for i in range(k)]
    else:
        names += ["Wl"] + [("S1l", i) for i in range(k)] + [("S2l", i) for i in range(k)] + [("T", i) for i in range(k)]
    return {name: n for n, name in enumerate(names)}


def _hp_loss(s, cfg, cvec):
    """(loss, npl, pen, eig) of core.py:406-457 from the sums, in the working precision of mpmath; cvec given."""
    k, lag = cfg["k"], cfg["lag_idx"]
    at = stat_names(k, lag)
    W = s[at["W"]]
    m = [s[at["S1", i]] / W for i in range(k)]
    v = [s[at["S2", i, i]] / W - m[i] ** 2 for i in range(k)]
    if lag == 0:
        num, den, pref = [s[at["E", i]] for i in range(k)], v, 1 / (W * mpmath.mpf(cfg["beta"]))
    else:
        Wl = s[at["Wl"]]
        ml = [s[at["S1l", i]] / Wl for i in range(k)]
        vl = [s[at["S2l", i]] / Wl - ml[i] ** 2 for i in range(k)]
        num, den = [s[at["T", i]] for i in range(k)], [v[i] + vl[i] for i in range(k)]
        pref = 1 / (mpmath.mpf(cfg["dt"]) * lag) / W
    eig = [pref * num[i] / den[i] for i in range(k)]
    npl = mpmath.mpf(0)
    for idx in range(k):
        c = cvec[idx]
        npl += mpmath.mpf(cfg["eig_w"][idx]) * num[c if lag == 0 else idx] / den[c]
    npl *= pref
    pen = sum(((vi - 1) ** 2 for vi in v), mpmath.mpf(0))
    for i in range(k):
        for j in range(i + 1, k):
            pen += (s[at["S2", i, j]] / W - m[i] * m[j]) ** 2
    return npl + mpmath.mpf(cfg["alpha"]) * pen, npl, pen, eig


def _central(f, s, n):
    """d f / d s_n by a central difference with a relative step of 1e-15 at 50 digits (truncation ~1e-30, rounding ~1e-35)."""
    h = (abs(s[n]) if s[n] != 0 else mpmath.mpf(1)) * mpmath.mpf("1e-15")
    up, dn = list(s), list(s)
    up[n], dn[n] = s[n] + h, s[n] - h
    return (f(up) - f(dn)) / (2 * h)


def hp_tail(sums, cfg):
    """The groups of ref_tail in mpmath at 50 digits, filled entry by entry from the definition in include/cvf.h: each `coef`
    entry is the central difference of the loss in the ONE sum the header names for it (ordering held fixed), found through
    stat_names - not through coef_groups_from_grad or pidx.  Entries are mpf; "cvec" is the stable order of the 50-digit
    eigenvalues."""
    k, lag = cfg["k"], cfg["lag_idx"]
    with mpmath.workdps(50):
        s = [mpmath.mpf(float(x)) for x in sums]
        at = stat_names(k, lag)
        assert len(at) == len(s), (len(at), len(s))
        eig = _hp_loss(s, cfg, list(range(k)))[3]
        cvec = sorted(range(k), key=lambda i: (eig[i], i)) if cfg["sort_eigvals"] else list(range(k))
        loss, npl, pen, _ = _hp_loss(s, cfg, cvec)

        def d(name):
            return _central(lambda t: _hp_loss(t, cfg, cvec)[0], s, at[name])
        out = {"gS1": [d(("S1", i)) for i in range(k)]}
        pair = {(i, j): d(("S2", i, j)) for i in range(k) for j in range(i, k)}       # one difference per STORED sum
        out["gS2"] = [pair[(min(i, j), max(i, j))] for i in range(k) for j in range(k)]   # [i][j] row-major, both triangles
        if lag == 0:
            out["gET"] = [d(("E", i)) for i in range(k)]
            out["gS1l"], out["gS2l"] = [mpmath.mpf(0)] * k, [mpmath.mpf(0)] * k
        else:
            out["gET"] = [d(("T", i)) for i in range(k)]
            out["gS1l"] = [d(("S1l", i)) for i in range(k)]
            out["gS2l"] = [d(("S2l", i)) for i in range(k)]
        out["loss"] = [loss, npl, pen]
        out["eig"] = [eig[c] for c in cvec]
        out["cvec"] = np.array(cvec, dtype=np.int64)
    return out


def _group_error(ref, hp):
    """(e_ref, s): the largest |ref - hp| and the largest |hp| over a group."""
    with mpmath.workdps(50):
        e = max([abs(mpmath.mpf(float(r)) - h) for r, h in zip(ref, hp)], default=mpmath.mpf(0))
        s = max([abs(h) for h in hp], default=mpmath.mpf(0))
        return float(e), float(s)


def bars_from(ref, hp, groups):
    """{group: (bar, e_ref, s)} with bar = 8 e_ref + 16 2^-53 s."""
    out = {}
    for g in groups:
        e, s = _group_error(ref[g], hp[g])
        out[g] = (MARGIN * e + FLOOR * s, e, s)
    return out


_BARS = {}


def tail_bars(sums, cfg):
    """{group: (bar, e_ref, s)} of the tail at these sums (cached by the sums' bits and the scalars)."""
    key = (np.asarray(sums, dtype=np.float64).tobytes(), tuple(sorted((n, v) for n, v in cfg.items())))
    if key not in _BARS:
        ref, hp = ref_tail(sums, cfg), hp_tail(sums, cfg)
        assert list(ref["cvec"]) == list(hp["cvec"]), (cfg, ref["cvec"], hp["cvec"])
        _BARS[key] = bars_from(ref, hp, GROUPS)
    return _BARS[key]


def split_outputs(loss_vec, coef, k):
    """The kernel's loss_vec and coef (arrays of at least CVF_LOSS_LEN / CVF_COEF_LEN doubles) -> {group: array}."""
    lv, cf = np.asarray(loss_vec, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    return {"loss": lv[:3], "eig": lv[3:3 + k], "cvec": lv[3 + k:3 + 2 * k], "gS1": cf[:k], "gS2": cf[k:k + k * k],
            "gET": cf[k + k * k:2 * k + k * k], "gS1l": cf[2 * k + k * k:3 * k + k * k], "gS2l": cf[3 * k + k * k:4 * k + k * k]}


# ------------------------------------------------------------------------------------------------ encoder regularisers
ENC_ETAS = ((1.5, 0.7), (0.0, 0.7), (1.5, 0.0))
ENC_GROUPS = ("terms", "gS1", "gS2")


def ref_enc(sums, k, eta1, eta2):
    """terms = {sum (var - 1)^2, sum_{i<j} cov^2} (core.py:934, 966) and coef = d(eta1 terms0 + eta2 terms1) / d{S1, S2} in
    the [gS1(k), gS2(k*k) symmetric] layout, torch fp64 autograd in the sums."""
    s = torch.as_tensor(sums, dtype=torch.float64)[:1 + k + npair(k)].clone().requires_grad_(True)
    W = s[0]
    m = [s[1 + i] / W for i in range(k)]
    tn = sum((s[1 + k + pidx(k, i, i)] / W - m[i] * m[i] - 1) ** 2 for i in range(k))
    to = sum(((s[1 + k + pidx(k, i, j)] / W - m[i] * m[j]) ** 2 for i in range(k) for j in range(i + 1, k)), 0 * W)
    (g,) = torch.autograd.grad(eta1 * tn + eta2 * to, s)
    return {"terms": np.array([float(tn.detach()), float(to.detach())]),
            "gS1": np.array([float(g[1 + i]) for i in range(k)]),
            "gS2": np.array([float(g[1 + k + pidx(k, i, j)]) for i in range(k) for j in range(k)])}


def hp_enc(sums, k, eta1, eta2):
    """The same at 50 digits; sums read and perturbed through stat_names, one central difference per stored sum."""
    with mpmath.workdps(50):
        at = stat_names(k, 0)
        s = [mpmath.mpf(float(x)) for x in list(sums)[:1 + k + npair(k)]]

        def terms(t):
            W = t[at["W"]]
            m = [t[at["S1", i]] / W for i in range(k)]
            tn = sum(((t[at["S2", i, i]] / W - m[i] ** 2 - 1) ** 2 for i in range(k)), mpmath.mpf(0))
            to = sum(((t[at["S2", i, j]] / W - m[i] * m[j]) ** 2 for i in range(k) for j in range(i + 1, k)), mpmath.mpf(0))
            return tn, to

        def f(t):
            a, b = terms(t)
            return mpmath.mpf(eta1) * a + mpmath.mpf(eta2) * b
        tn, to = terms(s)
        pair = {(i, j): _central(f, s, at["S2", i, j]) for i in range(k) for j in range(i, k)}
        return {"terms": [tn, to], "gS1": [_central(f, s, at["S1", i]) for i in range(k)],
                "gS2": [pair[(min(i, j), max(i, j))] for i in range(k) for j in range(k)]}


def enc_bars(sums, k, eta1, eta2):
    return bars_from(ref_enc(sums, k, eta1, eta2), hp_enc(sums, k, eta1, eta2), ENC_GROUPS)


# ------------------------------------------------------------------------------------------------ loss row
def ref_loss_row(out2, loss_vec, alpha, g0, g1, K, enc_terms, eta1, eta2):
    """(row [7 + K] as regae_loss_row_kernel defines it with row[0] left NaN, row[0] at 50 digits, sum of |terms| of row[0])."""
    ae = out2[0] / out2[1] if alpha != 0.0 else 0.0
    npl, pen = (loss_vec[1], loss_vec[2]) if loss_vec is not None else (0.0, 0.0)
    en = enc_terms[0] if enc_terms is not None and eta1 != 0.0 else 0.0
    eo = enc_terms[1] if enc_terms is not None and eta2 != 0.0 else 0.0
    row = [float("nan"), ae, npl, pen] + [loss_vec[3 + i] if loss_vec is not None else 0.0 for i in range(K)] + [0.0, en, eo]
    with mpmath.workdps(50):
        aeh = mpmath.mpf(float(out2[0])) / mpmath.mpf(float(out2[1])) if alpha != 0.0 else mpmath.mpf(0)
        parts = [mpmath.mpf(alpha) * aeh, mpmath.mpf(g0) * mpmath.mpf(float(npl)), mpmath.mpf(g1) * mpmath.mpf(float(pen)),
                 mpmath.mpf(eta1) * mpmath.mpf(float(en)), mpmath.mpf(eta2) * mpmath.mpf(float(eo))]
        return np.array(row, dtype=np.float64), float(sum(parts)), float(sum(abs(p) for p in parts))
