"""GPU (-m gpu): the fp64 code every eigenfunction route ends in, at the C ABI with inputs the test controls, against references
that do not share its arithmetic (tests/stats_tail_cases.py: cases, builders, references, bars).

  cvf_ef_stats              all 16 ef_stats_partial_kernel<K, LAG> instances + the row reduction + the tail
  cvf_ef_stats_finish_rows  rows [row][ns], every pass shape of ef_stats_finish_kernel at the row-count edges
  cvf_ef16_finish           rows [ns][row], the same, up to the cap of 16384 rows
  cvf_ef_loss               ef_loss_tail_wave on 64 tail cases (k 1..8, both modes, sorted or not, two eig_w vectors) and 6 tie cases
  cvf_regae_enc_loss, cvf_regae_loss_row, and what each of these entry points refuses

Sums.  |got - ref| <= (B + 3) 2^-53 sum_b |t_b| per statistic against exact summation of the fp64 terms (rows: n_rows 2^-53
sum |rows|); bit-equal on a repeat and when the padded lanes of the last tile hold other garbage.  Derived, not measured.

Tail.  Per output group ([loss, npl, pen], eig_sorted, gS1, gS2, gE_or_gT, gS1', gS2'_ii) the bar is 8 e_ref + 16 2^-53 s, where
e_ref is the error of the fp64 oracle (oracle/stats.py + autograd) against 50-digit arithmetic with central differences and s
the group's largest magnitude; cvec must be exact.  Where the tail runs behind a reduction, the reference is the oracle on the
sums the launch wrote to `stats` (the very doubles the tail read), and the bar comes from the exact sums of the case.  The tail
is not run at B = 1 (one frame has no variance: the loss is 0 / 0).

e_ref / s over the 70 tail cases, measured on the CPU:
    loss 6e-18 .. 5e-16   eig 2e-17 .. 3e-16   gS1 2e-17 .. 1.6e-15   gS2 5e-17 .. 8e-16   gE_or_gT 5e-18 .. 5e-16
    gS1' 4e-17 .. 5e-16   gS2'_ii 6e-17 .. 5e-16        (the floor 16 2^-53 = 1.8e-15 is the larger part of most bars)

Achieved on an MI355X, worst |got - ref| / bar over all cases (1.0 = at the bar):
                              sums    loss   eig    gS1    gS2    gE_or_gT  gS1'   gS2'_ii
    cvf_ef_stats              0.03    0.26   0.23   0.34   0.27   0.21      0.27   0.31
    cvf_ef_stats_finish_rows  0.02    0.30   0.21   0.40   0.28   0.27      0.42   0.34
    cvf_ef16_finish           0.49    0.30   0.18   0.40   0.34   0.27      0.35   0.34
    cvf_ef_loss               -       0.18   0.18   0.27   0.21   0.45      0.52   0.51
    cvf_regae_enc_loss        terms 0.09, gS1 0.07, gS2 0.09
(each test prints its own figures: run with -s)

What the file catches, each built once as a memory-safe change of the kernels and run against this file: the tie-break without
`t < ic` (62 tests red, the six tie cases among them); `c` for `nsrc` in transfer mode (every transfer test with k >= 2 and a
non-identity order); the off-diagonal gS2 without its factor 2 (every test with k >= 2); `<=` in the row loop's guard (all 48
reduction tests); the pair loop of `pen` from b = a (all 70 tail tests); and cvf_ef_stats refusing "loss_vec without coef" only
after its first launch, as it did before this file (test_refusals_launch_nothing).
"""
import numpy as np
import pytest
import torch

from tests import stats_tail_cases as S

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from colvarsfinder import _hip
    _hip.lib()
    return _hip


def cfg_struct(hip, cfg):
    c = hip.EFCfg()
    c.k, c.lag_idx, c.sort_eigvals, c.iso_metric = cfg["k"], cfg["lag_idx"], cfg["sort_eigvals"], 0
    c.alpha, c.beta, c.dt = cfg["alpha"], cfg["beta"], cfg["dt"]
    for i, v in enumerate(cfg["eig_w"]):
        c.eig_w[i] = v
    return c


def d64(a, dev):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev).contiguous()


def d32(a, dev):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev).contiguous()


def nans(n, dev):
    return torch.full((n,), NAN, device=dev, dtype=torch.float64)


def tail_buffers(dev):
    """loss_vec and coef at the k = 8 length, NaN everywhere: what a launch leaves NaN it did not write."""
    return nans(S.loss_len(S.MAX_NETS), dev), nans(S.coef_len(S.MAX_NETS), dev)


def same_bits(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def check_tail(lv, cf, cfg, ref, bars, where):
    """The launch's loss_vec / coef against the oracle's groups; entries past CVF_LOSS_LEN(k) / CVF_COEF_LEN(k) still NaN."""
    k = cfg["k"]
    lv, cf = lv.cpu().numpy(), cf.cpu().numpy()
    assert np.isnan(lv[S.loss_len(k):]).all(), f"{where}: loss_vec written past CVF_LOSS_LEN({k})"
    assert np.isnan(cf[S.coef_len(k):]).all(), f"{where}: coef written past CVF_COEF_LEN({k})"
    got = S.split_outputs(lv, cf, k)
    worst = {}
    for g in S.GROUPS:
        bar = bars[g][0]
        err = float(np.max(np.abs(got[g] - ref[g]))) if np.isfinite(got[g]).all() else float("inf")
        worst[g] = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
        print(f"{where} {g}: err {err:.3e} bar {bar:.3e} (e_ref {bars[g][1]:.1e}, s {bars[g][2]:.1e})")
    assert got["cvec"].tolist() == [float(c) for c in ref["cvec"]], f"{where}: cvec {got['cvec']} != {ref['cvec']}"
    for g in S.GROUPS:
        assert worst[g] <= 1.0, f"{where}: {g} is {worst[g]:.2f} x its bar {bars[g][0]:.3e}: got {got[g]}, want {ref[g]}"


def check_sums(stats, ref, bar, where):
    got = stats.cpu().numpy()
    share = np.abs(got - ref) / bar
    print(f"{where}: worst share of the sums' bound {share.max():.3f}")
    assert np.isfinite(got).all() and share.max() <= 1.0, f"{where}: statistic {int(share.argmax())}: got {got[share.argmax()]!r}, " \
                                                         f"want {ref[share.argmax()]!r}, bound {bar[share.argmax()]:.3e}"


# ------------------------------------------------------------------------------------------------ cvf_ef_stats
def stats_args(smp, B, k, mode, garbage, dev):
    w = d32(smp["w"][:B], dev)
    y = d32(S.tiled(smp["y"], B, garbage), dev)
    if mode == "gen":
        return [w, y, d32(S.tiled(smp["e"], B, garbage), dev), None, None]
    return [w, y, None, d32(smp["w_lag"][:B], dev), d32(S.tiled(smp["y_lag"], B, garbage), dev)]


@pytest.mark.parametrize("k,mode", S.KM)
def test_ef_stats_sums_and_tail(dev, hip, k, mode):
    lib, P = hip.lib(), hip.ptr
    cfg = S.make_cfg(k, mode, 1, k % 2)
    cs, ns = cfg_struct(hip, cfg), S.nstats(k, cfg["lag_idx"])
    batches = S.stats_batches(k, mode)
    smp = S.sample(k, mode, max(batches), 1, None, True)
    assert lib.cvf_ef_stats_scratch_doubles(k, cfg["lag_idx"]) == S.STAT_BLOCKS * ns and lib.cvf_ef_nstats(k, cfg["lag_idx"]) == ns

    def run(B, garbage, tail):
        args = stats_args(smp, B, k, mode, garbage, dev)
        scratch, stats = nans(S.STAT_BLOCKS * ns, dev), nans(ns + 3, dev)   # (rows past the grid are never read: NaN would show)
        lv, cf = tail_buffers(dev)
        hip.check(lib.cvf_ef_stats(cs, B, *[P(a) for a in args], P(scratch), P(stats), P(lv) if tail else None, P(cf), hip.stream()),
                  "cvf_ef_stats")
        torch.cuda.synchronize()
        assert torch.isnan(stats[ns:]).all()
        return stats[:ns], lv, cf

    for B in batches:
        where = f"ef_stats-{mode}-k{k} B={B}"
        tail = B >= 63
        stats, lv, cf = run(B, 1, tail)
        ref, abs_sums = S.ref_sums(smp, B, k, mode)
        check_sums(stats, ref, S.sums_bar(B, abs_sums), where)
        again = run(B, 1, tail)
        assert all(same_bits(a, b) for a, b in zip((stats, lv, cf), again)), f"{where}: a repeat run differs"
        other = run(B, 2, False)
        assert same_bits(stats, other[0]), f"{where}: the padded lanes' content reached the sums"
        assert torch.isnan(other[1]).all() and torch.isnan(other[2]).all(), f"{where}: loss_vec == NULL, yet the tail ran"
        if tail:
            check_tail(lv, cf, cfg, S.ref_tail(stats.cpu().numpy(), cfg), S.tail_bars(ref, cfg), where)


# ------------------------------------------------------------------------------------------------ the row reductions
def finish_case(dev, hip, k, mode, call, counts):
    """counts: [(n_rows, first argument of the call)]; call(cfg, arg, partial, stats, loss_vec, coef) -> rc."""
    cfg = S.make_cfg(k, mode, 1, 0)
    cs, ns = cfg_struct(hip, cfg), S.nstats(k, cfg["lag_idx"])
    bars = S.tail_bars(S.tail_sums(k, mode).numpy(), cfg)
    for n, arg, name, stat_major in counts:
        where = f"{name}-{mode}-k{k} rows={n}"
        rows = S.synth_rows(k, mode, n)
        part = d64(rows.T if stat_major else rows, dev).reshape(-1)
        ref, abs_sums = S.ref_rowsum(rows)
        stats, (lv, cf) = nans(ns + 3, dev), tail_buffers(dev)
        hip.check(call(cs, arg, part, stats, None, cf), name)
        torch.cuda.synchronize()
        assert torch.isnan(stats[ns:]).all()
        check_sums(stats[:ns], ref, S.rows_bar(n, abs_sums), where)
        assert torch.isnan(lv).all() and torch.isnan(cf).all(), f"{where}: loss_vec == NULL, yet coef was written"
        stats2 = nans(ns + 3, dev)
        hip.check(call(cs, arg, part, stats2, lv, cf), name)
        torch.cuda.synchronize()
        assert same_bits(stats, stats2), f"{where}: the sums differ when the tail follows"
        check_tail(lv, cf, cfg, S.ref_tail(stats2[:ns].cpu().numpy(), cfg), bars, where)


@pytest.mark.parametrize("k,mode", S.KM)
def test_finish_rows_row_major(dev, hip, k, mode):
    lib, P = hip.lib(), hip.ptr
    finish_case(dev, hip, k, mode, lambda cs, n, part, st, lv, cf: lib.cvf_ef_stats_finish_rows(cs, n, P(part), P(st), P(lv), P(cf), hip.stream()),
                [(n, n, "cvf_ef_stats_finish_rows", False) for n in S.row_counts(k, mode)])


@pytest.mark.parametrize("k,mode", S.KM)
def test_ef16_finish_statistic_major(dev, hip, k, mode):
    lib, P = hip.lib(), hip.ptr
    counts = []
    for B in S.ef16_batches(k, mode):
        assert lib.cvf_ef16_rows(B) == S.ef16_rows(B) > 0
        counts.append((S.ef16_rows(B), B, "cvf_ef16_finish", True))
    finish_case(dev, hip, k, mode, lambda cs, B, part, st, lv, cf: lib.cvf_ef16_finish(cs, B, P(part), P(st), P(lv), P(cf), hip.stream()), counts)


# ------------------------------------------------------------------------------------------------ cvf_ef_loss
def run_ef_loss(dev, hip, case):
    lib, P = hip.lib(), hip.ptr
    cfg, sums = S.cfg_of(case), S.case_sums(case).numpy()
    lv, cf = tail_buffers(dev)
    st = d64(sums, dev)
    hip.check(lib.cvf_ef_loss(cfg_struct(hip, cfg), P(st), P(lv), P(cf), hip.stream()), "cvf_ef_loss")
    torch.cuda.synchronize()
    check_tail(lv, cf, cfg, S.ref_tail(sums, cfg), S.tail_bars(sums, cfg), "ef_loss-" + case.id)


@pytest.mark.parametrize("k,mode", S.KM)
def test_ef_loss_tail_cases(dev, hip, k, mode):
    cases = [c for c in S.TAIL_CASES if (c.k, c.mode) == (k, mode)]
    assert len(cases) == 4
    for case in cases:
        run_ef_loss(dev, hip, case)


@pytest.mark.parametrize("case", S.TIE_CASES, ids=lambda c: c.id)
def test_ef_loss_tied_eigenvalues_keep_numpys_stable_order(dev, hip, case):
    run_ef_loss(dev, hip, case)


# ------------------------------------------------------------------------------------------------ RegAutoEncoderTask's scalars
@pytest.mark.parametrize("k", range(1, S.MAX_NETS + 1))
def test_regae_enc_loss(dev, hip, k):
    lib, P = hip.lib(), hip.ptr
    sums = S.tail_sums(k, "gen").numpy()
    st = d64(sums, dev)
    for eta1, eta2 in S.ENC_ETAS:
        where = f"regae_enc-k{k} eta=({eta1},{eta2})"
        terms, coef = nans(4, dev), nans(S.MAX_NETS + S.MAX_NETS ** 2, dev)
        hip.check(lib.cvf_regae_enc_loss(P(st), k, eta1, eta2, P(terms), P(coef), hip.stream()), "cvf_regae_enc_loss")
        torch.cuda.synchronize()
        terms, coef = terms.cpu().numpy(), coef.cpu().numpy()
        assert np.isnan(terms[2:]).all() and np.isnan(coef[k + k * k:]).all(), f"{where}: written past the end"
        got = {"terms": terms[:2], "gS1": coef[:k], "gS2": coef[k:k + k * k]}
        ref, bars = S.ref_enc(sums, k, eta1, eta2), S.enc_bars(sums, k, eta1, eta2)
        for g in S.ENC_GROUPS:
            err, bar = float(np.max(np.abs(got[g] - ref[g]))), bars[g][0]
            print(f"{where} {g}: err {err:.3e} bar {bar:.3e}")
            assert np.isfinite(got[g]).all() and err <= bar, f"{where}: {g} err {err:.3e} > bar {bar:.3e}: got {got[g]}, want {ref[g]}"


def test_regae_loss_row(dev, hip):
    lib, P = hip.lib(), hip.ptr
    rs = np.random.RandomState(3)
    out2 = np.array([3.7251, 811.3, NAN])
    variants = [dict(), dict(loss_vec=False), dict(enc=False), dict(alpha=0.0), dict(eta1=0.0), dict(eta2=0.0),
                dict(loss_vec=False, enc=False), dict(alpha=0.0, eta1=0.0, eta2=0.0)]
    for K in (1, 3, 8):
        loss_vec = rs.uniform(0.1, 9.0, S.loss_len(K)) * rs.choice([-1.0, 1.0], S.loss_len(K))
        enc = rs.uniform(0.1, 3.0, 2)
        for v in variants:
            alpha, eta1, eta2 = v.get("alpha", 0.8), v.get("eta1", 1.5), v.get("eta2", 0.7)
            lvh = loss_vec if v.get("loss_vec", True) else None
            ench = enc if v.get("enc", True) else None
            row = nans(7 + S.MAX_NETS + 2, dev)
            o2d, lvd, encd = d64(out2, dev), d64(lvh, dev) if lvh is not None else None, d64(ench, dev) if ench is not None else None
            hip.check(lib.cvf_regae_loss_row(P(o2d), P(lvd), alpha, 1.3, -0.45, K, P(encd), eta1, eta2, P(row), hip.stream()),
                      "cvf_regae_loss_row")
            torch.cuda.synchronize()
            row = row.cpu().numpy()
            want, row0, abs_terms = S.ref_loss_row(out2, lvh, alpha, 1.3, -0.45, K, ench, eta1, eta2)
            assert np.isnan(row[7 + K:]).all(), (K, v)
            assert abs(row[1] - want[1]) <= np.spacing(abs(want[1])), (K, v, row[1], want[1])     # one division
            assert row[2:7 + K].tobytes() == want[2:].tobytes(), (K, v, row[2:7 + K], want[2:])   # copies: bit for bit
            assert abs(row[0] - row0) <= 4 * np.spacing(abs_terms), (K, v, row[0], row0)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(dev, hip):
    lib, P, st = hip.lib(), hip.ptr, hip.stream()
    k = 2
    smp = S.sample(k, "gen", 65, 1, None, True)
    w, y, e = d32(smp["w"], dev), d32(S.tiled(smp["y"], 65), dev), d32(S.tiled(smp["e"], 65), dev)
    sums = d64(S.tail_sums(k, "gen").numpy(), dev)
    scratch, stats, terms = nans(S.STAT_BLOCKS * S.nstats(8, 1), dev), nans(S.nstats(8, 1), dev), nans(2, dev)
    lv, cf = tail_buffers(dev)
    rows = d64(S.synth_rows(k, "gen", 4), dev).reshape(-1)
    gen, tr = S.make_cfg(k, "gen"), S.make_cfg(k, "tr")
    cg, ct = cfg_struct(hip, gen), cfg_struct(hip, tr)

    def refused(call, *message):
        """cvf_last_error keeps its text between calls: first another refusal (cvf_regae_loss_row without `row`) replaces it, so
        what is matched afterwards - the entry point's name and the piece of ITS message - was written by this call."""
        assert lib.cvf_regae_loss_row(P(sums), None, 1.0, 1.0, 1.0, 1, None, 0.0, 0.0, None, st) != 0
        assert lib.cvf_last_error().decode() == "cvf_regae_loss_row: bad argument"
        rc = call()
        text = lib.cvf_last_error().decode()
        assert rc != 0 and all(m in text for m in message), (rc, text, message)
        torch.cuda.synchronize()
        for name, t in (("scratch", scratch), ("stats", stats), ("loss_vec", lv), ("coef", cf), ("terms", terms)):
            assert torch.isnan(t).all(), f"{message}: refused, yet {name} was written"

    def ef_stats(cs, B, e_, wl, yl, lv_, cf_):
        return lambda: lib.cvf_ef_stats(cs, B, P(w), P(y), P(e_), P(wl), P(yl), P(scratch), P(stats), P(lv_), P(cf_), st)

    for bad in (0, S.MAX_NETS + 1):
        cs = cfg_struct(hip, dict(gen, k=bad))
        refused(lambda: lib.cvf_ef_loss(cs, P(sums), P(lv), P(cf), st), "cvf_ef_loss", f"k={bad} out of range")
        refused(ef_stats(cs, 65, e, None, None, lv, cf), "cvf_ef_stats", f"k={bad} out of range")
        refused(lambda: lib.cvf_regae_enc_loss(P(sums), bad, 1.5, 0.7, P(terms), P(cf), st), "cvf_regae_enc_loss", f"(k={bad})")
    refused(ef_stats(cg, 0, e, None, None, lv, cf), "cvf_ef_stats: bad argument")
    refused(ef_stats(cg, 65, None, None, None, lv, cf), "cvf_ef_stats", "generator mode needs e_tiled")
    refused(ef_stats(ct, 65, None, w, None, lv, cf), "cvf_ef_stats", "transfer mode needs lagged inputs")
    refused(ef_stats(ct, 65, None, None, y, lv, cf), "cvf_ef_stats", "transfer mode needs lagged inputs")
    refused(ef_stats(cg, 65, e, None, None, lv, None), "cvf_ef_stats", "loss_vec without coef")
    refused(lambda: lib.cvf_ef_loss(cg, P(sums), P(lv), None, st), "cvf_ef_loss: bad argument")
    refused(lambda: lib.cvf_ef_stats_finish_rows(cg, 4, P(rows), P(stats), P(lv), None, st), "cvf_ef_stats_finish_rows", "loss_vec without coef")
    refused(lambda: lib.cvf_ef_stats_finish_rows(cg, 0, P(rows), P(stats), P(lv), P(cf), st), "cvf_ef_stats_finish_rows: bad argument")
    refused(lambda: lib.cvf_ef16_finish(cg, 64, P(rows), P(stats), P(lv), None, st), "cvf_ef16_finish", "loss_vec without coef")
    B = 64 * S.MAX_ROWS16 // 4 + 1
    assert lib.cvf_ef16_rows(B) == 0 == S.ef16_rows(B)
    refused(lambda: lib.cvf_ef16_finish(cg, B, P(rows), P(stats), P(lv), P(cf), st), "cvf_ef16_finish: bad argument")
    refused(lambda: lib.cvf_ef16_finish(cg, 0, P(rows), P(stats), P(lv), P(cf), st), "cvf_ef16_finish: bad argument")
