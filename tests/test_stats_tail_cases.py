"""CPU: the case table of tests/stats_tail_cases.py covers what tests/test_stats_tail_gpu.py is meant to cover - every compiled
ef_stats_partial_kernel<K, LAG> instance, every pass shape of the row reduction in both row layouts at the row counts where a
lane sweep or a trip of the row loop ends, the conditions that make the tail cases decisive (ordering not the identity, gaps,
bit-equal ties) - and the map from autograd's gradient to the `coef` layout agrees with 50-digit central differences."""
import os

import numpy as np
import pytest

from tests import stats_tail_cases as S
from tests.codeobj import built_objects, kernels_of, template_args


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    built = built_objects()
    names = kernels_of(os.path.join(built, "stats.o"), tmp_path_factory.mktemp("stats_o"))
    keys = {template_args(name, "ef_stats_partial_kernel") for name in names} - {None}
    return {("ef_stats_partial_kernel",) + key for key in keys}


def test_every_compiled_partial_sum_instance_is_claimed(compiled):
    assert len(compiled) == 16, sorted(compiled)
    assert compiled - S.claimed() == set(), "instances no case launches: " + str(sorted(compiled - S.claimed()))
    assert S.claimed() - compiled == set(), "instances the table claims but stats.o does not hold: " + str(sorted(S.claimed() - compiled))


def test_each_instance_sees_the_batch_edges():
    seen = set()
    for k, mode in S.KM:
        b = S.stats_batches(k, mode)
        assert set(S.SMALL_B) <= set(b) and max(b) > 8192, (k, mode, b)
        seen |= set(b)
    assert set(S.BIG_B) <= seen
    for mode in S.MODES:     # every big batch meets at least one instance of each LAG
        assert set(S.BIG_B) <= {B for k in range(1, S.MAX_NETS + 1) for B in S.stats_batches(k, mode)}, mode
    assert [S.stat_grid(B) for B in (1, 64, 65) + S.BIG_B] == [1, 1, 2, 128, 128, 128, 128]
    assert 64 * S.STAT_BLOCKS < S.BIG_B[2] <= 64 * (S.STAT_BLOCKS + 1)    # block 0 alone walks a second tile


def test_mirrored_rules():
    assert [S.nstats(k, 0) for k in (1, 3, 8)] == [4, 13, 53] and [S.nstats(k, 2) for k in (1, 3, 8)] == [7, 20, 70]
    assert S.finish_pass(4) == (1, 24) and S.finish_pass(16) == (1, 24) and S.finish_pass(17) == (2, 20)
    assert S.finish_pass(32) == (2, 20) and S.finish_pass(33) == (4, 6)
    assert S.ef16_rows(1) == 4 and S.ef16_rows(20000) == 1252 and S.ef16_rows(262144) == 16384 and S.ef16_rows(262145) == 0
    assert S.coef_len(8) == 96 and S.loss_len(8) == 19


def test_pair_index_formula_agrees_with_the_enumerated_layout():
    """pidx (the fp64 side's index formula) against stat_names (the 50-digit side's walk of the layout in include/cvf.h)."""
    for k in range(1, S.MAX_NETS + 1):
        for lag in (0, 2):
            at = S.stat_names(k, lag)
            assert len(at) == S.nstats(k, lag) and sorted(at.values()) == list(range(S.nstats(k, lag)))
            for i in range(k):
                for j in range(k):
                    assert 1 + k + S.pidx(k, i, j) == at["S2", min(i, j), max(i, j)]


@pytest.mark.parametrize("k,mode", S.KM)
def test_stats_batches_have_separated_eigenvalues(k, mode):
    """The tail behind cvf_ef_stats is compared in exact cvec: at every batch where it runs, the fp32 sample's sorted
    eigenvalues keep a relative gap of at least 1e-3 (the kernel's and the oracle's differ by a few 2^-53)."""
    cfg = S.make_cfg(k, mode, 1, k % 2)
    batches = S.stats_batches(k, mode)
    smp = S.sample(k, mode, max(batches), 1, None, True)
    for B in batches:
        if B < 63:
            continue
        e = S.ref_tail(S.ref_sums(smp, B, k, mode)[0], cfg)["eig"]
        assert np.all(e > 0) and (k == 1 or np.min(np.diff(e) / np.abs(e[1:])) >= 1e-3), (B, e)


def test_every_pass_shape_is_hit_at_the_row_edges_in_both_layouts():
    hit = {}
    for k, mode in S.KM:
        shape = S.finish_pass(S.nstats(k, S.lag_of(k, mode)))
        R = 64 * shape[1]
        rows = S.row_counts(k, mode)
        assert set(rows) == {1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 5}
        rows16 = [S.ef16_rows(B) for B in S.ef16_batches(k, mode)]
        assert all(r > 0 and r % 4 == 0 for r in rows16)
        for n in rows:       # the multiples of 4 on either side of every row-major count
            assert {max(4, 4 * (n // 4)), 4 * ((n + 3) // 4)} <= set(rows16), (k, mode, n)
        assert {S.ef16_rows(20000), S.MAX_ROWS16} <= set(rows16)
        hit.setdefault(shape, set()).update(rows)
    assert set(hit) == {(1, 24), (2, 20), (4, 6)}
    for (kst, kr), rows in hit.items():
        R = 64 * kr
        assert {1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 5} <= rows


def test_synthetic_rows_cannot_lose_a_row_unseen():
    """Every entry's magnitude is above the bar of its column, and the rows add up to a consistent sums vector."""
    for k, mode in ((1, "gen"), (3, "tr"), (8, "tr")):
        for n in (S.row_counts(k, mode)[-1], S.MAX_ROWS16):
            rows = S.synth_rows(k, mode, n)
            total, abs_sums = S.ref_rowsum(rows)
            bar = S.rows_bar(n, abs_sums)
            assert np.all(np.abs(rows).min(axis=0) > bar), (k, mode, n)
            assert np.abs(rows[:-1]).min() >= 1e-3 and np.abs(rows[:-1]).max() <= 1e3
            assert (rows > 0).any() and (rows < 0).any()
            np.testing.assert_allclose(total, S.tail_sums(k, mode).numpy(), rtol=0, atol=2 * S.EPS * np.abs(rows).max())


@pytest.mark.parametrize("k,mode", S.KM)
def test_inputs_are_as_described(k, mode):
    s = S.sample(k, mode, 4096, 1, None, True)
    assert s["w"].min() >= 0.5 and s["w"].max() <= 1.5
    for a in s.values():
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    var = s["y"].var(axis=0)
    assert var.min() > 0.3 and var.max() < 2.5 and np.abs(var - 1).min() > 0.05
    assert np.abs(s["y"].mean(axis=0)).min() > 0.3
    if k > 1:
        cov = np.cov(s["y"].T)
        assert np.abs(cov[np.triu_indices(k, 1)]).min() > 0.02
    if mode == "gen":
        assert s["e"].min() >= 0
    t = S.tiled(s["y"], 65, garbage=3).reshape(2, k, 64)
    assert np.array_equal(t[1, :, 0], s["y"][64].astype(np.float32)) and np.abs(t[1, :, 1:]).min() >= 500
    assert np.array_equal(S.tiled(s["y"], 65).reshape(2, k, 64)[0], s["y"][:64].T.astype(np.float32))


@pytest.mark.parametrize("case", S.TAIL_CASES, ids=lambda c: c.id)
def test_tail_case_conditions(case):
    cfg = S.cfg_of(case)
    assert cfg["alpha"] != 1 and cfg["beta"] != 1 and cfg["dt"] != 1
    ref = S.ref_tail(S.case_sums(case), dict(cfg, sort_eigvals=1))
    if case.k >= 2:
        assert list(ref["cvec"]) != list(range(case.k))
        e = ref["eig"]
        assert np.min(np.diff(e) / np.abs(e[1:])) >= 1e-3
    assert np.all(ref["eig"] > 0)


def test_tail_cases_cover_the_settings():
    assert {(c.k, c.mode, c.sort, c.wsel) for c in S.TAIL_CASES} == {(k, m, s, w) for k, m in S.KM for s in (0, 1) for w in (0, 1)}
    assert {S.cfg_of(c)["lag_idx"] for c in S.TAIL_CASES if c.mode == "tr"} == {1, 3}
    assert all(S.cfg_of(c)["lag_idx"] == 0 for c in S.TAIL_CASES if c.mode == "gen")
    for k in range(2, S.MAX_NETS + 1):
        w0, w1 = S.EIG_W[0][:k], S.EIG_W[1][:k]
        assert all(a > b for a, b in zip(w0, w0[1:]))
        assert any(a < b for a, b in zip(w1, w1[1:])) and (k < 3 or any(a > b for a, b in zip(w1, w1[1:])))
    assert {(c.k, c.mode) for c in S.TIE_CASES} == {(k, m) for k in (2, 4, 8) for m in S.MODES}


@pytest.mark.parametrize("case", S.TIE_CASES, ids=lambda c: c.id)
def test_tied_eigenvalues_are_bit_equal_in_the_oracle(case):
    a, b = case.tie
    unsorted = S.ref_tail(S.case_sums(case), dict(S.cfg_of(case), sort_eigvals=0))["eig"]
    assert unsorted[a].tobytes() == unsorted[b].tobytes()
    ref = S.ref_tail(S.case_sums(case), S.cfg_of(case))
    cvec = list(ref["cvec"])
    assert cvec == list(np.argsort(unsorted, kind="stable")) and cvec.index(b) == cvec.index(a) + 1


@pytest.mark.parametrize("case", S.TAIL_CASES + S.TIE_CASES, ids=lambda c: c.id)
def test_coef_map_agrees_with_central_differences_and_bars_are_usable(case):
    """autograd -> coef (ref_tail: coef_groups_from_grad, pidx) against hp_tail, which fills every `coef` entry by a central
    difference in the one sum include/cvf.h names for it, found by walking the layout (stat_names) - the two share no index
    code.  They must agree within the fp64 oracle's own error: a few units of 2^-53 of the group's largest entry times the
    conditioning of the tail (means ~1 against variances ~1: below 100).  A wrong offset, a transposed or one-sided gS2 or a
    missing factor in the map is an error of order 1 (test_a_wrong_map_is_seen).  And every bar is finite and, except the two
    groups that are identically zero in generator mode, positive."""
    sums, cfg = S.case_sums(case), S.cfg_of(case)
    ref, hp = S.ref_tail(sums, cfg), S.hp_tail(sums, cfg)
    assert list(ref["cvec"]) == list(hp["cvec"])
    for g, (bar, e_ref, s) in S.tail_bars(sums, cfg).items():
        assert np.isfinite(bar) and np.isfinite(e_ref) and np.isfinite(s)
        if cfg["lag_idx"] == 0 and g in ("gS1l", "gS2l"):
            assert bar == 0 and np.all(ref[g] == 0)
            continue
        assert s > 0 and bar > 0, (g, bar, e_ref, s)
        assert e_ref <= 100 * S.EPS * s, (g, e_ref, s)
    assert len(S.coef_vector(ref)) == S.coef_len(case.k)


def test_a_wrong_map_is_seen():
    """The criterion above, applied to maps that are wrong in the ways a map goes wrong: each is far outside 100 2^-53 s."""
    case = next(c for c in S.TAIL_CASES if (c.k, c.mode, c.sort, c.wsel) == (3, "tr", 1, 1))
    sums, cfg = S.case_sums(case), S.cfg_of(case)
    ref, hp = S.ref_tail(sums, cfg), S.hp_tail(sums, cfg)
    k = case.k
    wrong = {"offsets of gS1' and gS2'_ii swapped": dict(ref, gS1l=ref["gS2l"], gS2l=ref["gS1l"]),
             "gT read at the S2' block": dict(ref, gET=ref["gS2l"]),
             "gS2 halved off the diagonal": dict(ref, gS2=(ref["gS2"].reshape(k, k) * (0.5 + 0.5 * np.eye(k))).reshape(-1)),
             "gS2 one-sided": dict(ref, gS2=np.triu(ref["gS2"].reshape(k, k)).reshape(-1)),
             "gS2 rows rotated": dict(ref, gS2=np.roll(ref["gS2"].reshape(k, k), 1, axis=0).reshape(-1))}
    for what, bad in wrong.items():
        worst = max(e / s for g in S.COEF_GROUPS for _, e, s in [S.bars_from(bad, hp, [g])[g]])
        assert worst > 1e-3, (what, worst)
    assert max(e / s for _, e, s in S.bars_from(ref, hp, S.COEF_GROUPS).values()) <= 100 * S.EPS


@pytest.mark.parametrize("k", range(1, S.MAX_NETS + 1))
def test_encoder_reference_agrees_with_central_differences(k):
    sums = S.tail_sums(k, "gen").numpy()
    for eta1, eta2 in S.ENC_ETAS:
        for g, (bar, e_ref, s) in S.enc_bars(sums, k, eta1, eta2).items():
            assert np.isfinite(bar) and e_ref <= 100 * S.EPS * s, (k, eta1, eta2, g, e_ref, s)
