"""CPU (-m "not gpu"): the case table of the per-layer eigenfunction route (tests/ef_general_cases.py) against the library's
host-side answers (csrc/ef_general.hip) - the mirrors of its slab-row rule, of the `saved` layout and of its refusals; the
edges the table claims, asserted as properties of its shapes; the refusals and their reasons; and where the bars of the GPU
module (tests/test_ef_general_edges_gpu.py) come from."""
import pytest

from tests import ef_general_cases as G


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    from colvarsfinder import _hip
    _hip.lib()
    return _hip


def _desc(case):
    """The description a case runs on: core._SharedTrunkFlat's (the plain layout for n_shared None)."""
    import torch
    from colvarsfinder import core
    return core._SharedTrunkFlat(list(case.dims), G.act_codes(case), case.k, case.ns or 0, torch.device("cpu")).desc


def _plain(hip, dims, k, acts):
    """k nets net by net over a flat buffer, without allocating it (the 4096-wide shapes of the refusals)."""
    m, L, pos = hip.MLPDesc(), len(dims) - 1, 0
    m.n_nets, m.n_layers = k, L
    for l in range(L):
        m.dims[l], m.dims[l + 1], m.act[l] = dims[l], dims[l + 1], acts[l]
    for i in range(k):
        for l in range(L):
            m.w_off[i][l], pos = pos, pos + dims[l] * dims[l + 1]
            m.b_off[i][l], pos = pos, pos + dims[l + 1]
    m.n_params = pos
    return m


def _supported(lib, desc, ns):
    return lib.cvf_ef_general_supported(desc) if ns is None else lib.cvf_ef_general_shared_supported(desc, ns)


def _rows(lib, desc, ns, tiles):
    return lib.cvf_ef_general_slab_rows(desc, tiles) if ns is None else lib.cvf_ef_general_shared_slab_rows(desc, tiles, ns)


def test_mirrors_equal_the_library(hip):
    lib = hip.lib()
    for c in G.CASES:
        d, T = _desc(c), G.n_tiles(c.B)
        n = G.n_params(c.dims, c.k, c.ns)
        assert d.n_params == n, c.id
        assert _supported(lib, d, c.ns) == 1, (c.id, lib.cvf_last_error())
        assert G.efg_why(c.dims, c.k, G.act_codes(c), None if c.ns else n) is None
        for tiles in (T, 2 * T):
            assert _rows(lib, d, c.ns, tiles) == G.g64_rows(n, tiles), (c.id, tiles)
            if c.ns is None:
                for lag in (0, G.LAG):
                    assert lib.cvf_ef_general_saved_floats(d, tiles, lag) == G.efg_layout(c.dims, c.k, tiles, lag == 0).total, (c.id, tiles)
            else:
                assert lib.cvf_ef_general_shared_saved_floats(d, tiles, c.ns) == G.efg_layout(c.dims, c.k, tiles, True, c.ns).total
                assert G.efg_layout(c.dims, c.k, tiles, True, c.ns).total < G.efg_layout(c.dims, c.k, tiles, True).total
        assert lib.cvf_ef_general_saved_floats(d, 0, 0) == 0


def test_the_slab_row_rule_has_three_branches(hip):
    lib = hip.lib()
    cap, wide = G.BY_ID["slab-capped-gen"], G.BY_ID["one-row-4096-gen"]
    assert G.n_params(cap.dims, cap.k) == 131_242 and G.n_tiles(cap.B) == 257
    assert 4 * 255 * 131_242 <= G.SLAB_BYTES < 4 * 256 * 131_242
    assert lib.cvf_ef_general_slab_rows(_desc(cap), 257) == 255 == G.g64_rows(131_242, 257)
    assert G.n_params(wide.dims, wide.k) == 16_822_273 and 4 * 16_822_273 < G.SLAB_BYTES < 8 * 16_822_273
    assert lib.cvf_ef_general_slab_rows(_desc(wide), G.n_tiles(wide.B)) == 1 == G.g64_rows(16_822_273, 3) and G.n_tiles(wide.B) == 3
    assert max(wide.dims) == G.MAX_WIDTH
    many = G.BY_ID["many-tiles-gen"]
    assert lib.cvf_ef_general_slab_rows(_desc(many), 257) == 256 and lib.cvf_ef_general_slab_rows(_desc(many), 3) == 3


def test_the_table_reaches_its_edges():
    cases = G.CASES
    assert len({c.id for c in cases}) == len(cases) <= 48
    assert all(c.dims[-1] == 1 and c.mode in ("gen", "tr") and (c.ns is None or c.mode == "gen") for c in cases)
    for mode in ("gen", "tr"):
        plain = [c for c in cases if c.mode == mode and c.ns is None]
        hidden = {h for c in plain for h in c.dims[1:-1]}
        assert {1, 31, 32, 33, 63, 64, 65, 130} <= hidden, mode                    # M of a forward product, K of the next
        assert {h % G.KC for h in hidden} >= {0, 1, G.KC - 1} and {h % 64 for h in hidden} >= {0, 1, 63}
        assert {1, 3, 67, 384} <= {c.dims[0] for c in plain}
        assert {c.dims[0] % 64 for c in plain} >= {0, 1, 63}                       # d0 as M of g = W_0^T delta, as K of layer 0
        assert {2, 63, 64, 65, 130, 257} <= {c.B for c in plain}
        assert {c.act for c in plain} == set(G.ACTS)
        # sigma' in the operand load (every chain: the g product, the tangent chain) and sigma' / sigma'' in the epilogue of an
        # adjoint product (two hidden layers or more), under every activation
        assert {c.act for c in plain if len(c.dims) >= 4} == set(G.ACTS)
        assert {len(c.dims) - 2 for c in plain} >= {1, 2, 3, G.MAX_LAYERS - 1}
        assert any(c.k == G.MAX_NETS and c.dims[0] == 1 for c in plain) and any(c.k == 1 for c in plain)
        assert any(len(set(c.dims[1:-1])) >= 3 for c in plain)                     # unequal widths
        # the weight gradient [Mo][Ki + 1]: the bias column first of a block, last of a block, and one past a K stage
        ki = {c.dims[l] for c in plain for l in range(len(c.dims) - 1)}
        assert {(x + 1) % 64 for x in ki} >= {0, 1, 2} and {x % 64 for x in ki} >= {0, 63, 31, 32, 33}
        assert any((c.dims[l] + 1) % 64 == 1 and c.dims[l + 1] % 64 in (0, 63, 1) for c in plain for l in range(len(c.dims) - 2))
    # more tiles than slab rows
    many = G.BY_ID["many-tiles-gen"]
    assert G.step_tiles(many) == 257 and G.g64_rows(G.n_params(many.dims, many.k), 257) == 256
    half, T = G.BY_ID["lagged-wrap-tr"], G.n_tiles(G.HALF_B)
    assert T == 129 and G.step_tiles(half) == 258
    for rho in (0, 1):    # a base tile and a lagged one
        assert [t >= T for t in G.row_tiles(rho, 258, 256)] == [False, True]
    assert all(len(G.row_tiles(rho, 258, 256)) == 1 for rho in range(2, 256))
    full, T = G.BY_ID["many-tiles-tr"], G.n_tiles(G.MANY_B)
    assert T == 257 and G.step_tiles(full) == 514 and G.row_tiles(0, 514, 256) == [0, 256, 512]
    assert [t >= T for t in G.row_tiles(0, 514, 256)] == [False, False, True]          # base, base, lagged in ONE row
    assert any(c.mode == "tr" and any({t >= G.n_tiles(c.B) for t in G.row_tiles(r, G.step_tiles(c), G.g64_rows(
        G.n_params(c.dims, c.k), G.step_tiles(c)))} == {False, True} for r in range(2)) for c in cases)
    # the slab-row rule's other branches
    rows = {c.id: G.g64_rows(G.n_params(c.dims, c.k, c.ns), G.step_tiles(c)) for c in cases}
    assert rows["slab-capped-gen"] == 255 < 257 == G.step_tiles(G.BY_ID["slab-capped-gen"])
    assert rows["one-row-4096-gen"] == 1 < G.step_tiles(G.BY_ID["one-row-4096-gen"])
    # the shared trunk: d0 past 9, a trunk of some and of all hidden layers, a shared [W | b] of two column blocks and one
    # whose bias column is the last of its block
    shared = [c for c in cases if c.ns]
    assert {c.ns == len(c.dims) - 2 for c in shared} == {True, False} and all(c.dims[0] > 9 and c.k >= 2 for c in shared)
    assert any(c.dims[l] + 1 > 64 for c in shared for l in range(c.ns)) and any((c.dims[l] + 1) % 64 == 0 for c in shared for l in range(c.ns))
    # the once-only checks run on a small two-tile ragged chain
    for mode, c in G.RAGGED.items():
        assert c.mode == mode and G.n_tiles(c.B) == 2 and c.B % 64 != 0


def test_b_1_has_no_loss():
    """Why the one-frame batches of the table are two frames: with one frame the weighted variance is 0 in exact arithmetic."""
    import torch
    from oracle import losses
    y, w = torch.tensor([[0.3, -1.2]], dtype=torch.float64), torch.tensor([0.7], dtype=torch.float64)
    _, _, var = losses.ef_stats(y, w)
    assert all(abs(float(v)) < 1e-15 for v in var)


def test_refusals_say_why(hip):
    lib = hip.lib()
    tanh = lambda L: [1] * (L - 1) + [0]   # noqa: E731

    def refused(m, why, mirror):
        assert why and mirror == why, (mirror, why)
        assert lib.cvf_ef_general_supported(m) == 0 and why in lib.cvf_last_error().decode(), lib.cvf_last_error()
        assert lib.cvf_ef_general_slab_rows(m, 4) == 0 and lib.cvf_ef_general_saved_floats(m, 4, 0) == 0
        # the launching entries refuse the same way, before any launch (no device is touched: this runs without a GPU)
        assert lib.cvf_ef_general_fwd(m, None, None, 4, None, None, None, None) < 0 and why in lib.cvf_last_error().decode()
        cfg = hip.EFCfg()
        cfg.k = m.n_nets
        assert lib.cvf_ef_general_backward(cfg, m, None, 100, None, None, None, None, None, None, None, None, None, None) < 0
        assert why in lib.cvf_last_error().decode()

    d = [30, 20, 2]
    refused(_plain(hip, d, 2, tanh(2)), "the nets' output must be a scalar", G.efg_why(d, 2, tanh(2)))
    d = [30, 20, 20, 1]
    refused(_plain(hip, d, 2, [1, 1, 1]), "an activation after the output layer", G.efg_why(d, 2, [1, 1, 1]))
    m = _plain(hip, [6] + [9] * 11 + [1], 1, tanh(12))
    assert lib.cvf_ef_general_supported(m) == 1 and G.efg_why([6] + [9] * 11 + [1], 1, tanh(12)) is None
    m.n_layers = 13       # twelve hidden layers: past what the description can hold
    refused(m, "12 hidden layers: 1 to 11 are supported", G.efg_why([6] + [9] * 11 + [1], 1, tanh(13), n_layers=13))
    d = [30, 4097, 1]
    refused(_plain(hip, d, 1, tanh(2)), "hidden layer 1 is 4097 wide: 1 to 4096 units are supported", G.efg_why(d, 1, tanh(2)))
    assert lib.cvf_ef_general_supported(_plain(hip, [30, 4096, 1], 1, tanh(2))) == 1
    d = [30, 20, 1]
    m = _plain(hip, d, 2, tanh(2))
    m.n_params += 1       # a parameter no layer owns: its slab entries would never be written
    refused(m, "the flat buffer holds parameters outside the nets", G.efg_why(d, 2, tanh(2), n_par=m.n_params))
    # shared blocks given to the plain entry: the flat buffer of a shared trunk is shorter than k nets
    c = G.BY_ID["shared-1-of-2"]
    m = _desc(c)
    assert lib.cvf_ef_general_shared_supported(m, c.ns) == 1
    refused(m, "the flat buffer holds parameters outside the nets", G.efg_why(c.dims, c.k, G.act_codes(c), n_par=m.n_params))
    d = [30, 20, 1]
    for k in (0, 9):
        m = _plain(hip, d, 1, tanh(2))
        m.n_nets = k
        refused(m, f"{k} nets: 1 to 8 are supported", G.efg_why(d, k, tanh(2)))
    refused(_plain(hip, d, 1, [7, 0]), "an activation code outside include/cvf.h", G.efg_why(d, 1, [7, 0]))
    assert lib.cvf_ef_general_supported(None) == 0


def test_bars_are_tied_to_the_fp32_oracle_and_stay_under_the_ceilings():
    """Every bar is 8 x the worst distance of the fp32 CPU oracle from the fp64 oracle over its group's cases, recomputed here from
    the table's own inputs: between 4 x and 16 x; and under the project's ceilings, which are conditions and not measurements."""
    assert G.CEILING == dict(y=1e-4, g=3e-4, loss=1e-4, eig=1e-4, grad=3e-4)
    worst = G.group_e32()
    assert set(worst) == set(G.BARS) == {G.group(c) for c in G.CASES} == {(m, s) for m in ("gen", "tr") for s in ("small", "large", "deep")}
    for g, bars in G.BARS.items():
        assert set(bars) == set(worst[g]) == set(G.QUANTITIES) - ({"g"} if g[0] == "tr" else set()), g
        for q, bar in bars.items():
            e = worst[g][q]
            print(f"{g} {q}: bar {bar:.2e}, worst e32 {e:.2e}, ceiling {G.CEILING[q]:.0e}")
            assert 4 * e <= bar <= 16 * e, f"{g} {q}: bar {bar:.2e}, worst e32 {e:.2e}"
            assert bar < G.CEILING[q], f"{g} {q}: bar {bar:.2e}"


def test_eigenvalues_of_every_case_are_apart():
    """The eigenvalues are compared in sorted order, and the order is asserted: no case may have two of them closer than
    ten times the bar they are held to (two results within the bar keep the order of values more than two bars apart)."""
    import numpy as np
    for c in G.CASES:
        eig = G.reference(c)["eig"]
        assert np.all(eig > 0) and np.all(np.isfinite(G.reference(c)["grad"]))
        if c.k > 1:
            assert float(np.min(np.diff(eig) / eig[1:])) > 10 * G.BARS[G.group(c)]["eig"], c.id
