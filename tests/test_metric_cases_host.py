"""CPU (-m "not gpu"): the case table of the metric kernels (tests/metric_cases.py) against the compiled code objects and against
``cvf_metric_route`` - the plan function ``cvf_metric_apply`` and ``cvf_metric_apply_stats`` launch by, which is host arithmetic on the
descriptor's counts and answers without a device.

- every compiled instance of ``metric_rows_kernel``, ``metric_pure_kernel``, ``metric_align_kernel`` and ``metric_dense_kernel`` is
  claimed by a case or listed in ``UNREACHABLE`` with a reason, and nothing is claimed that is not compiled;
- the mirrors of the LDS formulae, of the instance choice and of the nets-per-workgroup rule agree with the route, field by field;
- the edges the table claims are properties of its feature lists, asserted on the tables ``AlignFeatureLayer`` builds;
- what the table's docstring calls unreachable is unreachable by the LDS formula;
- every bar is ``max(1.5e-5, 3 x twin)`` and stays under the 1e-4 condition."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import codeobj
from tests import metric_cases as M


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    codeobj.built_objects()
    from colvarsfinder import _hip
    _hip.lib()
    return _hip


@pytest.fixture
def npb_env():
    """CVF_METRIC_NPB is read on every call: set per case, restored afterwards."""
    old = os.environ.pop("CVF_METRIC_NPB", None)

    def set_(v):
        os.environ.pop("CVF_METRIC_NPB", None)
        if v is not None:
            os.environ["CVF_METRIC_NPB"] = str(v)

    yield set_
    os.environ.pop("CVF_METRIC_NPB", None)
    if old is not None:
        os.environ["CVF_METRIC_NPB"] = old


def _route(hip, desc, B, k, with_stats):
    plan = hip.MetricPlan()
    rc = hip.lib().cvf_metric_route(C.byref(desc), B, k, int(with_stats), C.byref(plan))
    return rc, {name: getattr(plan, name) for name, _ in plan._fields_ if name != "reserved"}


def _compiled(tmp_path):
    build = codeobj.built_objects()
    out = set()
    for obj in ("metric_large.o", "k1_align.o"):
        for name in codeobj.kernels_of(os.path.join(build, obj), tmp_path):
            for family in ("metric_rows_kernel", "metric_dense_kernel"):
                args = codeobj.template_args(name, family)
                if args is not None:
                    out.add((family, args))
            for family in ("metric_pure_kernel", "metric_align_kernel"):
                if re.search(rf"\d+{family}E", name):
                    out.add((family, ()))
    return out


def test_symbol_is_declared_bound_and_exported(hip):
    with open(os.path.join(codeobj.ROOT, "include", "cvf.h")) as f:
        header = f.read()
    assert re.search(r"\bint cvf_metric_route\(const cvf_pp_desc\* pp, int64_t B, int k, int with_stats, cvf_metric_plan\* plan\);", header)
    assert "cvf_metric_route" in hip.EXPORTED_SYMBOLS and hasattr(hip.lib(), "cvf_metric_route")
    assert (hip.METRIC_ALIGN, hip.METRIC_PURE, hip.METRIC_ROWS) == (M.ROUTE_ALIGN, M.ROUTE_PURE, M.ROUTE_ROWS)
    for name, value in (("IDENTITY", 0), ("FACTORED", 1), ("FEATURES", 2), ("ALIGN", 3), ("PURE", 4), ("ROWS", 5)):
        assert re.search(rf"CVF_METRIC_ROUTE_{name} = {value}\b", header), name


def test_every_compiled_instance_is_claimed_and_nothing_else(hip, tmp_path):
    compiled = _compiled(tmp_path)
    assert {f for f, _ in compiled} == {"metric_rows_kernel", "metric_dense_kernel", "metric_pure_kernel", "metric_align_kernel"}
    claimed = {M.instance(c) for c in M.ALL_CASES}
    claimed |= {("metric_dense_kernel", (int(c.weighted),)) for c in M.ALL_CASES if c.kind == "rows"}
    print(sorted(compiled))
    assert claimed <= compiled, sorted(claimed - compiled)
    assert not set(M.UNREACHABLE) & claimed and set(M.UNREACHABLE) <= compiled
    assert all(len(why) > 20 for why in M.UNREACHABLE.values())
    assert compiled - claimed == set(M.UNREACHABLE), sorted(compiled - claimed - set(M.UNREACHABLE))
    # the instances behind the process-wide switches are claimed by the child's cases only, the others by the test process
    here = {M.instance(c) for c in M.CASES}
    assert {a for f, a in compiled - here if f == "metric_rows_kernel"} == {(16, 16, 2, 1), (8, 16, 2, 1), (4, 16, 2, 1), (16, 8, 5, 1)}
    assert all((c.waves, c.pre) == (8, 7) for c in M.CASES) and all((c.waves, c.pre) != (8, 7) for c in M.SWITCH_CASES)


def test_mirrors_equal_the_route(hip, npb_env):
    """Every case, apply and apply_stats: the plan of the route equals the mirrors' field by field.  (The switch instances are asked
    of the route in the child process, where the switches are set: tests/metric_switch_child.py.)"""
    for c in M.CASES:
        desc, layer = M.host_desc(c)
        assert layer.derivative_table_limits() is None, c.id
        for npb in {c.npb, None}:
            npb_env(npb)
            for with_stats in (False, True):
                rc, plan = _route(hip, desc, c.B, c.k, with_stats)
                assert rc == 0, (c.id, hip.lib().cvf_last_error())
                assert plan == M.expected_plan(c, with_stats, npb=npb), (c.id, npb, with_stats)
    for cid, B, k in M.STATS_CASES:
        c = M.BY_ID[cid]
        desc, _ = M.host_desc(c)
        npb_env(c.npb)
        rc, plan = _route(hip, desc, B, k, True)
        assert rc == 0 and plan == M.expected_plan(c, True, B=B, k=k), (cid, B)


def test_npb_is_read_on_every_call_and_only_divisors_count(hip, npb_env):
    c = M.BY_ID["f8-rec-520"]
    desc, _ = M.host_desc(c)
    seen = []
    for env in (1, 2, 4, 8, 3, 0, None):
        npb_env(env)
        rc, plan = _route(hip, desc, c.B, c.k, False)
        assert rc == 0
        seen.append(plan["npb"])
        assert plan["multi"] == int(plan["npb"] > 1) and plan["grid"] == M.n_tiles(c.B) * 8 * c.k // plan["npb"]
    auto = M.rows_npb(c.B, c.k, 8)
    assert seen == [1, 2, 4, 8, auto, auto, auto]
    # the cost model takes both branches over the table's batches and the stats batches
    assert {M.rows_npb(B, 6, 16) for B in (65, 16000)} == {1, 6}


def test_route_refusals(hip, npb_env):
    npb_env(None)
    c = M.BY_ID["f4-lds-under"]
    desc, _ = M.host_desc(c)
    assert _route(hip, desc, c.B, c.k, False)[0] == 0
    desc.n_ref = M.M4 + 1                                     # one row past the smallest layout
    assert M.rows_F(M.M4, 100) == 4 and M.rows_F(M.M4 + 1, 100) is None
    assert _route(hip, desc, c.B, c.k, False)[0] < 0 and b"158 KiB" in hip.lib().cvf_last_error()
    desc.n_ref = c.n_ref
    for B, k in ((0, 1), (5, 0), (5, M.MAX_NETS + 1)):
        assert _route(hip, desc, B, k, False)[0] < 0
    desc.n_mrec = 0
    assert _route(hip, desc, c.B, c.k, False)[0] < 0 and b"record / row tables" in hip.lib().cvf_last_error()
    w = M.BY_ID["align-n10-w-k2-B63"]
    desc, _ = M.host_desc(w)
    assert _route(hip, desc, w.B, w.k, False)[0] == 0
    desc.flags = M.PP_ALIGN_CONTIG
    assert _route(hip, desc, w.B, w.k, False)[0] < 0 and b"flags == 0" in hip.lib().cvf_last_error()
    assert hip.lib().cvf_metric_route(None, 5, 1, 0, C.byref(hip.MetricPlan())) < 0


def _tables(case):
    layer = M.layer_of(case)
    rows = np.diff(layer.slot_row.numpy())
    return layer, rows


def test_the_table_reaches_its_edges():
    cases = M.ROWS_CASES + M.SWITCH_CASES
    assert len({c.id for c in M.ALL_CASES}) == len(M.ALL_CASES)
    assert set(M.BATCHES) <= {c.B for c in M.CASES}
    assert all(c.B in M.BATCHES or f"-B{c.B}" in c.id for c in M.ALL_CASES)       # (the ragged cases bring the batches their F needs)
    F_of = {c.id: M.rows_F(c.n_ref, c.n_slot, c.waves) for c in cases}
    for c in cases:                                             # the lists are what the table says they are
        layer, rows = _tables(c)
        assert (layer._n_slot, layer.mrec.shape[0], layer._n_ref) == (c.n_slot, c.n_mrec, c.n_ref), c.id
        assert c.id.split("-")[0 if c.waves == 8 and c.pre == 7 else 1] == f"f{F_of[c.id]}", c.id
        slot_of = {a: i for i, a in enumerate(layer.slot_atom.tolist())}
        pool = M.build(c).pool
        for idx, count in c.hubs:
            assert rows[slot_of[pool[idx]]] == count, c.id
    # LDS thresholds: both sides of each, at one row's distance
    for F, under, over in ((16, "f16-lds-under", "f8-lds-over"), (8, "f8-lds-under", "f4-lds-over")):
        u, o = M.BY_ID[under], M.BY_ID[over]
        assert o.n_ref == u.n_ref + 1 and u.n_slot == o.n_slot
        assert M.rows_lds(u.n_ref, u.n_slot, F) <= M.BUDGET < M.rows_lds(o.n_ref, o.n_slot, F)
    u = M.BY_ID["f4-lds-under"]
    assert M.rows_lds(u.n_ref, u.n_slot, 4) <= M.BUDGET < M.rows_lds(u.n_ref + 1, u.n_slot, 4)
    for F in (16, 8, 4):
        mine = [c for c in M.ROWS_CASES if F_of[c.id] == F]
        regs, LG = M.in_regs(F), M.lane_groups(F)
        recs = {c.n_mrec for c in mine}
        if F == 16:
            assert min(recs) < LG and {regs - 1, regs, regs + 1} <= recs
        if F == 8:
            assert {regs - 1, regs, regs + 1} <= recs
        assert max(recs) > 2 * regs and all(r > regs for r in recs) == (F == 4)
        # slots: LG * kSlots - 1, + 0, + 1 (two of them no multiple of 3 ... of kSlots), a tail that leaves one and two slots of a triple
        slots = {c.n_slot for c in mine}
        edge = LG * M.K_SLOTS
        assert {edge - 1, edge + 1} <= slots and any(s % M.K_SLOTS for s in slots), F
        assert {(c.n_slot - 1) % edge // LG for c in mine} >= {0, 1, 2}, F      # the last triple of some lane group holds 1, 2 and 3 slots
        # an atom shared by 1, by 2 and by 40 records; the last slot the most shared one; and a last slot of ONE row while the slot a
        # stride of LG before it - another slot of the same lane group's triple - has 40: that slot's reads run past the table's last
        # row and take the n_ref - 1 clamp
        counts = {n for c in mine for _, n in c.hubs}
        assert {1, 2, 40} <= counts, F
        most = [c for c in mine if (-1, 40) in c.hubs]
        assert most and any(_tables(c)[1].argmax() == c.n_slot - 1 and _tables(c)[1].max() == 40 for c in most), F
        clamp = [c for c in mine if (-1, 1) in c.hubs and (-1 - LG, 40) in c.hubs]
        assert clamp and all(c.n_slot > LG for c in clamp), F
        # nets: k = 1, 3, 6, 8; CVF_METRIC_NPB = 1, a proper divisor of k, k - kMulti both ways
        assert {1, 3, 6, 8} <= {c.k for c in mine}, F
        assert any(c.npb == 1 and c.k > 1 for c in mine) and any(c.npb == c.k > 1 for c in mine), F
        assert any(c.npb and 1 < c.npb < c.k for c in mine) and any(c.npb is None for c in mine), F
        assert {M.instance(c)[1][3] for c in mine} == {0, 1}, F
        # the other axes
        assert any(c.angle for c in mine) and any(not c.angle for c in mine), F
        assert any(c.n_pos == 0 for c in mine), F
        assert any(c.align == "subset" and M.build(c).unused for c in mine), F
        assert any(c.weighted for c in mine), F
        # ragged batches
        assert {c.B % 64 for c in mine} >= {1, F - 1, F, F + 1, 63}, F
    assert any(c.align == "subset" and c.weighted for c in M.ROWS_CASES)
    # the switch instances: the edges of their own LG * kGeoPre
    for W, pre, F in ((16, 7, 16), (16, 7, 8), (16, 7, 4), (8, 5, 16)):
        mine = [c for c in M.SWITCH_CASES if (c.waves, c.pre, F_of[c.id]) == (W, pre, F)]
        regs = M.in_regs(F, W, True, pre)
        assert mine and any(c.n_mrec > regs for c in mine) and any(abs(c.n_mrec - regs) == 1 for c in mine), (W, pre, F)
        assert all(M.expected_plan(c)["geo_pre"] == (2 if W == 16 else 5) for c in mine)
    assert any(c.n_mrec < M.lane_groups(16, 16) for c in M.SWITCH_CASES if c.waves == 16)
    # stats: the fused stage at 384 frame groups, the two-stage path at 385, on each F; the pure kernel at 1024 and 1025 tiles
    plans = {(cid, B): M.expected_plan(M.BY_ID[cid], True, B=B, k=k) for cid, B, k in M.STATS_CASES}
    for F in (16, 8, 4):
        got = {(p["fused"], p["fused_rows"]) for (cid, B), p in plans.items() if p["F"] == F and B > 1000}
        assert got == {(1, 384), (0, 0)}, F
        assert {B // F for (cid, B), p in plans.items() if p["F"] == F and B > 1000} == {384, 385}
    assert {(p["fused"], p["fused_rows"]) for (cid, B), p in plans.items() if p["family"] == M.ROUTE_PURE and B > 1000} == {(1, 1024), (0, 0)}
    assert min(c.n for c in M.PURE_CASES) == M.BY_ID["pure-n3-al3-k8-B65"].n


def test_pure_and_align_edges():
    pure = M.PURE_CASES
    assert {c.n_slot for c in pure} == {3, 7, 8, 9, 16, 17, 22, 64}                      # n_rec: around kGChunk = 8 and its multiples
    assert {c.n_slot % M.G_CHUNK for c in pure} >= {0, 1, 7} and M.G_CHUNK == 8
    for n_rec in (7, 8, 9, 16, 17, 22, 64):
        als = {c.align for c in pure if c.n_slot == n_rec}
        assert n_rec in als and min(als) < n_rec, n_rec
    assert any(c.n > c.n_slot for c in pure)                                             # atoms no feature reads
    wpb = {(c.n_slot, M.pure_wpb(3 * c.n, c.align, c.k), c.k) for c in pure}
    for n_rec in (16, 17, 22):                                                           # k on both sides of the 80 KiB line
        assert any(w == k > 1 for n, w, k in wpb if n == n_rec) and any(w == 1 < k for n, w, k in wpb if n == n_rec), n_rec
    c = M.BY_ID["pure-n22-al22-k3-B65"]
    assert M.pure_lds(66, 22, 3) <= M.PURE_ALL_NETS_LDS < M.pure_lds(66, 22, 4)
    assert {1, 3, 6, 8} <= {c.k for c in pure}
    for c in pure:
        assert M.layer_of(c)._flags & 3 == 3, c.id
    al = M.ALIGN_CASES
    assert {(c.n, c.weighted) for c in al} == {(10, False), (10, True), (64, False), (64, True)}
    for c in al:
        layer = M.layer_of(c)
        assert layer._flags & 3 != 3 and (not c.weighted or layer._flags == 0) and layer.features == [(t, tuple(a)) for t, a in M.MIXED]
    assert {c.angle for c in al} == {False, True}


def test_unreachable_edges_are_unreachable():
    """The docstring of tests/metric_cases.py: with n_slot <= n_ref <= 4 n_mrec the F = 8 and F = 4 layouts cannot meet a list of fewer
    than LG records, nor F = 4 with 8 waves one of 255 to 257."""
    for W in (8, 16):
        for F, bigger in ((8, 16), (4, 8)):
            LG = M.lane_groups(F, W)
            most_rows = 4 * (LG - 1)
            assert all(M.rows_lds(most_rows, s, bigger, W) <= M.BUDGET for s in range(1, most_rows + 1)), (W, F)
    assert all(M.rows_lds(4 * 257, s, 8, 8) <= M.BUDGET for s in range(1, 4 * 257 + 1))
    assert M.in_regs(4, 8) == 256 and M.in_regs(4, 16) == 512


def test_bars_are_tied_to_the_twin_and_keep_the_condition():
    worst = {}
    for c in M.ALL_CASES:
        r = M.reference(c)
        assert r.bar_q == max(M.FLOOR, M.TWIN_MARGIN * r.twin_q) and r.bar_E == max(M.FLOOR, M.TWIN_MARGIN * r.twin_E)
        assert r.bar_q <= M.CEILING and r.bar_E <= M.CEILING, (c.id, r.twin_q, r.twin_E)
        kind = c.kind if c.kind != "rows" else f"rows-f{M.rows_F(c.n_ref, c.n_slot, c.waves)}"
        w = worst.setdefault(kind, [0.0, 0.0])
        w[0], w[1] = max(w[0], r.twin_q), max(w[1], r.twin_E)
    for kind, (tq, tE) in sorted(worst.items()):
        print(f"{kind}: worst twin error q {tq:.2e}, E {tE:.2e}")
    assert (M.FLOOR, M.TWIN_MARGIN, M.CEILING) == (1.5e-5, 3.0, 1e-4)
