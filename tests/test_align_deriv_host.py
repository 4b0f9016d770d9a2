"""CPU (-m "not gpu"): the case table of the derivative entry points (tests/align_deriv_cases.py) against the compiled code objects and
against ``cvf_align_feature_deriv_route`` - the plan function ``cvf_align_feature_vjp``, ``_vjp_rows``, ``_jvp``, ``_hvp`` and the
launches of csrc/k1_features.hip launch by, which is host arithmetic on the descriptor's counts and answers without a device.

- the symbol is declared, bound and exported;
- the mirrors of the LDS sums, of the row grouping and of the frames-per-workgroup rule agree with the route, field by field;
- every kernel of k1_vjp.o, k1_jvp.o, k1_hvp.o and k1_features.o is claimed by a case, and nothing is claimed that is not compiled
  (``metric_gram_kernel`` belongs to tests/metric_cases.py);
- the table reaches the edges it names, both sides of every threshold one record apart;
- every bar is ``max(1.5e-5, 3 x twin)`` and stays under the 1e-4 condition;
- what the entry points refuse is still refused by name, by the route and by the calls themselves before any launch."""
import ctypes as C
import os
import re

import pytest

from tests import align_deriv_cases as D
from tests import codeobj

TEMPLATES = ("vjp_align_kernel", "vjp_rows_small_kernel", "hvp_align_kernel", "jvp_align_kernel", "vjp_large_kernel",
             "vjp_weighted_large_kernel", "vjp_rows_large_kernel", "vjp_rows_weighted_large_kernel", "jvp_large_kernel",
             "hvp_large_kernel")
PLAIN = ("features_fwd_kernel", "features_vjp_kernel", "features_jvp_kernel", "features_metric_kernel", "features_hvp_kernel")
# the instances no test launched before this table (the tables or the q image outside the LDS; the k-row kernels of large frames)
NEW = [("vjp_align_kernel", (0,)), ("vjp_rows_small_kernel", (0,)), ("hvp_align_kernel", (0,)), ("jvp_align_kernel", (0, 0)),
       ("jvp_align_kernel", (0, 1))] + [(f"vjp_rows_{w}large_kernel", (v,)) for w in ("", "weighted_") for v in (0, 1)]


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    codeobj.built_objects()
    from colvarsfinder import _hip
    _hip.lib()
    return _hip


def test_symbol_is_declared_bound_and_exported(hip):
    with open(os.path.join(codeobj.ROOT, "include", "cvf.h")) as f:
        header = f.read()
    assert re.search(r"\bint cvf_align_feature_deriv_route\(const cvf_pp_desc\* pp, int64_t B, int which, int k, int out_aligned16, "
                     r"cvf_deriv_plan\* plan\);", header)
    assert "cvf_align_feature_deriv_route" in hip.EXPORTED_SYMBOLS and hasattr(hip.lib(), "cvf_align_feature_deriv_route")
    for name, value in (("VJP", 0), ("VJP_ROWS", 1), ("JVP", 2), ("HVP", 3), ("ROUTE_IDENTITY", 0), ("ROUTE_FEATURES", 1),
                        ("ROUTE_SMALL", 2), ("ROUTE_LARGE", 3)):
        assert re.search(rf"CVF_DERIV_{name} = {value}\b", header), name
    assert (hip.DERIV_VJP, hip.DERIV_VJP_ROWS, hip.DERIV_JVP, hip.DERIV_HVP, hip.DERIV_FEATURES_FWD, hip.DERIV_FEATURES_METRIC) == \
        (D.VJP, D.VJP_ROWS, D.JVP, D.HVP, D.FWD, D.METRIC)
    assert (hip.DERIV_IDENTITY, hip.DERIV_FEATURES, hip.DERIV_SMALL, hip.DERIV_LARGE) == (D.IDENTITY, D.FEATURES, D.SMALL, D.LARGE)
    assert [n for n, _ in hip.DerivPlan._fields_] == ["family", "tables_lds", "q_lds", "u_lds", "weighted", "vec4", "lg", "rows_per_launch",
                                                       "launches", "reserved", "lds_bytes", "grid"]
    assert C.sizeof(hip.DerivPlan) == 10 * 4 + 2 * 8
    assert (D.MAX_SLOT, D.MAX_REF) == (hip.FEATURES_MAX_SLOT, hip.FEATURES_MAX_REF)


def test_mirrors_equal_the_route(hip):
    """Every case and every call it makes, at both alignments of the output: the plan of the route equals the mirrors' field by field."""
    for c in D.CASES:
        desc = D.host_desc(c)
        for which in (D.VJP, D.VJP_ROWS, D.JVP, D.HVP) + ((D.FWD, D.METRIC) if c.kind == "feat" else ()):
            for k in {c.k, 1, 3, D.MAX_NETS}:
                for al in (True, False):
                    rc, plan = D.abi_route(desc, c.B, which, k, al)
                    assert rc == 0, (c.id, which, hip.lib().cvf_last_error())
                    assert plan == D.expected_plan(c, which, k=k, aligned16=al), (c.id, which, k, al, plan)
    # batches: the grid follows B
    c = D.BY_ID["heavy64"]
    for B in D.BATCHES:
        assert D.abi_route(D.host_desc(c), B, D.HVP)[1]["grid"] == D.n_tiles(B)
    # identity: a copy, no kernel
    from colvarsfinder.pp import identity_desc
    for which in (D.VJP, D.VJP_ROWS, D.JVP, D.HVP):
        rc, plan = D.abi_route(identity_desc(7), 100, which, 2)
        assert rc == 0 and plan["family"] == D.IDENTITY and plan["lds_bytes"] == plan["grid"] == 0


def _compiled(tmp_path):
    build = codeobj.built_objects()
    out, names = set(), []
    for obj in ("k1_vjp.o", "k1_jvp.o", "k1_hvp.o", "k1_features.o"):
        for name in codeobj.kernels_of(os.path.join(build, obj), tmp_path):
            if codeobj.template_args(name, "metric_gram_kernel") is not None:
                continue                                       # (tests/metric_cases.py owns it)
            names.append(name)
            for family in TEMPLATES:
                args = codeobj.template_args(name, family)
                if args is not None:
                    out.add((family, args))
            for family in PLAIN:
                if re.search(rf"\d+{family}E", name):
                    out.add((family, ()))
    return out, names


def test_every_compiled_kernel_is_claimed_and_nothing_else(hip, tmp_path):
    compiled, names = _compiled(tmp_path)
    assert len(compiled) == len(names), sorted(names)          # every kernel of the four objects is one of the families above
    claimed = set().union(*(D.instances(c) for c in D.CASES))
    print(sorted(compiled))
    assert claimed == compiled, (sorted(claimed - compiled), sorted(compiled - claimed))
    assert set(NEW) <= compiled
    assert ("jvp_align_kernel", (1, 0)) not in compiled        # (the tables are never staged without the q image)


def test_the_table_reaches_its_edges(hip):
    assert len({c.id for c in D.CASES}) == len(D.CASES)
    assert {c.B for c in D.CASES} == set(D.BATCHES)
    for c in D.CASES:                                           # the lists are what the module's docstring says they are
        s, layer = D.build(c), D.layer_of(c)
        assert s.unused and c.n - 1 in s.unused, c.id
        assert s.feats[0][0] == "position" and len(s.feats[0][1]) == c.counts[0] >= 1, c.id
        assert set(s.cols) == set(D.TYPES) and D.counts_of(c.counts, c.angle) == (layer.rec.shape[0], layer.d_r, layer._n_ref), c.id
        if c.kind != "feat":
            assert 3 <= len(s.align) == c.n_align < c.n - 1 and layer._flags & 3 == 0, c.id
            assert (layer.align_w is not None) == c.weighted and (not c.weighted or c.kind == "large" or layer._flags == 0), c.id
        else:
            # (n_align: the pool of a features case; an atom whose partner was too close may stay unread)
            assert 0 <= c.n_align - layer._n_slot <= 2 + c.n_align // 100 and not layer.aligned, c.id
        assert c.kind == "feat" or (c.kind == "small") == (3 * c.n <= 192), c.id
    # every instance no test launched before: a batch below one tile and B = 65
    batches = {}
    for c in D.CASES:
        for inst in D.instances(c):
            batches.setdefault(inst, set()).add(c.B)
    for inst in NEW:
        assert 65 in batches[inst] and min(batches[inst]) < 64, (inst, batches[inst])
    # both sides of every small-frame threshold, one record apart
    plan = lambda cid, which: D.expected_plan(D.BY_ID[cid], which)
    for stem, which, field in (("vjp-tables", D.VJP, "tables_lds"), ("rows-tables", D.VJP_ROWS, "tables_lds"),
                               ("hvp-tables", D.HVP, "tables_lds"), ("jvp-q", D.JVP, "q_lds"), ("jvp-tables", D.JVP, "tables_lds")):
        u, o = D.BY_ID[stem + "-under"], D.BY_ID[stem + "-over"]
        assert D.counts(o)[1] == D.counts(u)[1] + 1 and u.n == o.n == 64 and u.n_align == o.n_align, stem
        assert (plan(u.id, which)[field], plan(o.id, which)[field]) == (1, 0), stem
        assert plan(u.id, which)["lds_bytes"] <= D.LIMIT and plan(u.id, which)["lds_bytes"] > D.LIMIT - 6 * 4 * 64, stem
    assert (plan("jvp-q-under", D.JVP)["tables_lds"], plan("jvp-tables-over", D.JVP)["q_lds"]) == (0, 1)
    q = plan("qwin40", D.JVP)
    assert D.BY_ID["qwin40"].n == 40 and (q["tables_lds"], q["q_lds"]) == (0, 1)
    for cid in ("heavy64", "heavy64w"):
        assert all(plan(cid, w)["tables_lds"] == plan(cid, w)["q_lds"] == 0 for w in (D.VJP, D.VJP_ROWS, D.JVP, D.HVP)), cid
    assert D.BY_ID["heavy64w"].weighted and D.layer_of(D.BY_ID["heavy64w"])._flags == 0
    # small rows: a grouping with kg < k and k % kg != 0, for k = 3 and k = 8
    groups = {(c.k, plan(c.id, D.VJP_ROWS)["rows_per_launch"]) for c in D.SMALL_CASES if "rows" in c.runs}
    for k in (3, 8):
        assert any(kk == k and kg < k and k % kg for kk, kg in groups), (k, groups)
    # large rows: two and three launches of each of the four instances, k = 8; the misaligned calls on 16-byte instances
    seen = {(c.weighted, plan(c.id, D.VJP_ROWS)["vec4"], plan(c.id, D.VJP_ROWS)["launches"]) for c in D.LARGE_CASES}
    assert seen == {(w, v, n) for w in (False, True) for v in (0, 1) for n in (2, 3)} and all(c.k == 8 for c in D.LARGE_CASES)
    for cid in D.MISALIGNED:
        assert plan(cid, D.VJP_ROWS)["vec4"] == 1 and D.expected_plan(D.BY_ID[cid], D.VJP_ROWS, aligned16=False)["vec4"] == 0
    assert {D.BY_ID[cid].weighted for cid in D.MISALIGNED} == {False, True}
    assert {c.angle for c in D.LARGE_CASES} == {c.angle for c in D.SMALL_CASES} == {False, True}
    # the features ladder: every frames-per-workgroup step of every launch, u in LDS and not, the limits of include/cvf.h kept
    for which in (D.FWD, D.VJP, D.VJP_ROWS, D.JVP, D.METRIC, D.HVP):
        assert {D.expected_plan(c, which)["lg"] for c in D.FEAT_CASES} == set(range(7)), which
    assert {D.expected_plan(c, D.HVP)["u_lds"] for c in D.FEAT_CASES} == {0, 1}
    assert {D.expected_plan(c, D.METRIC)["rows_per_launch"] < c.k for c in D.FEAT_CASES} == {False, True}    # nets in one pass and in several
    big = D.BY_ID["feat-s4000"]
    assert big.n == 4096 and big.B == 5 and max(c.n for c in D.CASES) == 4096
    assert all(D.counts(c)[4] <= D.MAX_SLOT and D.counts(c)[5] <= D.MAX_REF for c in D.FEAT_CASES)
    assert D.expected_plan(big, D.HVP)["lds_bytes"] <= D.LIMIT and D.expected_plan(big, D.METRIC)["lds_bytes"] + 8192 <= D.LIMIT


def test_bars_are_tied_to_the_twin_and_keep_the_condition():
    worst = {}
    for c in D.CASES:
        r = D.reference(c)
        assert set(r.twin) >= {"vjp" if q == "rows" else q for q in c.runs}, c.id      # (the double backward brings J^T g along)
        for q, d in r.twin.items():
            for t, e in d.items():
                assert r.bar[q][t] == max(D.FLOOR, D.TWIN_MARGIN * e) <= D.CEILING, (c.id, q, t, e)
                worst[(c.kind, q, t)] = max(worst.get((c.kind, q, t), 0.0), e)
    for key, e in sorted(worst.items()):
        print(f"{key}: worst twin error {e:.2e}")
    assert (D.FLOOR, D.TWIN_MARGIN, D.CEILING) == (1.5e-5, 3.0, 1e-4)


def test_the_older_abi_tests_keep_the_ceiling_too():
    """test_vjp_abi_vs_oracle and test_jvp_abi_vs_oracle hold their shapes to the same measure.  Their lists are not filtered: every
    (shape, type) keeps 3 x twin <= CEILING but the ones deriv_measure.TWIN_ABOVE_CEILING names, whose bar is the ceiling itself - no
    bar of either test exceeds it."""
    from tests import deriv_measure as DM
    from tests import test_align_jvp_gpu as J
    from tests import test_align_vjp_gpu as V
    assert (DM.FLOOR, DM.TWIN_MARGIN, DM.CEILING) == (D.FLOOR, D.TWIN_MARGIN, D.CEILING) and DM.bar_of(1.0) == DM.CEILING
    twins = {}
    for name, B, av, tol in V.ABI_CASES:
        assert tol == DM.FLOOR
        twins.update({("vjp", name, av, t): tw for t, (_, _, tw) in V.typed_refs(name, B, av)[0].items()})
    for name, B, av in J.ABI_CASES:
        twins.update({("jvp", name, av, t): tw for t, (_, tw) in J.typed_refs(name, B, av)[1].items()})
    assert DM.TWIN_ABOVE_CEILING <= set(twins)
    capped = {}
    for key, tw in twins.items():
        assert DM.FLOOR <= DM.bar_of(tw) <= DM.CEILING, key
        if DM.TWIN_MARGIN * tw > DM.CEILING:
            capped[key] = tw
        assert key in DM.TWIN_ABOVE_CEILING or DM.TWIN_MARGIN * tw <= DM.CEILING, (key, tw)
    print("bars capped at the ceiling:", {k: f"{v:.1e}" for k, v in capped.items()})
    assert capped, "no twin above the ceiling any more: empty TWIN_ABOVE_CEILING"


def test_refusals_by_name_and_before_any_launch(hip):
    lib, tok = hip.lib(), C.c_void_p(64)                        # (a non-NULL token: every call below is refused before it reads a pointer)

    def refused(desc, what, which=(D.VJP, D.VJP_ROWS, D.JVP, D.HVP), k=2, route=True):
        for w in which:
            if route:
                assert D.abi_route(desc, 5, w, k)[0] < 0 and what in lib.cvf_last_error(), (w, what, lib.cvf_last_error())
            rc = {D.VJP: lambda: lib.cvf_align_feature_vjp(C.byref(desc), tok, 5, tok, tok, tok, None),
                  D.VJP_ROWS: lambda: lib.cvf_align_feature_vjp_rows(C.byref(desc), tok, 5, tok, k, tok, tok, None),
                  D.JVP: lambda: lib.cvf_align_feature_jvp(C.byref(desc), tok, 5, tok, tok, tok, None),
                  D.HVP: lambda: lib.cvf_align_feature_hvp(C.byref(desc), tok, 5, tok, tok, tok, tok, None)}[w]()
            assert rc < 0 and what in lib.cvf_last_error(), (w, what, lib.cvf_last_error())

    # small-frame weights with flags != 0
    d = D.host_desc(D.BY_ID["heavy64w"])
    d.flags = hip.PP_ALIGN_CONTIG
    refused(d, b"need flags == 0")
    # large frames: the tables are missing (counts: the route; pointers: the calls), n_ref beyond the LDS
    big = D.BY_ID["lrows-n66-r700-u"]
    d = D.host_desc(big)
    d.align_idx = d.ref_c = d.rec = 64                          # (the small tables are there, the slot and row tables are not)
    refused(d, b"frames of more than 192 coordinates need", route=False)
    assert all(D.abi_route(d, 5, w, 2)[0] == 0 for w in (D.VJP, D.VJP_ROWS, D.JVP, D.HVP))
    d.n_slot = 0
    refused(d, b"frames of more than 192 coordinates need")
    d = D.host_desc(big)
    d.n_ref = D.LIMIT // 12 + 1
    refused(d, b"do not fit the LDS", which=(D.VJP, D.VJP_ROWS, D.HVP))
    # no alignment: the limits of include/cvf.h
    f = D.BY_ID["feat-s4000"]
    d = D.host_desc(f)
    d.n_slot = D.MAX_SLOT + 1
    refused(d, b"CVF_FEATURES_MAX_SLOT")
    assert D.abi_route(d, 5, D.FWD, 1)[0] < 0 and b"CVF_FEATURES_MAX_SLOT" in lib.cvf_last_error()
    d = D.host_desc(f)
    d.n_ref = D.MAX_REF + 1
    refused(d, b"CVF_FEATURES_MAX_REF")
    assert D.abi_route(d, 5, D.METRIC, 1)[0] < 0 and b"CVF_FEATURES_MAX_REF" in lib.cvf_last_error()
    # k beyond CVF_MAX_NETS, an empty batch, another mode, an unknown call
    for cid in ("heavy64", "lrows-n66-r700-u", "feat-s10"):
        d = D.host_desc(D.BY_ID[cid])
        refused(d, b"k outside 1..8", which=(D.VJP_ROWS,), k=D.MAX_NETS + 1)
        refused(d, b"k outside 1..8", which=(D.VJP_ROWS,), k=0)
        assert all(D.abi_route(d, 0, w, 1)[0] < 0 for w in range(4))
        assert D.abi_route(d, 5, 6, 1)[0] < 0 and D.abi_route(d, 5, -1, 1)[0] < 0
    d = D.host_desc(D.BY_ID["heavy64"])
    assert D.abi_route(d, 5, D.FWD, 1)[0] < 0 and b"CVF_PP_FEATURES only" in lib.cvf_last_error()
    from colvarsfinder.pp import factored_desc
    refused(factored_desc(4, 2), b"CVF_PP_FACTORED")
    assert lib.cvf_align_feature_deriv_route(None, 5, 0, 1, 1, C.byref(hip.DerivPlan())) < 0
    assert lib.cvf_align_feature_deriv_route(C.byref(d), 5, 0, 1, 1, None) < 0
