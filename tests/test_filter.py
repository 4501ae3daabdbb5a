"""Engine.filter_traces (tw_filter_traces, csrc/tw_filt.h): the stitched traces selected by a predicate on the device, the match as bit
MATCH of the forest's flags, which every later stage selects by.  The yardstick is traces.filter_host, the definitions of
include/traceweaver_amd.h restated with loops over the rows of a tree; part 1 checks it on the forest written out by hand in
tests/test_signatures.py, the rest compares the device with it, np.array_equal and equal dtype on every field of TraceFilter.FIELDS.
Corpora, cases and helpers are those of tests/test_stitch.py, test_attribute.py, test_signatures.py and test_profiles.py.  CPU tier:
host-emulation build (four trees to a wavefront, a tree of more than 12 rows alone: both routes occur; one lane per workgroup, and once
one host thread per lane); the HIP library under -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_attribute as ta
import test_profiles as tp
import test_signatures as tg
import test_stitch as ts
from traceweaver_amd import traces
from traceweaver_amd.engine import Engine, EngineError
from traceweaver_amd.traces import clause

NV = traces.NO_VALUE
W, M = traces.WHOLE, traces.MATCH
DTYPES = {"tree_match": np.uint8, "match_trees": np.int32}


def same(got, want, tag=None):
    for k in traces.TraceFilter.FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), (k, tag)
        assert getattr(got, k).dtype == getattr(want, k).dtype == DTYPES.get(k, np.int64), (k, tag)
    assert np.array_equal(got.match_trees, np.flatnonzero(got.tree_match)), tag


def with_match(st, f):
    """The forest as the device holds it after the filter: bit MATCH of the flags set on the matched trees."""
    flags = (np.asarray(st.tree_flags) | (M * np.asarray(f.tree_match))).astype(np.uint8)
    return traces.StitchedTraces(st.root, st.depth, st.tree_off, st.tree_rows, st.tree_root, st.tree_latency, flags, st.counts)


# ---- 1. the restatement on the forest written out by hand -----------------------------------------------------------------------
A, B, C, D = tg.A, tg.B, tg.C, tg.D


def hand(clauses, need=W, skip=0):
    """The HAND forest of tests/test_signatures.py, rows and latencies as hand() of tests/test_profiles.py builds them: a root row is
    [1000 r, 1000 r + latency], every other row [base + 1, base + 2]; the client rows (and the absent row 32) carry group 0 = A."""
    lat = dict(zip(tg.HAND_ROOTS, tg.HAND_LATENCY))
    rows, base = [], 0
    for r, (kind, g, link) in enumerate(tg.HAND):
        if r in lat:
            base = 1000 * r
            rows.append((base, base + lat[r], link))
        else:
            rows.append((base + 1, base + 2, link))
    st, link, start, end = ta.forest(rows, tg.HAND_FLAGS)
    kind, group = [x[0] for x in tg.HAND], [x[1] for x in tg.HAND]
    sig = traces.signatures_host(st, link, kind, group, 4, "levels", 1, 0)
    attr = traces.attribute_host(st, link, start, end, group, 4)
    f = traces.filter_host(st, link, kind, start, end, group, 4, clauses, need, skip, attribution=attr, signatures=sig)
    assert np.array_equal(f.match_trees, np.flatnonzero(f.tree_match)) and f.summary[1] == f.tree_match.sum()
    return f


def test_host_by_hand():
    # trees 0 .. 8: latencies 100, 250, 50, 70, 10, 5, 20, 30, 400; rows 7, 7, 9, 7, 2, 1, 2, 5, 7; trees 5 and 6 are no whole traces.
    # One clause of each subject, each a term of its own
    f = hand([clause("latency", 100, None, term=0), clause("rows", 9, 9, term=1), clause("start", 23000, 30000, term=2), clause("class", 1, 1, term=3),
              clause("group", 2, None, term=4, group=C), clause("edge", 1, None, term=5, group=D, caller=C)])
    assert f.clause_value.T.tolist() == [[100, 250, 50, 70, 10, 5, 20, 30, 400], [7, 7, 9, 7, 2, 1, 2, 5, 7],
                                         [0, 7000, 14000, 23000, 30000, 32000, 33000, 35000, 40000], [0, 0, 1, 2, 3, -1, -1, 4, 0],
                                         [1, 1, 2, 1, 0, 0, 0, 0, 1],            # C twice in tree 2
                                         [0, 1, 0, 0, 0, 0, 0, 0, 0]]            # D under C in tree 1 only
    assert f.clause_trees.tolist() == [3, 1, 2, 1, 1, 1] and f.term_trees.tolist() == [3, 1, 2, 1, 1, 1, 0, 0]
    assert f.tree_match.tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 1] and f.matched().tolist() == [0, 1, 2, 3, 4, 8]
    assert f.summary.tolist() == [7, 6, 880, 10, 400, 39]
    t = f.table(["a", "b", "c", "d"])
    assert t[4] == {"clause": 4, "term": 4, "text": "count[c]>=2", "trees": 1} and t[5]["text"] == "count[c>d]>=1" and t[6] == {"term": 0, "text": "latency>=100", "trees": 3}
    # a minimum over a group that trees 4, 5 and 6 lack: no value, which holds neither plain nor negated
    f = hand([clause("group", 1, None, term=0, group=D, metric="span", reduce="min"), clause("group", 1, None, term=1, group=D, metric="span", reduce="min", negate=True),
              clause("group", 2, None, term=2, group=D, metric="span", reduce="min", negate=True)])
    assert f.clause_value.T.tolist() == [[1, 1, 1, 1, NV, NV, NV, 1, 1]] * 3
    assert f.clause_trees.tolist() == [6, 0, 6] and f.term_trees.tolist() == [6, 0, 6, 0, 0, 0, 0, 0] and f.tree_match.tolist() == [1, 1, 1, 1, 0, 0, 0, 1, 1]
    # a term of two clauses: seven rows and at most 100 us
    f = hand([clause("rows", 7, 7), clause("latency", None, 100)])
    assert f.clause_trees.tolist() == [4, 5] and f.term_trees.tolist() == [2, 0, 0, 0, 0, 0, 0, 0] and f.tree_match.tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0]
    assert f.summary.tolist() == [7, 2, 170, 70, 100, 14]
    # two terms: slow, or at most four counted rows (tree 4: its client row; tree 7: all but the row of group -1)
    f = hand([clause("latency", 250, None, term=0), clause("group", None, 4, term=1, group=-1)])
    assert f.clause_value[:, 1].tolist() == [7, 7, 9, 7, 1, 1, 2, 4, 7]
    assert f.clause_trees.tolist() == [2, 2] and f.term_trees.tolist() == [2, 2, 0, 0, 0, 0, 0, 0] and f.tree_match.tolist() == [0, 1, 0, 0, 1, 0, 0, 1, 1]
    # no clause: every eligible tree
    f = hand([])
    assert f.tree_match.tolist() == [1, 1, 1, 1, 1, 0, 0, 1, 1] and f.summary.tolist() == [7, 7, 910, 10, 400, 44] and f.clause_value.shape == (9, 0)
    assert f.term_trees.tolist() == [0] * 8 and f.table() == []
    # edges without a caller: A at the root (tree 4's root has group -1); D in tree 7, whose caller has group -1
    f = hand([clause("edge", 1, 1, term=0, group=A, caller=-1), clause("edge", 1, None, term=1, group=D, caller=-1)])
    assert f.clause_value.T.tolist() == [[1, 1, 1, 1, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 0, 1, 0]]
    assert f.clause_trees.tolist() == [6, 1] and f.tree_match.tolist() == [1, 1, 1, 1, 0, 0, 0, 1, 1]
    # eligibility: with every tree eligible the fragment of B alone (tree 6) matches, among the whole traces it does not
    every, whole = (hand([clause("group", 1, None, group=B)], need=need) for need in (0, W))
    assert every.clause_value[:, 0].tolist() == whole.clause_value[:, 0].tolist() == [1, 1, 1, 1, 0, 0, 1, 0, 1]
    assert every.tree_match.tolist() == [1, 1, 1, 1, 0, 0, 1, 0, 1] and every.summary[:2].tolist() == [9, 6] and every.clause_trees.tolist() == [6]
    assert whole.tree_match.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 1] and whole.summary[:2].tolist() == [7, 5] and whole.clause_trees.tolist() == [5]
    # times: the largest self time among the rows of group A -- the root's, its latency less the one microsecond its calls cover; in tree
    # 4 the client row's own, in tree 5 the absent row's, in tree 6 the client root's
    f = hand([clause("group", 100, None, group=A, metric="self", reduce="max"), clause("group", 3, 3, term=1, group=-1, metric="onpath")])
    assert f.clause_value[:, 0].tolist() == [99, 249, 49, 69, 1, 5, 19, 29, 399] and f.clause_trees.tolist()[0] == 2
    # ... and the rows on the critical path: A, B, D in trees 0 and 8 (profiles' test has the walk), with their two calls five rows
    assert f.clause_value[[0, 8], 1].tolist() == [5, 5]
    for bad in ([clause("group", group=4)], [clause("edge", group=-1)], [clause("edge", group=A, caller=-2)], [clause("group", group=A, metric="count", reduce="min")],
                [clause("edge", group=A, metric="self")], [clause("latency", 2, 1)], [clause("latency", term=8)], [clause("latency")] * 17):
        with pytest.raises(ValueError):
            hand(bad)


# ---- 2. device = restatement ----------------------------------------------------------------------------------------------------
def pick_groups(link, kind, group, G):
    """What the fixed queries name: the group with the most server rows, one with the fewest (some tree lacks it), and the most
    frequent caller -> callee edge among the server rows."""
    link, kind, group = np.asarray(link), np.asarray(kind), np.asarray(group)
    server = np.flatnonzero((kind == 1) & (group >= 0))
    count = np.bincount(group[server], minlength=G)
    edges = {}
    for r in server.tolist():
        p = link[r]
        while p >= 0 and kind[p] != 1:
            p = link[p]
        if p >= 0:
            e = (int(group[p]), int(group[r]))
            edges[e] = edges.get(e, 0) + 1
    edge = min(edges, key=lambda e: (-edges[e], e)) if edges else (-1, int(np.argmax(count)))
    return int(np.argmax(count)), int(np.argmin(np.where(count > 0, count, count.max() + 1))), edge


def templates(ga, gb, edge):
    """The clauses of the fixed queries, bounds open: name -> keyword arguments of clause()."""
    return {"latency": dict(subject="latency"), "rows": dict(subject="rows"), "start": dict(subject="start"), "class": dict(subject="class"),
            "span_sum": dict(subject="group", group=ga, metric="span"), "self_min": dict(subject="group", group=gb, metric="self", reduce="min"),
            "path_max": dict(subject="group", group=-1, metric="path", reduce="max"), "count": dict(subject="group", group=gb),
            "onpath": dict(subject="group", group=ga, metric="onpath"), "span_max": dict(subject="group", group=gb, metric="span", reduce="max"),
            "edge": dict(subject="edge", group=edge[1], caller=edge[0]), "edge_span": dict(subject="edge", group=edge[1], caller=edge[0], metric="span", reduce="max")}


# name -> [(template, side, term)]: side ">=" / "<=" the median of the template's value over the eligible trees, "!" = the first, negated
QUERIES = {
    "latency": [("latency", ">=", 0)], "rows": [("rows", ">=", 0)], "start": [("start", ">=", 0)], "class": [("class", "<=", 0)],
    "group": [("span_sum", ">=", 0)], "edge": [("edge", ">=", 0)], "min": [("self_min", ">=", 0)], "negated": [("path_max", "!", 0)],
    "term": [("latency", ">=", 0), ("count", ">=", 0)], "two terms": [("latency", ">=", 0), ("span_sum", "<=", 1)],
    "all": [("latency", ">=", 0), ("span_sum", ">=", 0), ("rows", "<=", 1), ("self_min", ">=", 1), ("start", ">=", 2), ("path_max", "<=", 2),
            ("class", "<=", 3), ("count", ">=", 3), ("onpath", ">=", 4), ("edge", ">=", 4), ("span_max", "!", 5), ("edge_span", ">=", 5),
            ("latency", "<=", 6), ("onpath", "<=", 6), ("rows", ">=", 7), ("count", "<=", 7)],
}
assert len(QUERIES["all"]) == traces.FILTER_MAX_CLAUSES and {t for _, _, t in QUERIES["all"]} == set(range(traces.FILTER_MAX_TERMS))


def build_queries(host, tpl, eligible):
    """QUERIES with their thresholds: host(clauses) = filter_host on this forest; every threshold is the median over the eligible trees
    of the clause's value as filter_host gives it with the bounds open (lo = INT64_MIN)."""
    names = sorted(tpl)
    values = host([clause(term=0, **tpl[k]) for k in names]).clause_value
    median = {}
    for j, k in enumerate(names):
        v = values[eligible, j]
        v = v[v != NV]
        median[k] = int(np.sort(v)[len(v) // 2]) if len(v) else 0
    out = {}
    for name, parts in QUERIES.items():
        out[name] = [clause(term=term, lo=median[k] if side != "<=" else None, hi=median[k] if side == "<=" else None, negate=side == "!", **tpl[k])
                     for k, side, term in parts]
    return out


def note(seen, name, f, case, eligible):
    if name in ("latency", "rows", "group") and 0 < f.n_matched < f.n_eligible:
        seen.setdefault("mixed", set()).add((case, name))
    used = sorted({c[0] for c in f.clauses})
    if (f.clause_value[eligible] == NV).any():
        seen["no value"] = True
    for k in used:
        if all(f.term_trees[k] < f.clause_trees[j] for j, c in enumerate(f.clauses) if c[0] == k) and sum(c[0] == k for c in f.clauses) > 1:
            seen["term below its clauses"] = True
    if len(used) == 2 and f.n_matched > max(int(f.term_trees[k]) for k in used):
        seen["union above its terms"] = True


def check_forest(eng, st, link, rows, groupings, flag_queries, seen, case, tag):
    """The fixed queries on the forest last stitched, for every grouping and flag query, against the restatement."""
    kind, start, end = rows[3], np.asarray(rows[4]), np.asarray(rows[5])
    if len(np.unique(np.diff(st.tree_off))) > 1:
        seen.setdefault("rows vary", set()).add(case)
    for group, G in groupings:
        eng.set_row_groups(group, G)
        eng.attribute()                                           # (the times every clause on them reads; need_flags = WHOLE: it stays)
        attr_host = traces.attribute_host(st, link, start, end, group, G)
        tpl = templates(*pick_groups(link, kind, group, G))
        for need, skip in flag_queries:
            eng.signatures("edges", need, skip)                   # (the classes a class clause reads)
            sig_host = traces.signatures_host(st, link, kind, group, G, "edges", need, skip)
            host = lambda clauses: traces.filter_host(st, link, kind, start, end, group, G, clauses, need, skip, attribution=attr_host, signatures=sig_host)
            flags = np.asarray(st.tree_flags).astype(np.int64)
            eligible = ((flags & need) == need) & ((flags & skip) == 0)
            for name, clauses in build_queries(host, tpl, eligible).items():
                dev = eng.filter_traces(clauses, need, skip)
                same(dev, host(clauses), (tag, G, need, skip, name))
                note(seen, name, dev, case, eligible)
    t = eng.filter_timing()
    assert list(t) == ["trees", "list", "copies"] and all(v >= 0 for v in t.values())


def groupings_of(table, rows):
    g = traces.groups_from_table(table)
    return [(g[0], len(g[1])), tg.blind_groups(rows)]


def run_case(lib, tmp_path, name, seed, n, concurrency, expect, seen):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    arrays = [u.arrays for u in units]
    par = [r["parent"] for r in eng.results(2, fields=("parent",))]
    check_forest(eng, eng.stitch(), ta.links_of(arrays, par, rows), rows, groupings_of(table, rows), tg.FLAG_QUERIES, seen, name, (name, "pass 2"))
    check_forest(eng, eng.stitch(truth=True), ta.links_of(arrays, [u.true_parent for u in units], rows), rows, groupings_of(table, rows), tg.FLAG_QUERIES, seen,
                 name, (name, "truth"))
    eng.close()


def test_device_equals_host_restatement(emu_lib, tmp_path):
    seen = {}
    for c in tg.CASES:
        run_case(emu_lib, tmp_path, *c, seen=seen)
    # what the test is about occurred: in every case a query with matched and unmatched eligible trees for the latency and a group
    # clause, and for the rows wherever a query on them can part the trees -- every tree of the hotel and of the alibaba corpus, in the
    # pass-2 and in the true forest, has the same number of rows (11 and 13: one call graph, no fragments), so no bound on the rows
    # has both sides there; a clause without a value; a term that holds on fewer trees than each of its clauses; two terms whose
    # union is larger than either
    assert seen.get("rows vary") == {"media", "fanout"}, seen
    assert seen.get("mixed") == {(c[0], k) for c in tg.CASES for k in ("latency", "group")} | {(c, "rows") for c in seen["rows vary"]}, seen
    assert seen.get("no value") and seen.get("term below its clauses") and seen.get("union above its terms"), seen


def truth_engine(lib, tmp_path, name, seed, n, concurrency, expect):
    """The truth forest needs tw_set_truth but no pass: load, set_truth, the row maps, stitch(truth=True)."""
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = Engine(0, lib_path=lib)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    eng.set_span_rows(*rows)
    link = ta.links_of([u.arrays for u in units], [u.true_parent for u in units], rows)
    return eng, eng.stitch(truth=True), link, rows, groupings_of(table, rows)


GPU_CASE = tg.CASES[3]
assert GPU_CASE[:4] == ("fanout", 9, 300, 25.0)


def run_truth_forest(lib, tmp_path):
    """Parts 2 and 4 on the truth forest of one case, both groupings, the flag query (1, 0)."""
    eng, st, link, rows, groupings = truth_engine(lib, tmp_path, *GPU_CASE)
    seen = {}
    check_forest(eng, st, link, rows, groupings, ((1, 0),), seen, "fanout", ("fanout", "truth"))
    assert seen.get("mixed") and ("fanout", "latency") in seen["mixed"] and seen.get("no value") and seen.get("union above its terms"), seen
    run_reach(eng, st, link, rows, *groupings[0])
    eng.close()


@pytest.mark.gpu
def test_truth_forest_gpu(tmp_path):
    run_truth_forest(None, tmp_path)


def test_truth_forest_without_a_pass(emu_lib, tmp_path):
    run_truth_forest(emu_lib, tmp_path)


# ---- 3. sizes and routes ----------------------------------------------------------------------------------------------------------
def run_table(lib, table, queries, tag):
    eng, st, link, rows, group, G = tp.table_engine(lib, table)
    kind, start, end = rows[3], np.asarray(rows[4]), np.asarray(rows[5])
    eng.attribute()
    attr_host = traces.attribute_host(st, link, start, end, group, G)
    out = []
    for name, clauses in queries:
        dev = eng.filter_traces(clauses, 1, 0)
        same(dev, traces.filter_host(st, link, kind, start, end, group, G, clauses, 1, 0, attribution=attr_host), (tag, name))
        out.append(dev)
    eng.close()
    return st, out


def run_sizes(lib):
    """sized_table of tests/test_signatures.py: trees of 0, 1, 63, 64, 65, 300 and 600 items (two rows more each), either side of a
    wavefront and of kFiltCap in either build (12 / 256); tree 7: 300 rows of one group.  Group 3 occurs in trees 2 .. 6 only."""
    queries = [("sum", [clause("group", 1000, None, group=3, metric="span")]), ("min", [clause("group", 10, None, group=3, metric="span", reduce="min")]),
               ("max", [clause("group", None, 480, group=7, metric="self", reduce="max")]), ("edge", [clause("edge", 2, 100, group=5, caller=-1)]),
               ("all four", [clause("group", 1000, None, term=0, group=3, metric="span"), clause("group", 10, None, term=0, group=3, metric="span", reduce="min"),
                             clause("group", None, 480, term=1, group=7, metric="self", reduce="max"), clause("edge", 2, 100, term=2, group=5, caller=-1),
                             clause("group", 3, None, term=2, group=-1, metric="onpath")])]
    st, out = run_table(lib, tg.sized_table(), queries, "sizes")
    n_trees = len(tg.SIZES) + 1 + tg.N_DISTINCT
    assert st.n_trees == n_trees and np.diff(st.tree_off)[:8].tolist() == [k + 2 for k in tg.SIZES] + [302]
    by = dict(zip([q[0] for q in queries], out))
    assert (by["min"].clause_value[:2, 0] == NV).all() and (by["min"].clause_value[2:7, 0] != NV).all() and (by["min"].clause_value[7:, 0] == NV).all()
    # the items of trees 0 .. 6 hang under a request row without a group: their caller is -1; items j with (5 j + i) % 7 == 5
    assert by["edge"].clause_value[:7, 0].tolist() == [sum(1 for j in range(k) if (j * 5 + i) % 7 == 5) for i, k in enumerate(tg.SIZES)]
    assert 0 < by["sum"].n_matched < by["sum"].n_eligible and 0 < by["edge"].n_matched < n_trees
    assert by["max"].clause_value[7, 0] != NV and (np.delete(by["max"].clause_value[:, 0], 7) == NV).all()       # tree 7 alone has rows of group 7


def run_wide(lib, n_pairs=tp.N_PAIRS):
    """wide_table of tests/test_profiles.py: trees of three rows, so that the lanes of a wavefront share the tree slots (two lanes and
    more meet on one cell) and a lane's tree changes from position to position."""
    u, tp_, rows, group, G = tp.wide_table(n_pairs)
    dur = np.maximum(np.asarray(rows[5]) - np.asarray(rows[4]), 0)
    mid = int(np.median(dur[2 * 2 * n_pairs:]))                    # the callee rows' durations
    queries = [("sum", [clause("group", 900 + mid, None, group=-1, metric="span")]), ("min", [clause("group", mid, None, group=-1, metric="span", reduce="min")]),
               ("max", [clause("group", None, 300, group=-1, metric="path", reduce="max")]), ("edge", [clause("edge", mid, None, group=20, caller=0, metric="span", reduce="max")]),
               ("rows", [clause("group", 2, 2, group=-1), clause("group", 2, 2, group=-1, metric="onpath"), clause("rows", 3, 3)])]
    st, out = run_table(lib, (u, tp_, rows, group, G), queries, "wide")
    assert st.n_trees == 2 * n_pairs and (np.diff(st.tree_off) == 3).all()
    by = dict(zip([q[0] for q in queries], out))
    assert 0 < by["sum"].n_matched < 2 * n_pairs and 0 < by["min"].n_matched < 2 * n_pairs and by["rows"].n_matched == 2 * n_pairs
    assert np.flatnonzero(by["edge"].clause_value[:, 0] != NV).tolist() == [0, 1]  # the edge 0 > 20 is pair 0's alone: its two trees


def test_sizes_and_routes(emu_lib):
    run_sizes(emu_lib)
    run_wide(emu_lib)


@pytest.mark.gpu
def test_sizes_and_routes_gpu():
    run_sizes(None)
    run_wide(None)


def test_sizes_lane_threaded(emu_lib):
    """One host thread per lane (TW_EMU_LANES=1, workgroups of 256): the LDS atomics, ballots and shuffles of k_filt_trees run as they
    are written, 64 lanes to a wavefront and four wavefronts to a workgroup, without a GPU."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "import test_filter as t\n"
            "t.run_sizes(%r)\n"
            "t.run_wide(%r, 16)\n"
            "print('child ok')\n") % (os.path.dirname(here), here, emu_lib, emu_lib)
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stderr[-2000:]


# ---- 4. the bit reaches every stage -------------------------------------------------------------------------------------------------
def run_reach(eng, st, link, rows, group, G):
    kind, start, end = rows[3], np.asarray(rows[4]), np.asarray(rows[5])
    eng.set_row_groups(group, G)
    before = eng.attribute(0.5, need_flags=W)
    attr_host = traces.attribute_host(st, link, start, end, group, G)
    ga, gb, edge = pick_groups(link, kind, group, G)
    open_ = traces.filter_host(st, link, kind, start, end, group, G, [clause("latency"), clause("group", group=ga, metric="self")], 1, 0, attribution=attr_host)
    whole = (np.asarray(st.tree_flags) & W) != 0
    mid = [int(np.sort(open_.clause_value[whole, j])[whole.sum() // 2]) for j in range(2)]
    clauses = [clause("latency", mid[0], None, term=0), clause("group", mid[1], None, term=1, group=ga, metric="self")]
    f = eng.filter_traces(clauses, 1, 0)
    same(f, traces.filter_host(st, link, kind, start, end, group, G, clauses, 1, 0, attribution=attr_host), "reach")
    assert 0 < f.n_matched < f.n_eligible
    marked = with_match(st, f)
    assert eng.attribute(0.5, need_flags=W).same_as(before)       # a stage that does not name the bit answers what it answered
    for pct in (0.0, 0.5):
        a = eng.attribute(pct, need_flags=W | M, skip_flags=0)
        want = traces.attribute_host(marked, link, start, end, group, G, pct, need_flags=W | M, skip_flags=0)
        assert a.same_as(want) and a.summary[0] == f.n_matched
        d, d_want = eng.distributions((0.5, 0.9)), traces.distributions_host(marked, want, start, end, group, G, None, 1, (0.5, 0.9), None)
        assert all(np.array_equal(getattr(d, k), getattr(d_want, k)) for k in traces.LatencyDistributions.FIELDS)
        for mode in (0, 1):
            s = eng.signatures(mode, W | M, 0)
            s_want = traces.signatures_host(marked, link, kind, group, G, mode, W | M, 0)
            tg.same(s, s_want, ("reach", mode))
            assert s.n_eligible == f.n_matched
            tp.same(eng.class_profiles(), traces.class_profiles_host(marked, s_want, want, link, kind, start, end, group), ("reach", mode))


def test_the_bit_reaches_every_stage(emu_lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, emu_lib, "media", 7, 300, 6.0)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(emu_lib, units, n_traces, rows)
    par = [r["parent"] for r in eng.results(2, fields=("parent",))]
    group, names = traces.groups_from_table(table)
    run_reach(eng, eng.stitch(), ta.links_of([u.arrays for u in units], par, rows), rows, group, len(names))
    eng.close()


# ---- 5. residency and refusals ------------------------------------------------------------------------------------------------------
def refused(code, call, *args, **kw):
    with pytest.raises(EngineError) as ex:
        call(*args, **kw)
    assert ex.value.code == code and {-1: "TW_ERR_ARG", -4: "TW_ERR_STATE"}[code] in str(ex.value), str(ex.value)


def run_residency(lib):
    eng, st, link, rows, group, G = tp.table_engine(lib, tp.wide_table(16))
    kind, start, end = rows[3], np.asarray(rows[4]), np.asarray(rows[5])
    nt = st.n_trees
    callee = (np.maximum(end, start) - start)[2 * nt:]              # tree t's callee row: distinct durations, the shortest row of its tree
    least = lambda lo, hi: [clause("group", lo, hi, group=-1, metric="span", reduce="min")]
    slow = least(int(np.median(callee)) + 1, None)
    on_self = [clause("group", 1, None, group=-1, metric="self")]
    selected_by_bit = lambda: eng.signatures(0, W | M, 0).tree_class >= 0
    # a class clause before any signatures call; a clause on times before an attribution: refused, and the bit stays what it was
    refused(-4, eng.filter_traces, [clause("class", 0, 0)])
    f = eng.filter_traces(slow)
    assert 0 < f.n_matched < nt and np.array_equal(selected_by_bit(), f.tree_match != 0)
    for metric in ("self", "path", "onpath"):
        refused(-4, eng.filter_traces, [clause("latency"), clause("group", group=0, metric=metric)])
    assert np.array_equal(selected_by_bit(), f.tree_match != 0)
    assert np.array_equal(eng.attribute(need_flags=W | M).tree_selected, f.tree_match)
    # an attribution whose query named the bit is dropped by the next filter call, one that did not name it is not
    eng.signatures(0, W, 0)
    first = eng.class_profiles()
    g = eng.filter_traces(on_self)                                # (reads the attribution, then drops it)
    same(g, traces.filter_host(st, link, kind, start, end, group, G, on_self, attribution=traces.attribute_host(st, link, start, end, group, G)), "read, then dropped")
    refused(-4, eng.class_profiles)
    refused(-4, eng.filter_traces, on_self)
    eng.attribute(need_flags=W)
    kept = eng.class_profiles()
    eng.filter_traces(slow)
    assert eng.class_profiles().same_as(kept) and eng.filter_traces(on_self).n_matched == g.n_matched
    assert eng.class_profiles().same_as(kept)
    # ... and the same for the signature result
    eng.signatures(0, W | M, 0)
    eng.class_profiles()
    eng.filter_traces(slow)
    refused(-4, eng.class_profiles)
    refused(-4, eng.filter_traces, [clause("class", 0, 0)])
    eng.signatures(0, W, 0)
    assert eng.filter_traces([clause("class", 0, 0)]).n_matched == 2                # (a pair of trees per class)
    # a query may name the bit itself: the last match, narrowed
    h = eng.filter_traces(slow)
    again = eng.filter_traces(least(None, int(np.sort(callee)[-3])), W | M, 0)
    assert again.n_eligible == h.n_matched and again.n_matched == h.n_matched - 2
    # a new stitch makes a new forest without the bit, and its flags never show it
    st2 = eng.stitch(0)
    assert np.array_equal(st2.tree_flags, st.tree_flags) and (st2.tree_flags & M == 0).all()
    a = eng.attribute(need_flags=W | M)
    assert a.summary[0] == 0 and not a.tree_selected.any()
    # every argument error; a refused call changes nothing
    f = eng.filter_traces(slow)
    ok = clause("group", group=0)
    edge = clause("edge", group=0, caller=0)
    swap = lambda c, **kw: tuple(kw.get(k, v) for k, v in zip(("term", "subject", "group", "caller", "metric", "reduce", "negate", "lo", "hi"), c))
    for bad in ([clause("latency")] * 17, [swap(ok, term=-1)], [swap(ok, term=8)], [swap(ok, subject=-1)], [swap(ok, subject=6)], [swap(ok, metric=-1)],
                [swap(ok, metric=5)], [swap(edge, metric=2)], [swap(ok, reduce=-1)], [swap(ok, reduce=3)], [swap(ok, group=-2)], [swap(ok, group=G)],
                [swap(edge, group=-1)], [swap(edge, group=G)], [swap(edge, caller=-2)], [swap(edge, caller=G)], [swap(ok, lo=2, hi=1)],
                [swap(ok, metric=0, reduce=1)], [swap(ok, metric=4, reduce=2)], [clause("latency"), swap(ok, lo=1, hi=0)]):
        refused(-1, eng.filter_traces, bad)
    import ctypes
    from traceweaver_amd import _ffi
    q = _ffi.FilterQuery(1, 0, -1, None)
    assert eng._lib.tw_filter_traces(eng._h, ctypes.byref(q), None, None) == -1
    assert np.array_equal(eng.attribute(need_flags=W | M).tree_selected, f.tree_match)
    eng.close()


def test_residency_and_refusals(emu_lib):
    run_residency(emu_lib)
    # before a stitch, before the row groups
    u, tp_, rows, group, G = tp.wide_table(4)
    eng = Engine(0, lib_path=emu_lib)
    eng.load([u])
    refused(-4, eng.filter_traces, [])
    eng.set_span_rows(*rows)
    eng.set_parents([tp_])
    eng.stitch(0)
    refused(-4, eng.filter_traces, [])
    eng.set_row_groups(group, G)
    assert eng.filter_traces([]).n_matched == 8                   # (new groups leave the forest)
    eng.close()


@pytest.mark.gpu
def test_residency_and_refusals_gpu():
    run_residency(None)   # (all refused on the host: nothing malformed reaches the device)


def test_score_traces_keeps_the_bit(emu_lib, tmp_path):
    """A forest of a pass (score_traces refuses any other): the CONFIDENT bit is rewritten, the MATCH bit stays."""
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, emu_lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table)
    eng = ts.solve(emu_lib, units, n_traces, rows)
    eng.set_row_groups(group, len(names))
    st = eng.stitch()
    f = eng.filter_traces([clause("latency", int(np.median(st.tree_latency)), None)])
    assert 0 < f.n_matched < f.n_eligible
    conf = eng.score_traces(0.0)
    assert np.array_equal(eng.attribute(need_flags=W | M).tree_selected, f.tree_match)
    both = eng.attribute(need_flags=W | M | traces.CONFIDENT).tree_selected
    assert np.array_equal(both, f.tree_match & (conf.tree_confident != 0))
    eng.filter_traces([])                                         # ... and the filter keeps the CONFIDENT bit
    assert np.array_equal(eng.attribute(need_flags=W | traces.CONFIDENT, skip_flags=0).tree_selected, ((st.tree_flags & W) != 0) & (conf.tree_confident != 0))
    eng.close()


# ---- 6. the command line's language -------------------------------------------------------------------------------------------------
NAMES = ["frontend", "search", "profile", "cache-svc"]


def test_parse_filter():
    p = lambda e: traces.parse_filter(e, NAMES)
    assert p("latency>=20000") == [clause("latency", 20000, None)] and p("rows <= 7") == [clause("rows", None, 7)]
    assert p("start==5") == [clause("start", 5, 5)] and p("class in 2..4") == [clause("class", 2, 4)] and p("!latency>=-3") == [clause("latency", -3, None, negate=True)]
    for k, metric in enumerate(traces.FILTER_METRICS):
        assert p("%s[search]>=1" % metric) == [clause("group", 1, None, group=1, metric=k)]
    assert p("span.min[profile]<=9") == [clause("group", None, 9, group=2, metric="span", reduce="min")]
    assert p("self.max[*]>=5000") == [clause("group", 5000, None, group=-1, metric="self", reduce="max")]
    assert p("path.sum[cache-svc] in 1..2") == [clause("group", 1, 2, group=3, metric="path")]
    assert p("count[frontend>profile]>=1") == [clause("edge", 1, None, group=2, caller=0)]
    assert p("span.max[->frontend]>=1") == [clause("edge", 1, None, group=0, caller=-1, metric="span", reduce="max")]
    e = "latency>=20000 & !count[cache-svc]>=1 | span.max[search]>=5000 | count[frontend>profile]==1 & self.min[*] in 3..9"
    c = p(e)
    assert [x[0] for x in c] == [0, 0, 1, 2, 2] and c[1] == clause("group", 1, None, group=3, negate=True) and c[3] == clause("edge", 1, 1, term=2, group=2, caller=0)
    assert traces.format_filter(c, NAMES) == e and p(traces.format_filter(c, NAMES)) == c      # the round trip
    every = [clause(s, 1, 2, term=k % 8, group=1, caller=-1 + k % 3, metric=m, reduce=r, negate=k % 2) for k, (s, m, r) in enumerate(
        [("latency", 0, 0), ("rows", 0, 0), ("start", 0, 0), ("class", 0, 0), ("group", 0, 0), ("group", 1, 1), ("group", 2, 2), ("group", 3, 0), ("group", 4, 0),
         ("edge", 0, 0), ("edge", 1, 2)])]
    every = [c[:2] + ((-1, -1, 0, 0) if c[1] < 4 else (c[2], c[3] if c[1] == 5 else -1, c[4], c[5])) + c[6:] for c in every]
    assert sorted(p(traces.format_filter(every, NAMES))) == sorted(every)
    assert len(p(" | ".join(["rows>=1"] * 8))) == 8 and len(p(" & ".join(["rows>=1"] * 16))) == 16
    for bad, piece in ((" | ".join(["rows>=1"] * 8 + ["start>=77"]), "start>=77"), (" & ".join(["rows>=1"] * 16 + ["start>=78"]), "start>=78"),
                       ("count[nosuch]>=1", "nosuch"), ("count[nosuch>search]>=1", "nosuch"), ("count[search>nosuch]>=1", "nosuch"), ("depth>=1", "depth"),
                       ("width[search]>=1", "width"), ("span.mean[search]>=1", "mean"), ("count.max[search]>=1", "count.max[search]>=1"),
                       ("self[frontend>search]>=1", "self"), ("latency>=fast", "fast"), ("latency in 5..1", "latency in 5..1"), ("latency", "latency"),
                       ("latency>=1 &", "''")):
        with pytest.raises(ValueError) as ex:
            p(bad)
        assert piece in str(ex.value), (bad, str(ex.value))


# ---- 7. the command line ------------------------------------------------------------------------------------------------------------
def test_cli_trace_filter(emu_lib, reference_root, tmp_path, capsys):
    """--trace_filter / --filter_out on a shipped corpus (hotel_load100, the corpus of tests/test_executor_cli.py): the files equal what
    the same Engine calls give, made by hand in the order the run makes them on the assignment the run's --attribute_out file holds.
    Without the option there is no filter file, and the latency file is the one a filter that every whole trace matches gives."""
    from traceweaver_amd import executor
    from traceweaver_amd.ingest import REFERENCE_FIX, open_directory

    rel = "data/hotel_reservation/hotel_load100/"
    base = ["--relative_path", rel, "--cache_rate", "0", "--fix", "2", "--test_name", "f", "--load_level", "100", "--predictor_indices", "10",
            "--project_root", reference_root, "--engine_library", emu_lib]
    first_span, fix = REFERENCE_FIX[2]
    corpus, _ = open_directory(os.path.join(reference_root, rel), lib_path=emu_lib, first_span=first_span, fix=fix, max_traces=1001)
    units, skipped, n_traces = corpus.units()
    table = corpus.span_table()
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table, corpus)
    names = [str(x) for x in names]
    S = names.index("search")
    dur = np.maximum(np.asarray(rows[5]) - np.asarray(rows[4]), 0)
    T = int(np.median(dur[(np.asarray(rows[2]) == -1) & (np.asarray(rows[3]) == 1)]))          # the root spans' durations
    U = int(np.median(dur[(group == S) & (np.asarray(rows[3]) == 1)]))
    expr = "latency>=%d & span.max[search]>=%d" % (T, U)
    files = lambda tag: {k: str(tmp_path / ("%s_%s.npz" % (tag, k))) for k in ("latency", "profiles", "filter", "attr")}
    runs = {"plain": ["--latency_out", files("plain")["latency"], "--attribute_out", files("plain")["attr"]],
            "every": ["--trace_filter", "rows>=0", "--latency_out", files("every")["latency"]],
            "some": ["--trace_filter", expr, "--latency_out", files("some")["latency"], "--profiles_out", files("some")["profiles"],
                     "--filter_out", files("some")["filter"]]}
    text, pickles = {}, {}
    for tag, extra in runs.items():
        out = str(tmp_path / tag) + "/"
        executor.main(base + ["--results_directory", out] + extra)
        text[tag] = capsys.readouterr().out
        pickles[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
    assert len(pickles["plain"]) == 5 and pickles["plain"] == pickles["every"] == pickles["some"]
    assert not os.path.exists(files("plain")["filter"]) and not os.path.exists(files("every")["filter"]) and "Trace filter" not in text["plain"]
    plain, every, some = (np.load(files(tag)["latency"]) for tag in ("plain", "every", "some"))
    assert sorted(plain.files) == sorted(every.files) and all(np.array_equal(plain[k], every[k]) for k in plain.files)
    assert not np.array_equal(plain["seg_count"], some["seg_count"])
    # the run's parent arrays, read off the links of its attribution file
    link = np.load(files("plain")["attr"])["link"]
    par = []
    for u in units:
        request = {int(r): i for i, r in enumerate(u.in_rows)}
        p = np.full((u.arrays.E, u.arrays.n_in), -1, dtype=np.int32)
        for e, per in enumerate(u.out_rows):
            for x, r in enumerate(per):
                if link[r] >= 0:
                    p[e, request[int(link[r])]] = x
        par.append(p)
    clauses = traces.parse_filter(expr, names)
    assert clauses == [clause("latency", T, None), clause("group", U, None, group=S, metric="span", reduce="max")]
    eng = Engine(0, lib_path=emu_lib)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    eng.set_span_rows(*rows)
    eng.set_parents(par)
    eng.set_row_groups(group, len(names))
    st = eng.stitch(0)
    eng.attribute(0.95)
    d0 = eng.distributions((0.5, 0.95, 0.99))
    assert all(np.array_equal(plain[k], getattr(d0, k)) for k in traces.LatencyDistributions.FIELDS)       # without the option: what it was
    f = eng.filter_traces(clauses)
    assert 0 < f.n_matched < f.n_eligible
    same(f, traces.filter_host(st, link, rows[3], rows[4], rows[5], group, len(names), clauses), "cli")
    z = np.load(files("some")["filter"])
    for k in traces.TraceFilter.FIELDS:
        assert np.array_equal(z[k], getattr(f, k)) and z[k].dtype == getattr(f, k).dtype, k
    assert str(z["expression"]) == expr and z["clauses"].tolist() == [list(c) for c in clauses] and z["group_names"].tolist() == names
    a = eng.attribute(0.95, need_flags=W | M)
    assert a.summary[0] == f.n_matched
    d = eng.distributions((0.5, 0.95, 0.99))
    assert all(np.array_equal(some[k], getattr(d, k)) for k in traces.LatencyDistributions.FIELDS)
    sides = []
    for truth in (True, False):
        if truth:
            eng.stitch(truth=True)
        else:
            eng.stitch(0)
        eng.filter_traces(clauses)
        eng.signatures("levels", need_flags=W | M)
        eng.attribute(0.95, need_flags=W | M)
        sides.append(eng.class_profiles())
    eng.close()
    p = np.load(files("some")["profiles"])
    for prefix, want in (("true_", sides[0]), ("", sides[1])):
        for k in traces.ClassProfiles.FIELDS + ("class_off", "class_entries"):
            assert np.array_equal(p[prefix + k], getattr(want, k)), prefix + k
    assert sides[1].summary[0] + sides[1].summary[4] == f.n_matched     # the classed trees are the matched ones
    assert "Trace filter: %d of %d whole traces match %s" % (f.n_matched, f.n_eligible, expr) in text["some"].splitlines()
    bad = [x for x in base if x not in ("--cache_rate", "0", "--predictor_indices", "10")] + ["--results_directory", str(tmp_path) + "/"]
    for extra in (["--cache_rate", "0.1", "--predictor_indices", "10", "--trace_filter", "rows>=0"], ["--cache_rate", "0", "--predictor_indices", "3", "--trace_filter", "rows>=0"],
                  ["--cache_rate", "0", "--predictor_indices", "10", "--filter_out", "f.npz"], ["--cache_rate", "0", "--predictor_indices", "10", "--trace_filter", "count[nosuch]>=1"]):
        with pytest.raises(SystemExit):
            executor.main(bad + extra)
