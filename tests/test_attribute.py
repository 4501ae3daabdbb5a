"""Engine.attribute (tw_attribute_traces, csrc/tw_attr.h): self times, critical paths and the delay-culprit query on the
stitched forest.  The yardstick is traces.attribute_host, the definitions of include/traceweaver_amd.h restated in recursive
Python; part 1 checks it on forests written out by hand, the rest compares the device with it, np.array_equal on every
output.  Corpora and cases are those of tests/test_stitch.py.  CPU tier: host-emulation build (tiny tables: the packed, the
single-tree and the global-memory route of k_attr_tree all occur, and both routes of k_attr_reduce); the HIP library under
-m gpu."""
import os

import numpy as np
import pytest

import test_stitch as ts
from traceweaver_amd import synth, traces
from traceweaver_amd.engine import Engine, EngineError

W, U = traces.WHOLE, traces.UNASSIGNED


# ---- 1. the restatement on forests written out by hand --------------------------------------------------------------------
def forest(rows, flags=None):
    """rows: (start, end, link) per row -> (StitchedTraces as the stitch would give it, link, start, end).  flags: per root row."""
    start = np.array([r[0] for r in rows], dtype=np.int64)
    end = np.array([r[1] for r in rows], dtype=np.int64)
    link = np.array([r[2] for r in rows], dtype=np.int32)
    n = len(rows)
    root = np.arange(n)
    depth = np.zeros(n, dtype=np.int32)
    for r in range(n):
        x = r
        while link[x] >= 0:
            x = link[x]
            depth[r] += 1
        root[r] = x
    order = np.lexsort((np.arange(n), start, root))
    tree_root = np.unique(root)
    tree_off = np.concatenate([[0], np.cumsum(np.bincount(root, minlength=n)[tree_root])]).astype(np.int64)
    latency = np.array([end[root == r].max() - start[r] for r in tree_root], dtype=np.int64)
    fl = np.array([W if flags is None else flags[int(r)] for r in tree_root], dtype=np.uint8)
    st = traces.StitchedTraces(root.astype(np.int32), depth, tree_off, order.astype(np.int32), tree_root.astype(np.int32), latency, fl, [0, 0, 0, -1])
    return st, link, start, end


def host(rows, group=None, n_groups=1, flags=None, **query):
    st, link, start, end = forest(rows, flags)
    group = np.zeros(len(rows), dtype=np.int32) if group is None else np.asarray(group, dtype=np.int32)
    return traces.attribute_host(st, link, start, end, group, n_groups, **query), st


def test_host_sequential_chain():
    a, _ = host([(0, 100, -1), (10, 30, 0), (40, 70, 0), (80, 90, 0)])
    assert a.self_time.tolist() == [40, 20, 30, 10]
    assert a.path_time.tolist() == [40, 20, 30, 10]              # every gap between the calls is the root's own
    assert a.tree_path_rows.tolist() == [4] and a.tree_top_group.tolist() == [0]


def test_host_parallel_fan_out():
    # 1 [10, 90] holds 2 [20, 50] in time, 3 [85, 95] overlaps 1, 4 [96, 99] is disjoint; 5 is a call of 1
    rows = [(0, 100, -1), (10, 90, 0), (20, 50, 0), (85, 95, 0), (96, 99, 0), (30, 60, 1)]
    a, _ = host(rows, group=[0, 1, 1, 2, -1, 2], n_groups=3)
    assert a.self_time.tolist() == [12, 50, 30, 10, 3, 30]       # root: 100 less [10, 95] and [96, 99]
    # 4 with [96, 99], 3 with [85, 95], 1 with [10, 85] (5 with [30, 60] inside); 2 starts after the cursor has passed: never walked
    assert a.path_time.tolist() == [12, 45, 0, 10, 3, 30]
    assert a.tree_path_rows.tolist() == [5] and a.tree_top_group.tolist() == [1]
    assert a.group_path_time.tolist() == [12, 45, 40] and a.group_path_rows.tolist() == [1, 1, 2]
    assert a.group_self_time.tolist() == [12, 80, 40] and a.group_span_time.tolist() == [100, 110, 40] and a.group_span_rows.tolist() == [1, 2, 2]
    assert a.group_trees.tolist() == [1, 1, 1] and a.group_top_trees.tolist() == [0, 1, 0]
    assert a.summary.tolist() == [1, 1, 0, 100, 1] and a.culprit == 1 and a.mean_latency(1) == 55.0
    assert [r["group"] for r in a.table(["a", "b", "c"])] == ["a", "b", "c"] and a.table()[1]["path_share"] == 45 / 97


def test_host_child_outside_its_parent():
    a, st = host([(0, 50, -1), (40, 70, 0)])                      # ends after its parent: clipped to [40, 50]
    assert a.self_time.tolist() == [40, 30] and a.path_time.tolist() == [40, 10]
    assert st.tree_latency.tolist() == [70] and a.path_time.sum() == 50   # the path is the root's duration, not the latest end
    a, _ = host([(20, 60, -1), (10, 30, 0)])                      # starts before its parent: clipped to [20, 30]
    assert a.self_time.tolist() == [30, 20] and a.path_time.tolist() == [30, 10]


def test_host_equal_ends():
    a, _ = host([(0, 100, -1), (50, 80, 0), (40, 80, 0), (40, 80, 0)])
    assert a.path_time.tolist() == [60, 0, 40, 0]                 # same end: the earlier start, then the smaller row
    assert a.self_time.tolist() == [60, 30, 40, 40]
    # the cursor clips 2 [20, 90] and 3 [10, 80] to the same end 50: the smaller start wins, although 2 ends later
    a, _ = host([(0, 100, -1), (50, 100, 0), (20, 90, 0), (10, 80, 0)])
    assert a.path_time.tolist() == [10, 50, 0, 40] and a.self_time.tolist() == [10, 50, 70, 70]


def test_host_zero_length_rows():
    a, _ = host([(5, 5, -1), (5, 5, 0), (0, 10, -1), (4, 4, 2), (6, 2, 2)])   # (6, 2): end < start counts as [6, 6]
    assert a.path_time.tolist() == [0, 0, 10, 0, 0] and a.self_time.tolist() == [0, 0, 10, 0, 0]
    assert a.tree_path_rows.tolist() == [1, 1]
    assert a.group_span_time.tolist() == [10] and a.group_span_rows.tolist() == [5]


def test_host_selection_and_fragments():
    # single-row trees: latencies 10, 40, 20, 30 whole; a fragment; a whole trace with an unassigned call
    rows = [(0, 10, -1), (100, 140, -1), (200, 220, -1), (300, 330, -1), (400, 500, -1), (500, 700, -1)]
    flags = {0: W, 1: W, 2: W, 3: W, 4: 0, 5: W | U}
    a, _ = host(rows, flags=flags, percentile=0.5)
    assert a.summary.tolist() == [4, 2, 2, 30, 0] and a.tree_selected.tolist() == [0, 1, 0, 1, 0, 0]
    assert a.path_time.tolist() == [10, 40, 20, 30, 100, 200]     # per-row figures cover every tree, the fragment included
    a, _ = host(rows, flags=flags, percentile=0.5, start_max=250)
    assert a.summary.tolist() == [4, 1, 2, 30, 0] and a.tree_selected.tolist() == [0, 1, 0, 0, 0, 0] and a.group_span_time.tolist() == [40]
    a, _ = host(rows, flags=flags, percentile=0.5, start_min=300, start_max=301)
    assert a.tree_selected.tolist() == [0, 0, 0, 1, 0, 0]         # half-open
    a, _ = host(rows, flags=flags, skip_flags=0)
    assert a.summary.tolist() == [5, 5, 0, 10, 0] and a.tree_selected.tolist() == [1, 1, 1, 1, 0, 1]
    a, _ = host(rows, flags=flags, need_flags=0, skip_flags=0, percentile=0.95)
    assert a.summary.tolist() == [6, 1, 5, 200, 0] and a.tree_selected.tolist() == [0, 0, 0, 0, 0, 1]
    a, _ = host(rows, flags=flags, group=[-1] * 6)
    assert a.culprit == -1 and a.tree_top_group.tolist() == [-1] * 6 and a.n_selected == 4


def test_host_tree_beyond_the_wavefront_tables():
    n = 600                                                       # > kStitchCap = 512
    rows = [(0, 10000, -1)] + [(10 * i + 1, 10 * i + 6, 0) for i in range(n)]
    a, _ = host(rows)
    assert a.self_time.tolist() == [10000 - 5 * n] + [5] * n and a.path_time.tolist() == [10000 - 5 * n] + [5] * n
    assert a.tree_path_rows.tolist() == [n + 1]
    deep = [(0, 2000, -1)] + [(i, 2000 - i, i - 1) for i in range(1, n)]   # a chain 600 deep
    a, _ = host(deep)
    assert a.path_time.tolist() == [2] * (n - 1) + [2000 - 2 * (n - 1)] and np.array_equal(a.path_time, a.self_time)


# ---- 2. / 3. device = restatement, invariants -------------------------------------------------------------------------------
def links_of(unit_arrays, parents, rows):
    """The link table tw_stitch_traces builds (csrc/tw_stitch.h), from the parent arrays."""
    in_rows, out_rows, row_link, row_kind = rows[:4]
    row_link = np.asarray(row_link, dtype=np.int64)
    link = np.where((np.asarray(row_kind) == 1) & (row_link >= 0), row_link, -1)
    for u, p, ir, per in zip(unit_arrays, parents, in_rows, out_rows):
        ir = np.asarray(ir, dtype=np.int64)
        for e in range(u.E):
            x = np.asarray(p[e], dtype=np.int64)
            ok = (x >= 0) & (x < len(per[e]))
            link[np.asarray(per[e], dtype=np.int64)[x[ok]]] = ir[ok]
    return link.astype(np.int32)


def queries(st, start):
    mid = int(np.median(start[st.tree_root]))
    return [dict(), dict(percentile=0.5), dict(percentile=0.95), dict(percentile=0.5, start_max=mid), dict(start_min=mid),
            dict(skip_flags=0), dict(percentile=0.5, need_flags=0, skip_flags=0)]


def check_invariants(a, st, start, end, chain_only=False):
    dur = np.maximum(end, start) - start
    assert np.array_equal(np.add.reduceat(a.path_time[st.tree_rows], st.tree_off[:-1]), dur[st.tree_root])   # a tree's path is its root's duration
    assert np.all(a.self_time >= 0) and np.all(a.self_time <= dur) and np.all(a.path_time >= 0) and np.all(a.path_time <= dur)
    assert np.all(a.tree_path_rows >= 1) and np.all(a.tree_path_rows <= np.diff(st.tree_off))
    sel = a.tree_selected.astype(bool)
    assert int(a.group_top_trees.sum()) == a.n_selected - int((sel & (a.tree_top_group < 0)).sum())
    assert a.n_selected == int(sel.sum()) and a.n_selected <= a.n_eligible - a.rank
    if chain_only:
        assert np.array_equal(a.path_time, a.self_time) and np.array_equal(a.tree_path_rows, np.diff(st.tree_off))


def check_forest(eng, st, link, rows, group, n_groups, chain_only=False, all_queries=True):
    """Every query on the forest last stitched: device = restatement, invariants.  Returns the plain attribution."""
    start, end = np.asarray(rows[4]), np.asarray(rows[5])
    first = None
    for q in queries(st, start) if all_queries else [dict(), dict(percentile=0.5)]:
        dev = eng.attribute(**q)
        want = traces.attribute_host(st, link, start, end, group, n_groups, **q)
        assert np.array_equal(dev.link, link)
        for k in traces.Attribution.FIELDS:
            assert np.array_equal(getattr(dev, k), getattr(want, k)), (k, q)
        check_invariants(dev, st, start, end, chain_only)
        first = dev if first is None else first
    t = eng.attribute_timing()
    assert set(t) == {"tree", "select", "reduce"} and all(v >= 0 for v in t.values())
    return first


def check_both_forests(eng, units, rows, table, par=None, pass_=None, chain_truth=False):
    """The forest of the assignment and the true one; 4. they agree where the forests agree."""
    group, names = traces.groups_from_table(table)
    eng.set_row_groups(group, len(names))
    arrays = [u.arrays for u in units]
    if par is None:
        par = [r["parent"] for r in eng.results(2 if pass_ is None else pass_, fields=("parent",))]
    st = eng.stitch(pass_)
    link = links_of(arrays, par, rows)
    a = check_forest(eng, st, link, rows, group, len(names))
    tt = eng.stitch(truth=True)
    tlink = links_of(arrays, [u.true_parent for u in units], rows)
    b = check_forest(eng, tt, tlink, rows, group, len(names), chain_only=chain_truth)
    # a tree of the assignment all of whose rows have the true links, and to which the truth attaches no further row, is a
    # true tree: every per-row figure is the same
    same = np.ones(st.n_trees, dtype=bool)
    np.logical_and.at(same, np.searchsorted(st.tree_root, st.root), link == tlink)
    k = np.flatnonzero(same)
    at = np.searchsorted(tt.tree_root, st.tree_root[k])
    ok = (at < tt.n_trees) & (tt.tree_root[np.minimum(at, tt.n_trees - 1)] == st.tree_root[k])
    k, at = k[ok], at[ok]
    full = np.diff(st.tree_off)[k] == np.diff(tt.tree_off)[at]
    k, at = k[full], at[full]
    assert len(k) > 0
    r = np.concatenate([st.tree_rows[st.tree_off[i]:st.tree_off[i + 1]] for i in k])
    assert np.array_equal(a.self_time[r], b.self_time[r]) and np.array_equal(a.path_time[r], b.path_time[r])
    assert np.array_equal(a.tree_top_group[k], b.tree_top_group[at]) and np.array_equal(a.tree_path_rows[k], b.tree_path_rows[at])
    return a, b


def run_case(lib, tmp_path, name, seed, n, concurrency, expect):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    # hotel: every service calls its callees one after the other, nothing overlaps: the true forest is chains only
    a, b = check_both_forests(eng, units, rows, table, chain_truth=name == "hotel")
    sizes = np.diff(eng.stitch().tree_off)
    print("%s: trees of %d..%d rows; culprit %d (truth %d), %d of %d selected" % (name, sizes.min(), sizes.max(), a.culprit, b.culprit, a.n_selected, a.n_eligible))
    if expect == "unassigned":
        assert a.n_eligible < n_traces == b.n_eligible           # the default query drops traces with an unassigned call
    eng.close()


@pytest.mark.parametrize("name,seed,n,concurrency,expect", ts.CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in ts.CASES])
def test_device_equals_host_restatement(emu_lib, tmp_path, name, seed, n, concurrency, expect):
    run_case(emu_lib, tmp_path, name, seed, n, concurrency, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,n,concurrency,expect", ts.CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in ts.CASES])
def test_device_equals_host_restatement_gpu(tmp_path, name, seed, n, concurrency, expect):
    run_case(None, tmp_path, name, seed, n, concurrency, expect)


def run_left_out(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 300, 2.0)
    units = [u for u in units if u.service != "search"]
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    a, b = check_both_forests(eng, units, rows, table)
    assert b.n_eligible == n_traces                               # the fragments below the holes are not eligible by default
    eng.close()


def test_a_left_out_service(emu_lib, tmp_path):
    run_left_out(emu_lib, tmp_path)


@pytest.mark.gpu
def test_a_left_out_service_gpu(tmp_path):
    run_left_out(None, tmp_path)


def run_skip(lib, tmp_path):
    from traceweaver_amd import skipmode
    from traceweaver_amd.ingest import IngestedUnit

    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 11, 400, 1.5)
    u = [x for x in units if x.service == "frontend"][0]
    arr, truth, kept = skipmode.cache_hits(u.arrays, u.true_parent, 0.2, in_trace=u.in_trace)
    unit = IngestedUnit(arr, truth, u.in_trace, u.service, u.in_ep, u.out_eps, u.in_rows,
                        [r[kept] if e == 0 else r for e, r in enumerate(u.out_rows)], u.process_id)
    eng = Engine(0, lib_path=lib)
    eng.load([arr], skip=[skipmode.plan(eng, arr)])
    eng.set_truth([truth], [unit.in_trace], n_traces)
    eng.run_pass1()
    rows = traces.rows_from_units([unit], table, deleted=u.out_rows[0][~kept])
    eng.set_span_rows(*rows)
    check_both_forests(eng, [unit], rows, table, pass_=1)
    eng.close()


def test_skip_mode_batch(emu_lib, tmp_path):
    run_skip(emu_lib, tmp_path)


@pytest.mark.gpu
def test_skip_mode_batch_gpu(tmp_path):
    run_skip(None, tmp_path)


def run_scaled(lib, tmp_path):
    from traceweaver_amd import transforms
    from traceweaver_amd.ingest import IngestedUnit

    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 300, 1.5)
    factors = [3, 2]
    eng = Engine(0, lib_path=lib)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    rows = list(traces.rows_from_units(units, table))
    eng.set_span_rows(*rows)
    group, names = traces.groups_from_table(table)
    eng.set_row_groups(group, len(names))
    eng.stitch(truth=True)
    eng.attribute()
    perms = eng.scale_load(factors)
    with pytest.raises(EngineError) as ex:                        # the row maps are dropped, the groups and the forest with them
        eng.attribute()
    assert ex.value.code == -4
    host = [transforms.compress_unit(u.arrays, u.true_parent, f) for u, f in zip(units, factors)]
    rows[0] = [u.in_rows[ip] for u, (ip, _, _) in zip(units, perms)]
    rows[1] = [[r[p] for r, p in zip(u.out_rows, ops)] for u, (_, ops, _) in zip(units, perms)]
    eng.set_span_rows(*rows)
    eng.run_pass1()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    scaled = [IngestedUnit(s.arrays, s.true_parent, u.in_trace, u.service, u.in_ep, u.out_eps, r_in, r_out, u.process_id)
              for s, u, r_in, r_out in zip(host, units, rows[0], rows[1])]
    check_both_forests(eng, scaled, rows, table)
    eng.close()


def test_after_load_scaling(emu_lib, tmp_path):
    run_scaled(emu_lib, tmp_path)


@pytest.mark.gpu
def test_after_load_scaling_gpu(tmp_path):
    run_scaled(None, tmp_path)


def run_given(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "media", 7, 300, 6.0)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    par = [r["parent"] for r in eng.results(2, fields=("parent",))]
    eng.close()
    other = Engine(0, lib_path=lib)
    other.load([u.arrays for u in units])
    other.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    other.set_span_rows(*rows)
    other.set_parents(par)
    check_both_forests(other, units, rows, table, par=par, pass_=0)
    other.close()


def test_parents_handed_over_by_the_caller(emu_lib, tmp_path):
    run_given(emu_lib, tmp_path)


@pytest.mark.gpu
def test_parents_handed_over_by_the_caller_gpu(tmp_path):
    run_given(None, tmp_path)


def run_many_groups(lib, tmp_path):
    """One group per row and a group that is not counted: more groups than a workgroup of k_attr_reduce keeps in LDS."""
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "media", 7, 120, 6.0)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    n = len(table["service"])
    group = (np.arange(n, dtype=np.int32) * 7) % 1031
    group[::5] = -1
    eng.set_row_groups(group, 1031)
    st = eng.stitch()
    link = links_of([u.arrays for u in units], [r["parent"] for r in eng.results(2, fields=("parent",))], rows)
    check_forest(eng, st, link, rows, group, 1031, all_queries=False)
    eng.close()


def test_more_groups_than_the_lds_table(emu_lib, tmp_path):
    run_many_groups(emu_lib, tmp_path)


@pytest.mark.gpu
def test_more_groups_than_the_lds_table_gpu(tmp_path):
    run_many_groups(None, tmp_path)


def run_large_tree(lib):
    """A tree of more rows than a wavefront of the HIP build holds in LDS (and far more than the host build's tables): 600 server
    spans that name one call as their caller -- the table of tw_set_span_rows allows it -- some of them overlapping."""
    u, tp = synth.make_unit(3, 2, shape="single")
    n = 600
    c0, c1 = 2 + int(tp[0][0]), 2 + int(tp[0][1])                 # rows 0, 1: the requests; 2, 3: the calls; then the callees
    start = np.zeros(4 + n, dtype=np.int64)
    end = np.zeros(4 + n, dtype=np.int64)
    start[[0, 1, c0, c1]], end[[0, 1, c0, c1]] = [0, 5, 10, 6], [100000, 50, 99990, 40]
    i = np.arange(n)
    start[4:] = 100 + 150 * i
    end[4:] = start[4:] + np.where(i % 3 == 0, 220, 100)          # every third one reaches into the next
    row_link = np.array([-1, -1, -1, -1] + [c0] * n, dtype=np.int32)
    kind = np.array([1, 1, 2, 2] + [1] * n, dtype=np.uint8)
    rows = ([np.array([0, 1], dtype=np.int32)], [[np.array([2, 3], dtype=np.int32)]], row_link, kind, start, end)
    group = (np.arange(4 + n) % 5).astype(np.int32)
    eng = Engine(0, lib_path=lib)
    eng.load([u])
    eng.set_span_rows(*rows)
    eng.set_parents([tp])
    eng.set_row_groups(group, 5)
    st = eng.stitch(0)
    assert np.diff(st.tree_off).tolist() == [n + 2, 2]
    a = check_forest(eng, st, links_of([u], [tp], rows), rows, group, 5, all_queries=False)
    assert a.tree_path_rows.tolist() == [n + 2, 2] and a.path_time[c0] == a.self_time[c0] == 99980 - 100 * n - 50 * (n // 3)   # a reaching span and the next cover 250, not 200
    eng.close()


def test_a_tree_beyond_the_lds_tables(emu_lib):
    run_large_tree(emu_lib)


@pytest.mark.gpu
def test_a_tree_beyond_the_lds_tables_gpu():
    run_large_tree(None)


# ---- 5. state and argument errors -------------------------------------------------------------------------------------------
def run_errors(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table)
    eng = Engine(0, lib_path=lib)

    def error(code, f, *a, **kw):
        with pytest.raises(EngineError) as ex:
            f(*a, **kw)
        assert ex.value.code == code and {-4: "TW_ERR_STATE", -1: "TW_ERR_ARG"}[code] in str(ex.value)

    def load():
        eng.load([u.arrays for u in units])
        eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)

    load()
    eng._n_rows = len(group)
    error(-4, eng.set_row_groups, group, len(names))              # before set_span_rows
    eng.set_span_rows(*rows)
    eng.stitch(truth=True)
    error(-4, eng.attribute)                                      # before set_row_groups
    eng.set_row_groups(group, len(names))
    assert eng.attribute().n_selected == n_traces
    eng.set_span_rows(*rows)                                      # new row maps drop the groups and the forest
    error(-4, eng.attribute)
    eng.set_row_groups(group, len(names))
    error(-4, eng.attribute)                                      # before a stitch
    eng.stitch(truth=True)
    assert eng.attribute(percentile=0.5).n_selected == n_traces - n_traces // 2
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        error(-1, eng.attribute, percentile=bad)
    error(-1, eng.attribute, start_min=5, start_max=4)
    for value in (len(names), -2):
        g = group.copy()
        g[3] = value
        error(-1, eng.set_row_groups, g, len(names))
    error(-1, eng.set_row_groups, group, 0)
    with pytest.raises(ValueError):
        eng.set_row_groups(group[:-1], len(names))
    assert eng.attribute().n_selected == n_traces                 # a refused call leaves the groups as they were
    eng.run_pass1()                                               # a new pass drops the forest
    error(-4, eng.attribute)
    eng.stitch()
    eng.attribute()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    error(-4, eng.attribute)
    eng.stitch()
    eng.attribute()
    load()                                                        # a load drops everything
    error(-4, eng.attribute)
    eng.close()


def test_state_and_argument_errors(emu_lib, tmp_path):
    run_errors(emu_lib, tmp_path)


@pytest.mark.gpu
def test_state_and_argument_errors_gpu(tmp_path):
    run_errors(None, tmp_path)   # (all refused on the host: nothing malformed reaches the device)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------
def test_cli_attribute_out(emu_lib, tmp_path, capsys):
    from traceweaver_amd import executor

    synth.write_jaeger_corpus(str(tmp_path / "corpus"), 11, 400, app=synth.HOTEL_APP, concurrency=2.5)
    runs, text = {}, {}
    both = ["--stitch_out", str(tmp_path / "traces.npz"), "--attribute_out", str(tmp_path / "attr.npz"), "--query_percentile", "0.9", "-v"]
    for tag, extra in (("plain", []), ("both", both), ("alone", ["--attribute_out", str(tmp_path / "alone.npz"), "--query_percentile", "0.9"])):
        out = str(tmp_path / tag) + "/"
        executor.main(["--absolute_path", str(tmp_path / "corpus"), "--cache_rate", "0", "--fix", "2", "--results_directory", out,
                       "--test_name", "gen", "--load_level", "7", "--engine_library", emu_lib] + extra)
        runs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        text[tag] = capsys.readouterr().out
    assert len(runs["plain"]) == 5 and runs["plain"] == runs["both"] == runs["alone"]     # the five pickles, byte for byte
    assert "Delay culprit" not in text["plain"] and "Stitched traces:" not in text["alone"] and "Stitched traces:" in text["both"]
    z, s = np.load(str(tmp_path / "attr.npz")), np.load(str(tmp_path / "traces.npz"))
    alone = np.load(str(tmp_path / "alone.npz"))
    assert all(np.array_equal(z[k], alone[k]) for k in z.files)
    line = [x for x in text["both"].splitlines() if x.startswith("Delay culprit:")]
    assert len(line) == 1 and line == [x for x in text["alone"].splitlines() if x.startswith("Delay culprit")]
    assert len([x for x in text["both"].splitlines() if x.startswith("Delay culprit (true traces):")]) == 1
    g = int(z["summary"][4])
    cols = {c: z["groups"][i] for i, c in enumerate(z["group_columns"])}
    assert line[0] == "Delay culprit: %s, mean service latency %.1f us over %d of %d traces (critical-path share %.1f %%)" % (
        z["group_names"][g], cols["span_time"][g] / cols["span_rows"][g], z["summary"][1], z["summary"][0],
        100.0 * cols["path_time"][g] / cols["path_time"].sum())
    assert z["summary"][2] == int(0.9 * z["summary"][0]) and 0 < z["summary"][1] <= z["summary"][0] - z["summary"][2]
    # the per-group table again, from the stitched file of the same run
    st = traces.StitchedTraces(*[s[k] for k in traces.StitchedTraces.FIELDS])
    names = z["group_names"].tolist()
    assert sorted(names) == np.unique(s["row_service"]).tolist()
    group = np.array([names.index(x) for x in s["row_service"]], dtype=np.int32)
    want = traces.attribute_host(st, z["link"], s["row_start"], s["row_end"], group, len(names), percentile=0.9)
    assert np.array_equal(want.groups, z["groups"]) and np.array_equal(want.summary, z["summary"])
    assert np.array_equal(want.path_time, z["path_time"]) and np.array_equal(want.tree_selected, z["tree_selected"])
    base = ["--absolute_path", "x", "--fix", "2", "--results_directory", str(tmp_path) + "/", "--engine_library", emu_lib, "--attribute_out", "a.npz"]
    for extra in (["--cache_rate", "0.1"], ["--cache_rate", "0", "--predictor_indices", "3"], ["--cache_rate", "0", "--query_percentile", "1"]):
        with pytest.raises(SystemExit):
            executor.main(base + extra)


# ---- 7. a shipped corpus ----------------------------------------------------------------------------------------------------
def test_shipped_hotel_corpus(emu_lib, reference_root):
    """hotel_load100 end to end: device = restatement on the predicted and on the true forest, and the true forest's figures
    equal a direct computation from the span table's trace column.  How close the predicted traces' answer comes to the true
    one is printed (recorded in DESIGN.md section 9), not asserted."""
    from traceweaver_amd.ingest import REFERENCE_FIX, open_directory

    first_span, fix = REFERENCE_FIX[2]
    corpus, _ = open_directory(os.path.join(reference_root, "data", "hotel_reservation", "hotel_load100"), lib_path=emu_lib, first_span=first_span,
                               fix=fix, cache=False)
    units, skipped, n_traces = corpus.units()
    table = corpus.span_table()
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(emu_lib, units, n_traces, rows)
    group, names = traces.groups_from_table(table, corpus)
    eng.set_row_groups(group, len(names))
    start, end = rows[4], rows[5]
    out = {}
    for tag, kw, par in (("predicted", {}, [r["parent"] for r in eng.results(2, fields=("parent",))]), ("true", dict(truth=True), [u.true_parent for u in units])):
        st = eng.stitch(**kw)
        link = links_of([u.arrays for u in units], par, rows)
        for q in (dict(percentile=0.95), dict()):
            dev = eng.attribute(**q)
            want = traces.attribute_host(st, link, start, end, group, len(names), **q)
            for k in traces.Attribution.FIELDS:
                assert np.array_equal(getattr(dev, k), getattr(want, k)), (tag, k)
        out[tag] = (st, eng.attribute(percentile=0.95))
    st, a = out["true"]
    # the true forest from the table alone: the traces are the trace column, their latency is the latest end less the root's start
    root_of = ts.trace_roots(table, n_traces)
    latest = np.full(n_traces, np.iinfo(np.int64).min)
    np.maximum.at(latest, table["trace"], end)
    latency = latest - start[root_of]
    order = np.lexsort((root_of, latency))                        # (latency, tree): trees are numbered by root row
    k = int(0.95 * n_traces)
    chosen = np.zeros(n_traces, dtype=bool)
    chosen[order[k:]] = True
    in_sel = chosen[table["trace"]]
    assert a.summary[:4].tolist() == [n_traces, n_traces - k, k, int(latency[order[k]])]
    assert np.array_equal(a.group_span_rows, np.bincount(group[in_sel], minlength=len(names)))
    assert np.array_equal(a.group_span_time, np.bincount(group[in_sel], weights=(end - start)[in_sel], minlength=len(names)).astype(np.int64))
    assert int(a.group_path_time.sum()) == int((end - start)[root_of[chosen]].sum())
    for tag in ("predicted", "true"):
        a = out[tag][1]
        print("%s traces: culprit %s, %d of %d selected, rank latency %d us" % (tag, names[a.culprit], a.n_selected, a.n_eligible, a.rank_latency))
        for row in a.table(names):
            print("    %-12s mean %10.1f us  path share %5.1f %%  top in %d trees" % (row["group"], row["mean_latency"], 100 * row["path_share"], row["top_trees"]))
    eng.close()
