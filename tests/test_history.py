"""Engine.history_* (tw_history_reset / _push / _merge / _info / _distributions / _compare, csrc/tw_hist.h): the latency
distributions of batch after batch kept on the device, merged segment by segment, and the distribution and comparison queries
over that store.  The yardstick is traces.history_host -- the parts concatenated and sorted with numpy and Python integers --
and traces.compare_cohorts_host on its result; part 1 checks the restatement by hand, the rest compares the device with it,
np.array_equal on every field of LatencyDistributions.FIELDS / CohortComparison.FIELDS.  Corpora, cases and helpers are those of
tests/test_stitch.py, tests/test_distributions.py and tests/test_compare.py.  CPU tier: host-emulation build (a merge tile of 8
items, so a few dozen rows cross tile boundaries; one lane per workgroup, and once one host thread per lane); the HIP library,
whose tile holds 2048 items, under -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_attribute as ta  # noqa: F401  (test_distributions imports it by this name)
import test_compare as tc
import test_distributions as td
import test_stitch as ts
from traceweaver_amd import synth, traces
from traceweaver_amd.engine import Engine, EngineError

PROBS, EDGES = td.PROBS, td.EDGES
TILE_EMU, TILE_GPU = 8, 2048                                      # kHistTile of csrc/tw_hist.h under TW_TILE_SMALL / in the HIP build
STORED = ("seg_count", "seg_sum", "seg_off", "values")            # what the history holds; the rest of FIELDS follows from a query


def same(dev, want, tag=None, fields=traces.LatencyDistributions.FIELDS):
    for k in fields:
        assert np.array_equal(getattr(dev, k), getattr(want, k)), (k, tag)


def error(code, f, *a, **kw):
    with pytest.raises(EngineError) as ex:
        f(*a, **kw)
    assert ex.value.code == code and {-4: "TW_ERR_STATE", -1: "TW_ERR_ARG", -2: "TW_ERR_UNSUPPORTED"}[code] in str(ex.value)


# ---- 1. the restatement by hand ---------------------------------------------------------------------------------------------
def test_host_by_hand():
    h = traces.history_host([(tc.lists([[1, 5, 5]]), None), (tc.lists([[2, 5]]), None)], (0.5, 1.0), [5])
    assert h.segment(0, 0, 0).tolist() == [1, 2, 5, 5, 5] and h.seg_count.tolist() == [5, 0, 0, 0] and h.seg_sum.tolist() == [18, 0, 0, 0]
    assert h.seg_off.tolist() == [0, 5, 5, 5, 5] and h.quantile[0].tolist() == [5, 5] and h.hist[0].tolist() == [2, 3] and h.quantile[1].tolist() == [td.EMPTY] * 2
    assert h.summary.tolist() == [5, 1, 1, 2] and len(h.tree_cohort) == 0 and (h.n_cohorts, h.n_groups) == (1, 1)
    # a map [1, -1]: the part's cohort 0 goes to cohort 1, its cohort 1 nowhere; cohort 0 of the history exists and is empty
    h = traces.history_host([(tc.lists([[3, 1], [7]]), [1, -1])])
    assert h.n_cohorts == 2 and h.seg_count.tolist() == [0] * 4 + [2, 0, 0, 0] and h.segment(1, 0, 0).tolist() == [1, 3] and h.summary.tolist() == [2, 1, 2, 1]
    # a map to cohort 3 of a history of two cohorts: cohort 2 exists and is empty
    h = traces.history_host([(tc.lists([[4], [6, 2]]), None), (tc.lists([[5]]), [3])])
    assert h.n_cohorts == 4 and h.seg_count[::4].tolist() == [1, 2, 0, 1] and len(h.segment(2, 0, 0)) == 0 and h.segment(3, 0, 0).tolist() == [5]
    assert h.values.tolist() == [4, 2, 6, 5] and h.summary.tolist() == [4, 3, 4, 2]
    # a negative trace latency sorts first (a root with end < start: latency -50, duration 0)
    d, _ = td.hand([(100, 50, -1), (200, 230, -1), (300, 300, -1)], [0, 0, 0], 1)
    e, _ = td.hand([(10, 12, -1), (400, 300, -1)], [0, 0], 1)
    h = traces.history_host([(d, None), (e, None)], (0.0,))
    assert h.segment(0, 3).tolist() == [-100, -50, 0, 2, 30] and h.segment(0, 0, 0).tolist() == [0, 0, 0, 2, 30] and h.quantile[3].tolist() == [-100]
    assert h.seg_sum[3] == -118
    for bad in ([(tc.lists([[1], [2]]), [0, 0])], [(tc.lists([[1]]), [-2])], [(tc.lists([[1]]), [0, 1])], []):
        with pytest.raises(ValueError):
            traces.history_host(bad)


def run_by_hand(lib):
    """The same parts through tw_history_merge on an engine that never saw a batch."""
    eng = Engine(0, lib_path=lib)
    assert eng.history_info() == dict(cohorts=0, groups=0, segments=0, items=0, pushes=0, capacity=0)
    parts = [(tc.lists([[1, 5, 5]]), None), (tc.lists([[2, 5]]), None)]
    assert eng.history_merge(parts[0][0]).tolist() == [3, 3, 1, 1] and eng.history_merge(parts[1][0]).tolist() == [2, 5, 1, 2]
    h = eng.history_distributions((0.5, 1.0), [5])
    assert h.segment(0, 0, 0).tolist() == [1, 2, 5, 5, 5] and h.seg_count[0] == 5 and h.seg_sum[0] == 18
    same(h, traces.history_host(parts, (0.5, 1.0), [5]))
    parts += [(tc.lists([[3, 1], [7]]), [1, -1]), (tc.lists([[5]]), [3])]
    eng.history_merge(parts[2][0], [1, -1])
    assert eng.history_merge(parts[3][0], [3]).tolist() == [1, 8, 4, 4]
    h = eng.history_distributions(PROBS, EDGES)
    assert h.n_cohorts == 4 and len(h.segment(2, 0, 0)) == 0 and h.segment(1, 0, 0).tolist() == [1, 3] and h.segment(3, 0, 0).tolist() == [5]
    same(h, traces.history_host(parts, PROBS, EDGES))
    info = eng.history_info()
    assert (info["cohorts"], info["groups"], info["segments"], info["items"], info["pushes"]) == (4, 1, 16, 8, 4) and info["capacity"] >= 8
    t = eng.history_timing()
    assert set(t) == {"plan", "merge", "quantiles", "observed", "permutations"} and all(v >= 0 for v in t.values())
    eng.close()


def test_by_hand(emu_lib):
    run_by_hand(emu_lib)


@pytest.mark.gpu
def test_by_hand_gpu():
    run_by_hand(None)


# ---- 2. a partition gives back the whole ------------------------------------------------------------------------------------
def run_partition(lib, tmp_path, name, seed, n, concurrency, expect):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    group, names = traces.groups_from_table(table)
    eng.set_row_groups(group, len(names))
    st = eng.stitch()
    eng.attribute(**td.EVERY)
    D = eng.distributions(PROBS, EDGES)
    # the window is [start_min, start_max): the trees that start before T and those that start at T or later partition the forest
    starts = np.sort(np.asarray(rows[4])[st.tree_root])
    T = int(starts[len(starts) // 2])
    halves = []
    for window in (dict(start_max=T), dict(start_min=T)):
        a = eng.attribute(**dict(td.EVERY, **window))
        assert 0 < a.n_selected < st.n_trees
        halves.append((eng.distributions(PROBS, EDGES), None))
        eng.history_push()
    assert halves[0][0].summary[2] + halves[1][0].summary[2] == D.summary[2] == st.n_trees
    h = eng.history_distributions(PROBS, EDGES)
    same(h, D, name, STORED + ("quantile", "hist"))
    same(h, traces.history_host(halves, PROBS, EDGES), name)
    assert h.summary.tolist() == [D.n_items, D.summary[1], 1, 2]
    eng.close()


@pytest.mark.parametrize("name,seed,n,concurrency,expect", td.CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in td.CASES])
def test_partition_gives_back_the_whole(emu_lib, tmp_path, name, seed, n, concurrency, expect):
    run_partition(emu_lib, tmp_path, name, seed, n, concurrency, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,n,concurrency,expect", td.CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in td.CASES])
def test_partition_gives_back_the_whole_gpu(tmp_path, name, seed, n, concurrency, expect):
    run_partition(None, tmp_path, name, seed, n, concurrency, expect)


# ---- 3. across loads ----------------------------------------------------------------------------------------------------------
def run_across_loads(lib, tmp_path):
    name, _, n, concurrency, _ = td.CASES[0]
    eng = Engine(0, lib_path=lib)
    parts, order = [], None
    for k, seed in enumerate((5, 6)):
        corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path / ("load%d" % k), lib, name, seed, n, concurrency)
        rows = traces.rows_from_units(units, table)
        eng.load([u.arrays for u in units])                       # a load, new row maps, passes, a stitch: the history outlives them all
        eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
        eng.run_pass1()
        eng.fit_mixtures(seed=0)
        eng.run_pass2()
        eng.set_span_rows(*rows)
        group, names = traces.groups_from_table(table, corpus)
        if order is None:
            order = names
        else:                                                     # the groups of the second corpus in the order of the first one's services
            assert sorted(names) == sorted(order)
            group = np.array([order.index(x) for x in names], dtype=np.int32)[group]
        eng.set_row_groups(group, len(names))
        eng.stitch()
        eng.attribute(**td.EVERY)
        if k == 1:                                                # labels in between: one cohort, told by the rows of one service
            eng.set_row_cohorts(np.where(group == len(names) - 1, 0, -1).astype(np.int32), 1)
        parts.append((eng.distributions(tc.PROBS), [k]))
        assert eng.history_push([k]).tolist() == [parts[k][0].n_items, sum(p[0].n_items for p in parts), k + 1, k + 1]
    want = traces.history_host(parts, tc.PROBS)
    same(eng.history_distributions(tc.PROBS), want)
    full = eng.history_compare(((0, 1),), tc.PROBS, permutations=70, seed=5)
    tc.same(full, traces.compare_cohorts_host(want, ((0, 1),), tc.PROBS, 70, 5), "full")
    assert full.summary[0] == full.summary[1] > 0
    pooled = np.sort((full.n_a + full.n_b)[(full.n_a > 0) & (full.n_b > 0)])
    limit = int(pooled[len(pooled) // 2])
    part = eng.history_compare(((0, 1),), tc.PROBS, permutations=70, seed=5, max_pool=limit)
    tc.same(part, traces.compare_cohorts_host(want, ((0, 1),), tc.PROBS, 70, 5, limit), "max_pool")
    assert 0 < part.summary[1] <= part.summary[0]
    # the resident batch answers after a push what it answered before: three cohorts of the second load, two of them kept
    eng.set_row_cohorts(td.service_cohorts(table, rows, group, len(names) - 1), 3)
    before_d, before_c = eng.distributions(PROBS, EDGES), eng.compare_cohorts(tc.PAIRS, tc.PROBS, 20, 4)
    eng.history_push([-1, 2, 3])
    assert eng.distributions(PROBS, EDGES).same_as(before_d)
    tc.same(eng.compare_cohorts(tc.PAIRS, tc.PROBS, 20, 4), before_c)
    same(eng.history_distributions(PROBS, EDGES), traces.history_host(parts + [(before_d, [-1, 2, 3])], PROBS, EDGES))
    tc.same(eng.history_compare(((0, 1),), tc.PROBS, permutations=70, seed=5), full)          # cohorts 0 and 1 were not touched
    eng.close()


def test_across_loads(emu_lib, tmp_path):
    run_across_loads(emu_lib, tmp_path)


@pytest.mark.gpu
def test_across_loads_gpu(tmp_path):
    run_across_loads(None, tmp_path)


# ---- 4. edge shapes against the tile ------------------------------------------------------------------------------------------
def edge_shapes(T):
    """(values of run A, values of run B) per shape: A is pushed first, B merged into it.  Sizes against a tile of T items."""
    rng = np.random.RandomState(T)
    draw = lambda k: rng.randint(0, 3 * T, size=k).tolist()       # noqa: E731  (values with ties)
    return [
        ([], [5, 6, 7]), ([5, 6, 7], []),                         # either run empty
        ([3], [3]), ([4], [2]),                                   # one item against one
        ([1000 + i for i in range(T)], list(range(T - 1))),       # all source values below the history: 2 T - 1 items
        (list(range(T - 1)), [5000, 5001]),                       # ... above: T + 1 items
        (list(range(0, 3 * T + 5, 2)), list(range(1, 3 * T + 5, 2))),                         # strict interleaving: 3 T + 5 items
        ([1, 7] + [7] * (2 * T + 3) + [9], [0] + [7] * (2 * T + 1) + [7, 8]),                 # one run of equal values longer than two tiles on both sides
        (draw(T // 2), draw(T - T // 2)),                         # T items
        (draw(T - 2), [T]),                                       # T - 1 items
        (draw(T), draw(1)),                                       # T + 1 items
    ]


def run_edges(lib, T, shapes_only=False):
    shapes = edge_shapes(T)
    extra, label = [], [-1] * 4                                   # (the table's first four rows stay outside every group and cohort)
    for k, (A, B) in enumerate(shapes):
        for c, run in enumerate((A, B)):
            extra += [(1000 + 3 * len(extra) + i, 1000 + 3 * len(extra) + i + int(v), False) for i, v in enumerate(run)]
            label += [2 * k + c] * len(run)
    lone = 2 * len(shapes)                                        # a cohort that only the first push keeps: copied intact by the second
    extra += [(50, 50 + v, False) for v in (9, 4, 4)]
    label += [lone] * 3
    n = 4 + len(extra)
    group = np.array([-1] * 4 + [0] * len(extra), dtype=np.int32)
    eng, st, rows, group = td.hand_engine(lib, extra, group, 1)
    eng.set_row_cohorts(np.array(label, dtype=np.int32), lone + 1)
    a = eng.attribute(**td.EVERY)
    assert a.n_selected == st.n_trees == len(extra) + 2 and n == len(label)
    d = eng.distributions(PROBS, EDGES)
    first = [k // 2 if k % 2 == 0 else -1 for k in range(lone)] + [len(shapes)]
    second = [k // 2 if k % 2 == 1 else -1 for k in range(lone)] + [-1]
    eng.history_push(first)
    once = eng.history_distributions(PROBS, EDGES)
    same(once, traces.history_host([(d, first)], PROBS, EDGES), "first push")
    eng.history_push(second)
    h = eng.history_distributions(PROBS, EDGES)
    same(h, traces.history_host([(d, first), (d, second)], PROBS, EDGES), "second push")
    for k, (A, B) in enumerate(shapes):
        for m in range(4):                                        # a root of its own: duration = self time = path time = trace latency
            assert h.segment(k, m, None if m == 3 else 0).tolist() == sorted(A + B), (k, m)
    assert h.segment(len(shapes), 0, 0).tolist() == [4, 4, 9] and np.array_equal(h.segment(len(shapes), 3), once.segment(len(shapes), 3))
    sizes = set(h.seg_count.tolist())
    assert {T - 1, T, T + 1, 2 * T - 1, 3 * T + 5} <= sizes
    if shapes_only:
        eng.close()
        return
    # enough pushes of one batch that the value buffers grow: after k pushes every count is k times the batch's
    eng.history_reset()
    ident, caps = list(range(lone + 1)), []
    for k in range(1, 7):
        assert eng.history_push(ident).tolist() == [d.n_items, k * d.n_items, lone + 1, k]
        info = eng.history_info()
        assert info["items"] == k * d.n_items <= info["capacity"]
        caps.append(info["capacity"])
    assert len(set(caps)) >= 3 and caps == sorted(caps)           # the capacity grew at least twice
    h = eng.history_distributions(PROBS, EDGES)
    assert np.array_equal(h.seg_count, 6 * d.seg_count) and np.array_equal(h.seg_sum, 6 * d.seg_sum)
    same(h, traces.history_host([(d, None)] * 6, PROBS, EDGES), "six pushes")
    assert eng.distributions(PROBS, EDGES).same_as(d)
    eng.close()
    # durations up to 2^60 beside a negative trace latency (the data of test_distributions.run_key_width), sums that wrap
    big = 1 << 60
    extra = [(1000 + 7 * i, 1000 + 7 * i + (big >> (i % 50)), False) for i in range(150)] + [(500, 100, False), (700, 650, False)] + \
            [(100 + 150 * i, 100 + 150 * i + 90, True) for i in range(40)]
    n = 4 + len(extra)
    eng, st, rows, group = td.hand_engine(lib, extra, (np.arange(n) % 3).astype(np.int32), 3)
    eng.set_row_cohorts((np.arange(n) % 3 - 1).astype(np.int32), 2)
    a = eng.attribute()
    d = eng.distributions(PROBS, EDGES)
    assert a.n_selected == st.n_trees and st.tree_latency.min() == -400
    parts = [(d, [0, 1]), (d, [1, 0]), (d, [0, -1]), (d, [0, 1])]
    for _, m in parts:
        eng.history_push(m)
    h = eng.history_distributions(PROBS, EDGES)
    same(h, traces.history_host(parts, PROBS, EDGES), "wide values")
    assert h.values.min() == -400 and h.values.max() == big and h.seg_count[h.index(0, 3)] == 3 * d.seg_count[d.index(0, 3)] + d.seg_count[d.index(1, 3)]
    c = eng.history_compare(((0, 1), (1, 0)), (0.0, 0.5, 1.0), permutations=65, seed=1)
    tc.same(c, traces.compare_cohorts_host(h, ((0, 1), (1, 0)), (0.0, 0.5, 1.0), 65, 1), "wide values")
    eng.close()


def test_edge_shapes(emu_lib):
    run_edges(emu_lib, TILE_EMU)


def test_edge_shapes_lane_threaded(emu_lib):
    """One host thread per lane (TW_EMU_LANES=1, workgroups of 256): the two splits of a tile by two threads, the staging, every
    thread's own split on the staged copies and the barriers of k_hist_merge run as they are written, without a GPU (the edge
    shapes and their two pushes)."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "import test_history as t\n"
            "t.run_edges(%r, t.TILE_EMU, shapes_only=True)\n"
            "print('lanes ok')\n") % (os.path.dirname(here), here, emu_lib)
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "lanes ok" in out.stdout, out.stderr[-2000:]


@pytest.mark.gpu
def test_edge_shapes_gpu():
    run_edges(None, TILE_GPU)


# ---- 5. merge from the host ---------------------------------------------------------------------------------------------------
def small_engine(lib, shift=0):
    """A few hundred rows in two groups and two cohorts (the table of test_compare.run_edges), attributed."""
    extra = [(1000 + 7 * i, 1000 + 7 * i + (i * 37 + shift) % 1500, False) for i in range(256)] + [(100 + 150 * i, 100 + 150 * i + 90 + i, True) for i in range(40)]
    n = 4 + len(extra)
    eng, st, rows, group = td.hand_engine(lib, extra, (np.arange(n) % 2).astype(np.int32), 2)
    eng.set_row_cohorts(((np.arange(n, dtype=np.int32) + shift) % 3) - 1, 2)
    eng.attribute(**td.EVERY)
    return eng


def run_merge(lib):
    eng, other = small_engine(lib), small_engine(lib, 11)
    dA, dB = eng.distributions(PROBS, EDGES), other.distributions(PROBS, EDGES)
    assert not np.array_equal(dA.values, dB.values)
    eng.history_push([1, 0])
    eng.history_push([2, -1])
    back = eng.history_distributions(PROBS, EDGES)
    eng.history_reset()
    assert eng.history_info() == dict(cohorts=0, groups=0, segments=0, items=0, pushes=0, capacity=0)
    assert eng.history_merge(back).tolist() == [back.n_items, back.n_items, 3, 1]
    again = eng.history_distributions(PROBS, EDGES)
    same(again, back, "read back and merged", STORED + ("quantile", "hist"))
    assert again.summary.tolist() == back.summary.tolist()[:3] + [1]
    # the distributions of a second engine merged here = pushed there
    eng.history_merge(dB, [0, 3])
    other.history_merge(back)
    other.history_push([0, 3])
    parts = [(dA, [1, 0]), (dA, [2, -1]), (dB, [0, 3])]
    here, there = eng.history_distributions(PROBS, EDGES), other.history_distributions(PROBS, EDGES)
    same(here, there, "merged here, pushed there", STORED + ("quantile", "hist"))
    same(here, traces.history_host(parts, PROBS, EDGES), fields=STORED + ("quantile", "hist"))
    assert here.summary.tolist() == [dA.n_items + int(dA.seg_off[7]) + dB.n_items, here.summary[1], 4, 2]     # (seg_off[7]: cohort 0 of dA)
    # a segment with one inversion; offsets that do not start at 0 or that decrease: refused, the history as it was
    info = eng.history_info()
    s = int(np.flatnonzero(dB.seg_count >= 3)[-1])
    lo = int(dB.seg_off[s])
    k = lo + int(np.flatnonzero(np.diff(dB.values[lo:int(dB.seg_off[s + 1])]) > 0)[0])
    bad = dB.values.copy()
    bad[k], bad[k + 1] = bad[k + 1], bad[k]
    error(-1, eng.history_merge, (2, 2, dB.seg_off, bad))
    off = dB.seg_off.copy()
    off[0] = 1
    error(-1, eng.history_merge, (2, 2, off, dB.values))
    off = dB.seg_off.copy()
    off[s] = off[s + 1] + 1
    error(-1, eng.history_merge, (2, 2, off, dB.values))
    error(-1, eng.history_merge, dB, [0, 0])
    error(-1, eng.history_merge, dB, [0, -2])
    error(-1, eng.history_merge, (1, 1, np.zeros(5, dtype=np.int64), np.zeros(0, dtype=np.int64)))       # another G
    with pytest.raises(ValueError):
        eng.history_merge((2, 2, dB.seg_off[:-1], dB.values))
    assert eng.history_info() == info
    same(eng.history_distributions(PROBS, EDGES), here, "after the refusals")
    # a swap across a segment boundary is no inversion: the segments are checked one by one
    assert eng.history_merge((2, 2, dB.seg_off, dB.values), [-1, -1]).tolist() == [0, here.n_items, 4, 3]
    eng.close()
    other.close()


def test_merge_from_the_host(emu_lib):
    run_merge(emu_lib)


@pytest.mark.gpu
def test_merge_from_the_host_gpu():
    run_merge(None)


# ---- 6. state and arguments ---------------------------------------------------------------------------------------------------
def run_errors(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table)
    G = len(names)
    label = td.service_cohorts(table, rows, group, G - 1)
    eng = td.truth_engine(lib, units, n_traces, rows)
    eng.set_row_groups(group, G)
    eng.set_row_cohorts(label, 3)
    for f in (eng.history_distributions, eng.history_compare):    # queries on an empty history
        error(-4, f)
    error(-4, eng.history_push)                                   # before a stitch
    eng.stitch(0)
    error(-4, eng.history_push)                                   # before attribute()
    assert eng.history_info()["pushes"] == 0
    eng.attribute(**td.EVERY)
    d = eng.distributions(PROBS, EDGES)
    eng.history_push()                                            # builds nothing anew: the items are resident
    eng.history_push([2, 1, 0])
    parts = [(d, None), (d, [2, 1, 0])]
    want = traces.history_host(parts, PROBS, EDGES)
    info = eng.history_info()

    def intact():
        assert eng.history_info() == info
        same(eng.history_distributions(PROBS, EDGES), want)

    intact()
    for bad in ([0, 1], [0, 1, 2, 3], [0, 1, 1], [0, 0, -1], [0, -2, 1]):                                 # n_map, a repeated entry, below -1
        error(-1, eng.history_push, bad)
    error(-2, eng.history_push, [0, 1, (1 << 24) // (3 * G + 1)])                                        # C_h * per beyond 2^24
    error(-1, eng.history_merge, (1, G + 1, np.zeros(3 * (G + 1) + 2, dtype=np.int64), np.zeros(0, dtype=np.int64)))     # another G
    # the argument errors of tw_latency_distributions / tw_compare_cohorts, pairs against C_h = 3
    for bad in ((-0.1,), (1.5,), (0.5, float("nan")), [0.5] * 33):
        error(-1, eng.history_distributions, bad)
    for bad in ((3, 3), (5, 4), list(range(64))):
        error(-1, eng.history_distributions, (0.5,), bad)
    assert eng.history_distributions((), list(range(63))).hist.shape == (3 * (3 * G + 1), 64)
    for bad in ((), [(0, 1)] * 65, ((0, 3),), ((-1, 0),), ((1, 1),)):
        error(-1, eng.history_compare, bad)
    for bad in ((-0.1,), (1.5,), (0.5, float("nan")), [0.5] * 9):
        error(-1, eng.history_compare, tc.PAIRS, bad)
    error(-1, eng.history_compare, tc.PAIRS, tc.PROBS, -1)
    error(-1, eng.history_compare, tc.PAIRS, tc.PROBS, 65537)
    error(-1, eng.history_compare, tc.PAIRS, tc.PROBS, 5, 0, -1)
    with pytest.raises(ValueError):
        eng.history_compare((0, 1, 2))
    intact()
    tc.same(eng.history_compare(tc.PAIRS, tc.PROBS, 20, 4), traces.compare_cohorts_host(want, tc.PAIRS, tc.PROBS, 20, 4))
    # another number of groups after the first push: refused; whatever drops the forest leaves the history alone
    eng.set_row_groups(np.where(group >= 0, 0, -1).astype(np.int32), 1)
    eng.attribute(**td.EVERY)
    error(-1, eng.history_push)
    eng.set_span_rows(*rows)
    error(-4, eng.history_push)
    eng.run_pass1()
    eng.load([u.arrays for u in units])
    error(-4, eng.history_push)
    intact()
    eng.history_reset()
    for f in (eng.history_distributions, eng.history_compare):
        error(-4, f)
    assert eng.history_info() == dict(cohorts=0, groups=0, segments=0, items=0, pushes=0, capacity=0)
    eng.history_merge(tc.lists([[1, 2], [3]]))                    # G is open again
    assert eng.history_info()["groups"] == 1 and eng.history_compare(((0, 1),), ()).ks_gap[0] == 2
    eng.close()


def test_state_and_argument_errors(emu_lib, tmp_path):
    run_errors(emu_lib, tmp_path)


@pytest.mark.gpu
def test_state_and_argument_errors_gpu(tmp_path):
    run_errors(None, tmp_path)   # (all refused before a merge kernel runs: nothing malformed reaches it)


# ---- 7. the command line ------------------------------------------------------------------------------------------------------
def test_cli_history(emu_lib, tmp_path, capsys):
    from traceweaver_amd import executor

    synth.write_jaeger_corpus(str(tmp_path / "corpus"), 11, 400, app=synth.HOTEL_APP, concurrency=2.5)
    store, cmp_out = str(tmp_path / "h.npz"), str(tmp_path / "c.npz")

    def run(tag, extra):
        out = str(tmp_path / tag) + "/"
        executor.main(["--absolute_path", str(tmp_path / "corpus"), "--cache_rate", "0", "--fix", "2", "--results_directory", out,
                       "--test_name", "gen", "--load_level", "7", "--engine_library", emu_lib, "--query_percentile", "0.5", "--quantiles", "0.5,0.9,1",
                       "--latency_out", str(tmp_path / (tag + ".npz"))] + extra)
        return {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}, open(str(tmp_path / (tag + ".npz")), "rb").read(), capsys.readouterr().out

    plain = run("plain", [])                                      # no store beside it
    first = run("first", ["--history", store, "--history_cohort", "0"])
    (C, G, off, values), group_names, cohort_names = traces.read_history_npz(store)
    lat = np.load(str(tmp_path / "first.npz"))
    assert (C, G) == (1, int(lat["n_groups"])) and np.array_equal(off, lat["seg_off"]) and np.array_equal(values, lat["values"])
    assert group_names == lat["group_names"].tolist() and cohort_names == ["0"]
    second = run("second", ["--history", store, "--history_cohort", "1", "--history_compare_out", cmp_out, "--permutations", "20", "--compare_seed", "8"])
    (C, G, off2, values2), _, cohort_names = traces.read_history_npz(store)
    assert C == 2 and cohort_names == ["0", "1"] and len(values2) == 2 * len(values) and np.array_equal(off2, np.concatenate([off, off[-1] + off[1:]]))
    assert np.array_equal(values2[:len(values)], values) and np.array_equal(values2[len(values):], values)
    d = traces.LatencyDistributions(np.zeros(0, np.int32), lat["seg_count"], lat["seg_sum"], lat["seg_off"], lat["values"], lat["quantile"], lat["hist"],
                                    lat["summary"], 1, G, lat["probs"])
    want = traces.compare_cohorts_host(traces.history_host([(d, [0]), (d, [1])]), ((0, 1),), (0.5, 0.9, 1.0), 20, 8)
    z = np.load(cmp_out)
    for k in traces.CohortComparison.FIELDS:
        assert np.array_equal(z[k], getattr(want, k)), k
    assert z["pairs"].tolist() == [[0, 1]] and z["n_perm"] == 20 and (z["ks_gap"] == 0).all() and z["group_names"].tolist() == group_names
    assert "History: %d values added to cohort 1, %d held in 2 cohorts" % (len(values), 2 * len(values)) in second[2] and "History comparison: 1 pairs" in second[2]
    # without the flags nothing changes, with or without a store lying beside the run
    again = run("again", [])
    assert plain[0] == first[0] == second[0] == again[0] and len(plain[0]) == 5                          # the five pickles, byte for byte
    assert plain[1] == again[1] == first[1] == second[1] and "History" not in plain[2] + again[2]
    # a store of other services is refused; so are the flags without what they need
    h = traces.history_host([(tc.lists([[1]]), None)])
    traces.write_history_npz(str(tmp_path / "foreign_store.npz"), h, ["nobody"])
    with pytest.raises(SystemExit) as ex:
        run("other", ["--history", str(tmp_path / "foreign_store.npz")])
    assert "nobody" in str(ex.value)
    with pytest.raises(SystemExit):                                # a cohort the store does not have
        run("range", ["--history", store, "--history_compare_out", cmp_out, "--compare_pairs", "0,9"])
    base = ["--absolute_path", "x", "--fix", "2", "--results_directory", str(tmp_path) + "/", "--engine_library", emu_lib, "--cache_rate", "0"]
    ok = ["--latency_out", "l.npz", "--history", "h.npz", "--history_compare_out", "c.npz"]
    for extra in (ok[2:], ok[:2] + ok[4:], ok[:4] + ["--history_cohort", "-1"], ok[:2] + ["--history_cohort", "1"], ok + ["--compare_pairs", "0,0"],
                  ok + ["--permutations", "65537"], ok + ["--compare_seed", "-1"], ok + ["--quantiles", ",".join(["0.5"] * 9)]):
        with pytest.raises(SystemExit):
            executor.main(base + extra)
