"""Engine.set_row_cohorts / Engine.distributions (tw_set_row_cohorts, tw_latency_distributions, csrc/tw_dist.h): the populations
behind an attribution -- per cohort, metric and group the sorted values, counts, sums, quantiles and a histogram.  The yardstick
is traces.distributions_host, the definitions of include/traceweaver_amd.h restated in plain Python; part 1 checks it on forests
written out by hand, the rest compares the device with it, np.array_equal on every field of LatencyDistributions.FIELDS.
Corpora, cases and helpers are those of tests/test_stitch.py and tests/test_attribute.py.  CPU tier: host-emulation build (an
LDS table of 16 segments: both counting routes occur; one lane per workgroup, and once one host thread per lane, which is
where the wavefront aggregation is exercised without a GPU); the HIP library under -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_attribute as ta
import test_stitch as ts
from traceweaver_amd import synth, traces
from traceweaver_amd.engine import Engine, EngineError

W, U = traces.WHOLE, traces.UNASSIGNED
EMPTY = np.iinfo(np.int64).min
PROBS = (0.0, 0.5, 0.9, 0.95, 0.99, 1.0)
EDGES = (0, 1, 50, 400, 2000, 10000, 60000)
EVERY = dict(need_flags=0, skip_flags=0)                          # the query that selects every tree


# ---- 1. the restatement on a forest written out by hand -------------------------------------------------------------------
def hand(rows, group, n_groups, flags=None, label=None, n_cohorts=1, probs=(0.0, 0.5, 1.0), edges=None, **query):
    a, st = ta.host(rows, group=group, n_groups=n_groups, flags=flags, **query)
    start, end = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    return traces.distributions_host(st, a, start, end, group, n_groups, label, n_cohorts, probs, edges), a


# tree 0: rows 0..5 (the fan-out of test_attribute), tree 1: rows 6..8, a chain; tree 2: row 9; tree 3: row 10, a fragment;
# tree 4: row 11, slower than all of them
ROWS = [(0, 100, -1), (10, 90, 0), (20, 50, 0), (85, 95, 0), (96, 99, 0), (30, 60, 1),
        (200, 260, -1), (210, 250, 6), (220, 240, 7), (300, 310, -1), (400, 450, -1), (500, 700, -1)]
GROUP = [0, 1, 1, 2, -1, 2, 0, 1, 2, 0, 0, 0]
FLAGS = {0: W, 6: W, 9: W, 10: 0, 11: W}


def test_host_items_by_hand():
    d, a = hand(ROWS, GROUP, 3, FLAGS, edges=[30, 100])
    assert a.tree_selected.tolist() == [1, 1, 1, 0, 1] and d.summary.tolist() == [33, 10, 4, 0]
    assert d.tree_cohort.tolist() == [0] * 5 and len(d.seg_count) == 10
    assert d.segment(0, 0, 0).tolist() == [10, 60, 100, 200] and d.segment(0, "span_latency", 1).tolist() == [30, 40, 80]
    assert d.segment(0, 0, 2).tolist() == [10, 20, 30]
    assert d.segment(0, 1, 0).tolist() == [10, 12, 20, 200] and d.segment(0, 1, 1).tolist() == [20, 30, 50] and d.segment(0, 1, 2).tolist() == [10, 20, 30]
    # row 2 is never walked (test_attribute): metric 2 holds one value less of group 1
    assert d.segment(0, 2, 0).tolist() == [10, 12, 20, 200] and d.segment(0, 2, 1).tolist() == [20, 45] and d.segment(0, 2, 2).tolist() == [10, 20, 30]
    assert d.segment(0, 3).tolist() == [10, 60, 100, 200]     # the fragment's 50 is not selected: it contributes nothing
    assert d.seg_count.tolist() == [4, 3, 3, 4, 3, 3, 4, 2, 3, 4]
    assert d.seg_off.tolist() == np.concatenate([[0], np.cumsum(d.seg_count)]).tolist() and d.seg_off[-1] == 33
    assert d.seg_sum[:3].tolist() == [370, 150, 60] and d.seg_sum[9] == 370
    # quantile index min(n - 1, int(p * n)): n = 4: 0, 2, 3; n = 3: 0, 1, 2; n = 2: 0, 1, 1
    assert d.quantile[0].tolist() == [10, 100, 200] and d.quantile[1].tolist() == [30, 40, 80] and d.quantile[7].tolist() == [20, 45, 45]
    # a value on an edge falls in the upper bin: 30 >= 30, 100 >= 100
    assert d.hist[0].tolist() == [1, 1, 2] and d.hist[1].tolist() == [0, 3, 0] and d.hist[2].tolist() == [2, 1, 0]
    assert np.array_equal(d.hist.sum(axis=1), d.seg_count)
    rows = d.table(["a", "b", "c"])
    assert len(rows) == 10 and rows[1] == {"cohort": 0, "metric": "span_latency", "group": "b", "count": 3, "mean": 50.0, "p0": 30, "p50": 40, "p100": 80}
    assert rows[9]["group"] is None and rows[9]["metric"] == "trace_latency"


def test_host_single_and_empty_segments():
    d, _ = hand(ROWS, GROUP, 3, FLAGS, percentile=0.75)           # the slowest of four eligible trees alone: one row of group 0
    assert d.summary.tolist() == [4, 4, 1, 0]
    assert d.quantile[0].tolist() == [200, 200, 200] and d.quantile[9].tolist() == [200] * 3    # one item: every quantile is it
    assert d.quantile[1].tolist() == [EMPTY] * 3 and d.seg_count[1] == 0 and len(d.segment(0, 0, 1)) == 0
    d, _ = hand(ROWS, GROUP, 3, FLAGS, start_min=10 ** 6)         # nothing selected: every segment is empty
    assert d.summary.tolist() == [0, 0, 0, 0] and (d.quantile == EMPTY).all() and d.seg_off.tolist() == [0] * 11 and len(d.values) == 0


def test_host_cohorts_by_hand():
    # tree 0 holds labels 2 and 1: the smallest; tree 1 label 0 on its deepest row; tree 2 none: left out; tree 4 label 2
    label = [-1, 2, -1, 1, -1, 2, -1, -1, 0, -1, -1, 2]
    d, _ = hand(ROWS, GROUP, 3, FLAGS, label=label, n_cohorts=3)
    assert d.tree_cohort.tolist() == [1, 0, -1, -1, 2] and d.summary.tolist() == [33 - 4, 10 + 10 + 4, 3, 1]
    assert d.segment(0, 3).tolist() == [60] and d.segment(1, 3).tolist() == [100] and d.segment(2, 3).tolist() == [200]
    assert d.segment(1, 0, 1).tolist() == [30, 80] and d.segment(0, 0, 1).tolist() == [40] and len(d.segment(2, 0, 1)) == 0
    assert d.segment(2, 0, 0).tolist() == [200] and d.segment(0, 0, 0).tolist() == [60]     # tree 2's 10 is in no cohort
    one = d.cohort(1)
    assert one.n_cohorts == 1 and one.segment(0, 0, 1).tolist() == [30, 80] and one.summary.tolist() == [15, 10, 1, 3]
    assert one.seg_off[0] == 0 and np.array_equal(one.quantile, d.quantile[10:20])
    with pytest.raises(IndexError):
        d.segment(3, 0, 0)


def test_host_signed_order():
    rows = [(100, 50, -1), (200, 230, -1), (300, 300, -1)]        # a root with end < start: latency -50, duration 0
    d, _ = hand(rows, [0, 0, 0], 1, edges=[-50, 0])
    assert d.segment(0, 3).tolist() == [-50, 0, 30] and d.segment(0, 0, 0).tolist() == [0, 0, 30]
    assert d.hist[3].tolist() == [0, 1, 2] and d.quantile[3].tolist() == [-50, 0, 30]


# ---- 6. compare_distributions ---------------------------------------------------------------------------------------------
def test_compare_distributions():
    d, _ = hand(ROWS, GROUP, 3, FLAGS)
    c = traces.compare_distributions(d, d)
    assert (c["quantile_diff"] == 0).all() and (c["cdf_gap"][c["both"]] == 0).all() and c["both"].all()

    def one(values):                                              # a result of one group whose span latencies are `values`
        n = len(values)
        v = np.sort(np.array(values, dtype=np.int64))
        q = np.array([[v[min(n - 1, int(p * n))] for p in (0.5, 1.0)] if n else [EMPTY] * 2] + [[EMPTY] * 2] * 3)
        return traces.LatencyDistributions(np.zeros(0, np.int32), np.array([n, 0, 0, 0]), np.array([v.sum(), 0, 0, 0]), np.array([0, n, n, n, n]), v, q,
                                           np.zeros((4, 1), np.int64), [n, 1 if n else 0, 0, 0], 1, 1, (0.5, 1.0))

    # F_a = .25 .5 .75 1 1 1 and F_b = 0 0 .25 .5 .75 1 at 1 .. 6: the gap is .5 (at 2, 3 and 4)
    c = traces.compare_distributions(one([1, 2, 3, 4]), one([3, 4, 5, 6]))
    assert c["cdf_gap"][0] == 0.5 and c["quantile_diff"][0].tolist() == [2, 2] and c["both"].tolist() == [True, False, False, False]
    assert np.isnan(c["cdf_gap"][1:]).all() and (c["quantile_diff"][1:] == 0).all()
    # different sizes, ties: F_a = 2/3 2/3 1 and F_b = 0 1/2 1 at 5, 7, 9
    c = traces.compare_distributions(one([5, 5, 9]), one([7, 9]))
    assert c["cdf_gap"][0] == 2.0 / 3.0 and c["quantile_diff"][0].tolist() == [4, 0]
    assert np.isnan(traces.compare_distributions(one([1]), one([]))["cdf_gap"][0])
    with pytest.raises(ValueError):
        traces.compare_distributions(d, one([1]))


# ---- 2. device = restatement, invariants ----------------------------------------------------------------------------------
def check(eng, st, rows, group, n_groups, a, label=None, n_cohorts=1, probs=PROBS, edges=EDGES, tag=None):
    dev = eng.distributions(probs, edges)
    want = traces.distributions_host(st, a, rows[4], rows[5], group, n_groups, label, n_cohorts, probs, edges)
    for k in traces.LatencyDistributions.FIELDS:
        assert np.array_equal(getattr(dev, k), getattr(want, k)), (k, tag)
    G = n_groups
    assert np.array_equal(dev.hist.sum(axis=1), dev.seg_count) and np.array_equal(dev.seg_off, np.concatenate([[0], np.cumsum(dev.seg_count)]))
    inner = np.ones(max(dev.n_items - 1, 0), dtype=bool)
    inner[dev.seg_off[1:-1][(dev.seg_off[1:-1] > 0) & (dev.seg_off[1:-1] < dev.n_items)] - 1] = False
    assert np.all(np.diff(dev.values)[inner] >= 0)            # non-decreasing inside every segment
    if label is None:                                             # against the attribution of the same call
        assert np.array_equal(dev.seg_sum[0:G], a.group_span_time) and np.array_equal(dev.seg_count[0:G], a.group_span_rows)
        assert np.array_equal(dev.seg_count[G:2 * G], a.group_span_rows) and np.array_equal(dev.seg_sum[G:2 * G], a.group_self_time)
        assert np.array_equal(dev.seg_sum[2 * G:3 * G], a.group_path_time) and np.array_equal(dev.seg_count[2 * G:3 * G], a.group_path_rows)
        assert dev.seg_count[3 * G] == a.n_selected == dev.summary[2] and dev.summary[3] == 0
    else:
        assert dev.summary[2] + dev.summary[3] == a.n_selected
    t = eng.distributions_timing()
    assert set(t) == {"items", "sort", "quantiles"} and all(v >= 0 for v in t.values())
    return dev


def service_cohorts(table, rows, group, g):
    """Three cohorts taken from the rows of one service: label = start % 3 there, -1 elsewhere."""
    return np.where(group == g, np.asarray(rows[4]) % 3, -1).astype(np.int32)


def run_case(lib, tmp_path, name, seed, n, concurrency, expect):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    group, names = traces.groups_from_table(table)
    G = len(names)
    eng.set_row_groups(group, G)
    label = service_cohorts(table, rows, group, G - 1)
    seen = set()
    for kw in (dict(), dict(truth=True)):
        st = eng.stitch(**kw)
        for q in ta.queries(st, np.asarray(rows[4])):
            a = eng.attribute(**q)
            check(eng, st, rows, group, G, a, tag=(kw, q))
            eng.set_row_cohorts(label, 3)
            d = check(eng, st, rows, group, G, a, label, 3, tag=(kw, q, "cohorts"))
            seen.update(d.tree_cohort.tolist())
            eng.set_row_cohorts(None, 1)
    assert seen >= {0, 1, 2}
    eng.close()


# one case per corpus of test_stitch.CASES; its fifth is the hotel corpus again at 40 requests in flight, whose two passes take a
# minute on the device and whose forest has nothing the fanout case lacks (fragments, unassigned calls)
CASES = ts.CASES[:4]
assert [c[0] for c in CASES] == ["hotel", "media", "alibaba", "fanout"]


@pytest.mark.parametrize("name,seed,n,concurrency,expect", CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in CASES])
def test_device_equals_host_restatement(emu_lib, tmp_path, name, seed, n, concurrency, expect):
    run_case(emu_lib, tmp_path, name, seed, n, concurrency, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,n,concurrency,expect", CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in CASES])
def test_device_equals_host_restatement_gpu(tmp_path, name, seed, n, concurrency, expect):
    run_case(None, tmp_path, name, seed, n, concurrency, expect)


# ---- 3. both counting routes and the wavefront aggregation ------------------------------------------------------------------
def truth_engine(lib, units, n_traces, rows):
    """The true assignment handed over as pass 0: a forest without running a pass."""
    eng = Engine(0, lib_path=lib)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    eng.set_span_rows(*rows)
    eng.set_parents([u.true_parent for u in units])
    return eng


def run_routes(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "media", 7, 120, 6.0)
    rows = traces.rows_from_units(units, table)
    eng = truth_engine(lib, units, n_traces, rows)
    st = eng.stitch(0)
    n = len(table["service"])
    assert n >= 600
    label = (np.arange(n, dtype=np.int32) % 4) - 1
    # one group per row and a group that is not counted: 3094 segments, more than the LDS table of the HIP build (2048) holds
    many = (np.arange(n, dtype=np.int32) * 7) % 1031
    many[::5] = -1
    # a single group and a single cohort: all 64 lanes of a wavefront meet on one cell (4 segments: the LDS table of either build)
    single = np.zeros(n, dtype=np.int32)
    # 97 groups in turn: the 64 lanes of a wavefront lie in 64 different segments (292 segments: LDS in the HIP build)
    spread = (np.arange(n, dtype=np.int32) % 97).astype(np.int32)
    for group, G in ((many, 1031), (single, 1), (spread, 97)):
        eng.set_row_groups(group, G)
        for q in (EVERY, dict(percentile=0.5)):
            a = eng.attribute(**q)
            d = check(eng, st, rows, group, G, a, tag=(G, q))
            if q is EVERY:
                assert d.summary[2] == st.n_trees and d.n_items >= 2 * int((group >= 0).sum())
            eng.set_row_cohorts(label, 3)
            check(eng, st, rows, group, G, a, label, 3, tag=(G, q, "cohorts"))
            eng.set_row_cohorts(None, 1)
    eng.close()


def test_counting_routes(emu_lib, tmp_path):
    run_routes(emu_lib, tmp_path)


@pytest.mark.gpu
def test_counting_routes_gpu(tmp_path):
    run_routes(None, tmp_path)


def run_lanes(lib, queries=(EVERY, dict(percentile=0.5))):
    """A hand-built table of 300 rows, a few hundred single-row trees and one tree of 42: a single group (every lane of a wavefront
    on one cell), 97 groups in turn (every lane in another segment), with and without cohorts."""
    extra = [(1000 + 7 * i, 1000 + 7 * i + (i * 37) % 1500, False) for i in range(256)] + [(100 + 150 * i, 100 + 150 * i + 90 + i, True) for i in range(40)]
    n = 4 + len(extra)
    label = (np.arange(n, dtype=np.int32) % 4) - 1
    eng, st, rows, _ = hand_engine(lib, extra, np.zeros(n, dtype=np.int32), 1)
    for group, G in ((np.zeros(n, dtype=np.int32), 1), ((np.arange(n, dtype=np.int32) % 97).astype(np.int32), 97)):
        eng.set_row_groups(group, G)
        for q in queries:
            a = eng.attribute(**q)
            check(eng, st, rows, group, G, a, tag=(G, q))
            eng.set_row_cohorts(label, 3)
            check(eng, st, rows, group, G, a, label, 3, tag=(G, q, "cohorts"))
            eng.set_row_cohorts(None, 1)
    eng.close()


def test_wavefront_aggregation_lane_threaded(emu_lib):
    """One host thread per lane (TW_EMU_LANES=1, workgroups of 256): the ballots, shuffles and leaders' adds of k_dist_items run
    as they are written, 64 lanes to a wavefront, without a GPU."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "import test_distributions as t\n"
            "t.run_lanes(%r, (t.EVERY,))\n"
            "print('lanes ok')\n") % (os.path.dirname(here), here, emu_lib)
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "lanes ok" in out.stdout, out.stderr[-2000:]


@pytest.mark.gpu
def test_wavefront_aggregation_gpu():
    run_lanes(None)


# ---- 4. key width -------------------------------------------------------------------------------------------------------------
def hand_engine(lib, extra, group, n_groups):
    """A table written out by hand in the manner of test_attribute.run_large_tree: rows 0, 1 two requests, 2, 3 their calls, then
    `extra` = (start, end, callee of call 0?) server spans: callees of the first request's call, or roots of trees of their own."""
    u, tp = synth.make_unit(3, 2, shape="single")
    c0, c1 = 2 + int(tp[0][0]), 2 + int(tp[0][1])
    n = len(extra)
    start, end = np.zeros(4 + n, dtype=np.int64), np.zeros(4 + n, dtype=np.int64)
    start[[0, 1, c0, c1]], end[[0, 1, c0, c1]] = [0, 5, 10, 6], [100000, 50, 99990, 40]
    start[4:], end[4:] = [x[0] for x in extra], [x[1] for x in extra]
    row_link = np.array([-1, -1, -1, -1] + [c0 if x[2] else -1 for x in extra], dtype=np.int32)
    kind = np.array([1, 1, 2, 2] + [1] * n, dtype=np.uint8)
    rows = ([np.array([0, 1], dtype=np.int32)], [[np.array([2, 3], dtype=np.int32)]], row_link, kind, start, end)
    eng = Engine(0, lib_path=lib)
    eng.load([u])
    eng.set_span_rows(*rows)
    eng.set_parents([tp])
    group = np.asarray(group, dtype=np.int32)
    eng.set_row_groups(group, n_groups)
    st = eng.stitch(0)
    return eng, st, rows, group


def run_key_width(lib):
    # durations up to 2^60 and a negative trace latency: 61 value bits, and 10 segments need 4: the two-pass sort
    big = 1 << 60
    extra = [(1000 + 7 * i, 1000 + 7 * i + (big >> (i % 50)), False) for i in range(150)] + [(500, 100, False), (700, 650, False)] + \
            [(100 + 150 * i, 100 + 150 * i + 90, True) for i in range(40)]
    group = (np.arange(4 + len(extra)) % 3).astype(np.int32)
    eng, st, rows, group = hand_engine(lib, extra, group, 3)
    a = eng.attribute()
    assert a.n_selected == st.n_trees == 154 and st.tree_latency.min() == -400
    edges = [-400, -399, 0, 1, 1 << 30, big - 1, big]
    d = check(eng, st, rows, group, 3, a, edges=edges)
    assert d.segment(0, 3)[:3].tolist() == [-400, -50, 45] and d.segment(0, 3)[-1] == big and d.hist[9][0] == 0 and d.hist[9][1] == 1
    label = (np.arange(4 + len(extra)) % 3 - 1).astype(np.int32)
    eng.set_row_cohorts(label, 2)
    check(eng, st, rows, group, 3, a, label, 2, edges=edges)
    eng.close()
    # the same shape with small values: 10 segments and 11 value bits in one key; the signed order across zero
    extra = [(1000 + 7 * i, 1000 + 7 * i + (i * 37) % 1500, False) for i in range(150)] + [(500, 100, False), (700, 650, False)]
    group = (np.arange(4 + len(extra)) % 3).astype(np.int32)
    eng, st, rows, group = hand_engine(lib, extra, group, 3)
    d = check(eng, st, rows, group, 3, eng.attribute(), edges=[-400, 0, 1])
    assert d.segment(0, 3)[:2].tolist() == [-400, -50] and d.hist[9][:2].tolist() == [0, 2]
    # every value the same: a key without value bits
    extra = [(1000 + 7 * i, 1000 + 7 * i + 5, False) for i in range(70)]
    eng2, st2, rows2, group2 = hand_engine(lib, extra, np.zeros(74, dtype=np.int32), 1)
    a2 = eng2.attribute(start_min=1000)
    d = check(eng2, st2, rows2, group2, 1, a2)
    assert d.values.tolist() == [5] * 280
    eng.close()
    eng2.close()


def test_key_width(emu_lib):
    run_key_width(emu_lib)


@pytest.mark.gpu
def test_key_width_gpu():
    run_key_width(None)


# ---- 5. state and argument errors -------------------------------------------------------------------------------------------
def run_errors(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table)
    G = len(names)
    label = service_cohorts(table, rows, group, 0)
    eng = Engine(0, lib_path=lib)

    def error(code, f, *a, **kw):
        with pytest.raises(EngineError) as ex:
            f(*a, **kw)
        assert ex.value.code == code and {-4: "TW_ERR_STATE", -1: "TW_ERR_ARG", -2: "TW_ERR_UNSUPPORTED"}[code] in str(ex.value)

    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    eng._n_rows = len(group)
    error(-4, eng.set_row_cohorts, label, 3)                      # before set_span_rows
    eng.set_span_rows(*rows)
    eng.set_parents([u.true_parent for u in units])
    eng.set_row_groups(group, G)
    error(-4, eng.distributions)                                  # before a stitch
    st = eng.stitch(0)
    error(-4, eng.distributions)                                  # before attribute()
    a = eng.attribute()
    full = check(eng, st, rows, group, G, a)
    eng.stitch(0)                                                 # a second stitch drops the attribution
    error(-4, eng.distributions)
    a = eng.attribute(percentile=0.5)                             # ... and after attribute() it works again, on the new selection
    half = check(eng, st, rows, group, G, a)
    assert half.summary[2] == n_traces - n_traces // 2 < full.summary[2] == n_traces
    assert half.segment(0, 3)[0] >= np.median(full.segment(0, 3)) and half.segment(0, 3)[-1] == full.segment(0, 3)[-1]
    for bad in ((-0.1,), (1.5,), (0.5, float("nan")), [0.5] * 33):
        error(-1, eng.distributions, bad)
    for bad in ((3, 3), (5, 4), list(range(64))):
        error(-1, eng.distributions, (0.5,), bad)
    assert eng.distributions((), list(range(63))).hist.shape == (3 * G + 1, 64)     # no probs, 63 edges: the limits are allowed
    for value in (3, -2):
        x = label.copy()
        x[3] = value
        error(-1, eng.set_row_cohorts, x, 3)
    error(-1, eng.set_row_cohorts, label, 0)
    error(-1, eng.set_row_cohorts, None, 2)
    with pytest.raises(ValueError):
        eng.set_row_cohorts(label[:-1], 3)
    check(eng, st, rows, group, G, a)                             # a refused call leaves everything as it was
    eng.set_row_cohorts(label, 3)
    check(eng, st, rows, group, G, a, label, 3)
    eng.set_row_cohorts(np.full(len(group), -1, dtype=np.int32), (1 << 24) // (3 * G + 1) + 1)
    error(-2, eng.distributions)                                  # more than 2^24 segments
    eng.set_row_cohorts(None, 1)
    check(eng, st, rows, group, G, a)
    eng.set_row_groups(group, G)                                  # new groups drop the attribution
    error(-4, eng.distributions)
    eng.attribute()
    eng.set_row_cohorts(label, 3)
    eng.set_span_rows(*rows)                                      # new row maps drop the forest, the groups and the labels
    error(-4, eng.distributions)
    eng.set_row_groups(group, G)
    st = eng.stitch(0)
    check(eng, st, rows, group, G, eng.attribute())               # (one cohort again)
    eng.run_pass1()                                               # a new pass drops the forest
    error(-4, eng.distributions)
    eng.load([u.arrays for u in units])                           # a load drops everything
    error(-4, eng.distributions)
    eng.close()


def test_state_and_argument_errors(emu_lib, tmp_path):
    run_errors(emu_lib, tmp_path)


@pytest.mark.gpu
def test_state_and_argument_errors_gpu(tmp_path):
    run_errors(None, tmp_path)   # (all refused on the host: nothing malformed reaches the device)


# ---- 7. the command line ----------------------------------------------------------------------------------------------------
def test_cli_latency_out(emu_lib, tmp_path, capsys):
    from traceweaver_amd import executor
    from traceweaver_amd.ingest import open_directory

    synth.write_jaeger_corpus(str(tmp_path / "corpus"), 11, 400, app=synth.HOTEL_APP, concurrency=2.5)
    runs, text = {}, {}
    lat = ["--latency_out", str(tmp_path / "lat.npz"), "--query_percentile", "0.9", "--quantiles", "0.5,0.9,1"]
    for tag, extra in (("plain", []), ("alone", lat), ("both", lat[:1] + [str(tmp_path / "both.npz")] + lat[2:] + ["--attribute_out", str(tmp_path / "attr.npz"), "-v"]),
                       ("cohorts", lat[:1] + [str(tmp_path / "cohorts.npz")] + lat[2:] + ["--cohort_service", "search"])):
        out = str(tmp_path / tag) + "/"
        executor.main(["--absolute_path", str(tmp_path / "corpus"), "--cache_rate", "0", "--fix", "2", "--results_directory", out,
                       "--test_name", "gen", "--load_level", "7", "--engine_library", emu_lib] + extra)
        runs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        text[tag] = capsys.readouterr().out
    assert len(runs["plain"]) == 5 and runs["plain"] == runs["alone"] == runs["both"] == runs["cohorts"]    # the five pickles, byte for byte
    assert "Latency distributions" not in text["plain"] and "Delay culprit" not in text["alone"] and "Delay culprit:" in text["both"]
    z, both, attr = np.load(str(tmp_path / "lat.npz")), np.load(str(tmp_path / "both.npz")), np.load(str(tmp_path / "attr.npz"))
    assert all(np.array_equal(z[k], both[k]) for k in z.files)
    assert z["probs"].tolist() == [0.5, 0.9, 1.0] and z["metrics"].tolist() == list(traces.METRICS) and z["group_names"].tolist() == attr["group_names"].tolist()
    # the same engine calls by hand
    corpus, _ = open_directory(str(tmp_path / "corpus"), lib_path=emu_lib, first_span=synth.HOTEL_APP["root_op"], fix=None, cache=False)
    units, skipped, n_traces = corpus.units()
    table = corpus.span_table()
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(emu_lib, units, n_traces, rows)
    group, names = traces.groups_from_table(table, corpus)
    eng.set_row_groups(group, len(names))
    st = eng.stitch()
    a = eng.attribute(percentile=0.9)
    d = eng.distributions((0.5, 0.9, 1.0))
    for k in traces.LatencyDistributions.FIELDS:
        assert np.array_equal(z[k], getattr(d, k)), k
    G, g = len(names), int(attr["summary"][4])
    assert np.array_equal(z["seg_sum"][:G], attr["groups"][3]) and np.array_equal(z["seg_count"][:G], attr["groups"][4])
    line = [x for x in text["both"].splitlines() if x.startswith("Culprit span latency:")]
    assert line == ["Culprit span latency: p50 %d us, p90 %d us, p100 %d us over %d spans" % (tuple(z["quantile"][g]) + (z["seg_count"][g],))]
    assert len([x for x in text["both"].splitlines() if x.startswith("Culprit span latency (true traces):")]) == 1
    assert "Latency distributions: %d values in %d segments over %d traces (0 without a cohort)" % tuple(z["summary"][:3]) in text["alone"]
    # cohorts: the rows of `search` labelled by their operation's index
    c = np.load(str(tmp_path / "cohorts.npz"))
    of = group == names.index("search")
    ops, inverse = np.unique(table["op_name"][of], return_inverse=True)
    label = np.full(len(group), -1, dtype=np.int32)
    label[of] = inverse
    eng.set_row_cohorts(label, len(ops))
    d = eng.distributions((0.5, 0.9, 1.0))
    assert c["n_cohorts"] == len(ops) and all(np.array_equal(c[k], getattr(d, k)) for k in traces.LatencyDistributions.FIELDS)
    eng.close()
    base = ["--absolute_path", "x", "--fix", "2", "--results_directory", str(tmp_path) + "/", "--engine_library", emu_lib, "--latency_out", "l.npz"]
    for extra in (["--cache_rate", "0.1"], ["--cache_rate", "0", "--predictor_indices", "3"], ["--cache_rate", "0", "--query_percentile", "1"],
                  ["--cache_rate", "0", "--quantiles", "0.5,1.5"], ["--cache_rate", "0", "--quantiles", "a"]):
        with pytest.raises(SystemExit):
            executor.main(base + extra)
    with pytest.raises(SystemExit):
        executor.main(base[:-2] + ["--cache_rate", "0", "--cohort_service", "search"])
    with pytest.raises(SystemExit):                                # a service the table does not hold
        executor.main(["--absolute_path", str(tmp_path / "corpus"), "--cache_rate", "0", "--fix", "2", "--results_directory", str(tmp_path / "no") + "/",
                       "--test_name", "gen", "--load_level", "7", "--engine_library", emu_lib, "--latency_out", str(tmp_path / "no.npz"),
                       "--cohort_service", "nowhere"])
