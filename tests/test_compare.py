"""Engine.compare_cohorts (tw_compare_cohorts, csrc/tw_cmp.h): two cohorts of the latency distributions compared segment by
segment -- the two-sample KS gap and where it lies, twice the Mann-Whitney U, quantile shifts, and a permutation test of all
three.  The yardstick is traces.compare_cohorts_host, the definitions of include/traceweaver_amd.h restated in plain Python
integers; parts 1 to 3 check it by hand, against scipy and for the permutation rule, the rest compares the device with it,
np.array_equal on every field of CohortComparison.FIELDS.  Corpora, cases and helpers are those of tests/test_distributions.py.
CPU tier: host-emulation build (one lane per workgroup, and once one host thread per lane); the HIP library under -m gpu.

Not reached by any test: the two size limits of TW_ERR_UNSUPPORTED (n_a n_b >= 2^61, N >= 2^32) need segments of 2^31 items."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_attribute as ta  # noqa: F401  (test_distributions imports it by this name)
import test_distributions as td
import test_stitch as ts
from traceweaver_amd import synth, traces
from traceweaver_amd.engine import Engine, EngineError

EMPTY = np.iinfo(np.int64).min
PAIRS = ((0, 1), (0, 2), (2, 1))
PROBS = (0.5, 0.95, 1.0)


def lists(cohorts, probs=(0.5, 1.0)):
    """A LatencyDistributions of one group whose span latencies are `cohorts[c]`, every other segment empty."""
    count, values, quant = [], [], []
    for x in cohorts:
        v = sorted(int(y) for y in x)
        count += [len(v), 0, 0, 0]
        values += v
        quant += [[v[min(len(v) - 1, int(p * len(v)))] for p in probs] if v else [EMPTY] * len(probs)] + [[EMPTY] * len(probs)] * 3
    count = np.array(count, dtype=np.int64)
    return traces.LatencyDistributions(np.zeros(0, np.int32), count, np.zeros(len(count), np.int64), np.concatenate([[0], np.cumsum(count)]).astype(np.int64),
                                       np.array(values, dtype=np.int64), np.array(quant, dtype=np.int64).reshape(len(count), len(probs)),
                                       np.zeros((len(count), 1), np.int64), [len(values), int((count > 0).sum()), 0, 0], len(cohorts), 1, probs)


# ---- 1. the restatement by hand -------------------------------------------------------------------------------------------
def test_host_by_hand():
    c = traces.compare_cohorts_host(lists([[1, 2, 3, 4], [3, 4, 5, 6]]), ((0, 1),), (0.5, 1.0))
    r = c.row(0, "span_latency", 0)
    # g = 4 8 8 8 4 0 at 1 .. 6: the greatest first at 2; A below B 13 times, equal twice
    assert (c.n_a[r], c.n_b[r], c.ks_gap[r], c.ks_at[r], c.u2[r]) == (4, 4, 8, 2, 28) and c.quantile_shift[r].tolist() == [2, 2]
    assert c.ks()[r] == 0.5 and c.superiority()[r] == 28 / 32.0 and c.summary.tolist() == [1, 0, 0, 0]
    assert (c.perm_ge_ks == -1).all() and (c.perm_ge_q == -1).all() and np.isnan(c.p_value("ks")).all()
    # the other way round: the gap and the shifts change sign, u2 = 2 n_a n_b - u2
    back = traces.compare_cohorts_host(lists([[1, 2, 3, 4], [3, 4, 5, 6]]), ((1, 0),), (0.5, 1.0))
    assert (back.ks_gap[r], back.ks_at[r], back.u2[r]) == (-8, 2, 4) and back.quantile_shift[r].tolist() == [-2, -2]
    # different sizes, ties: g = 4 1 0 at 5, 7, 9
    c = traces.compare_cohorts_host(lists([[5, 5, 9], [7, 9]]), ((0, 1),), (0.5, 1.0))
    assert (c.ks_gap[r], c.ks_at[r], c.u2[r]) == (4, 5, 9) and c.quantile_shift[r].tolist() == [4, 0]
    # the empty segments of that layout, and an empty side
    for k in (1, 2, 3):
        assert (c.n_a[k], c.n_b[k], c.ks_gap[k], c.ks_at[k], c.u2[k]) == (0, 0, 0, EMPTY, 0) and (c.quantile_shift[k] == 0).all()
    c = traces.compare_cohorts_host(lists([[1, 2], []]), ((0, 1),), (0.5,), permutations=5)
    assert (c.n_a[r], c.n_b[r], c.ks_gap[r], c.ks_at[r], c.u2[r]) == (2, 0, 0, EMPTY, 0) and c.quantile_shift[r].tolist() == [0]
    assert c.perm_ge_ks[r] == c.perm_ge_u[r] == -1 and c.perm_ge_q[r].tolist() == [-1] and np.isnan(c.ks()[r]) and np.isnan(c.superiority()[r])
    assert c.summary.tolist() == [0, 0, 0, 5] and c.table() == []
    with pytest.raises(IndexError):
        c.row(1, 0, 0)


def test_host_signed_order():
    # roots of their own: latencies -50 and 30 in cohort 0, 0 and 10 in cohort 1 (a root with end < start: duration 0)
    rows = [(100, 50, -1), (200, 230, -1), (300, 300, -1), (400, 410, -1)]
    d, _ = td.hand(rows, [0, 0, 0, 0], 1, label=[0, 0, 1, 1], n_cohorts=2)
    c = traces.compare_cohorts_host(d, ((0, 1),), (0.0, 1.0))
    r = c.row(0, "trace_latency")
    # g = 2 0 -2 0 at -50, 0, 10, 30: the first of the two greatest is the negative value
    assert (c.ks_gap[r], c.ks_at[r], c.u2[r]) == (2, -50, 4) and c.quantile_shift[r].tolist() == [50, -20]
    r = c.row(0, 0, 0)                                            # durations 0, 30 against 0, 10: g = 0 -2 0
    assert (c.ks_gap[r], c.ks_at[r], c.u2[r]) == (-2, 10, 3)
    t = c.table(["svc"])
    assert len(t) == 4 and t[0]["group"] == "svc" and t[3]["group"] is None and t[3]["ks"] == 0.5 and t[3]["shift_p100"] == -20 and "p_ks" not in t[3]


# ---- 2. the restatement against scipy -------------------------------------------------------------------------------------
def test_host_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.RandomState(17)
    for _ in range(200):
        A = rng.randint(0, 30, size=rng.randint(1, 40)).tolist()
        B = (rng.randint(0, 30, size=rng.randint(1, 40)) + rng.randint(0, 8)).tolist()
        d = lists([A, B])
        c = traces.compare_cohorts_host(d, ((0, 1),), (0.5, 1.0))
        assert abs(abs(int(c.ks_gap[0])) / float(len(A) * len(B)) - stats.ks_2samp(A, B).statistic) <= 1e-12
        assert c.u2[0] == 2 * stats.mannwhitneyu(B, A, method="asymptotic").statistic
        gap = traces.compare_distributions(d.cohort(0), d.cohort(1))
        assert abs(c.ks()[0] - gap["cdf_gap"][0]) <= 1e-12 and np.array_equal(c.quantile_shift[0], gap["quantile_diff"][0])


# ---- 3. the permutation rule ----------------------------------------------------------------------------------------------
def test_permutation_labels():
    for N, n_a in ((1, 1), (2, 1), (7, 0), (7, 7), (9, 4), (64, 20), (65, 64)):
        for p in range(20):
            x = traces.permutation_labels_host(N, n_a, 3, 5, p)
            assert len(x) == N and x.count(0) == n_a and set(x) <= {0, 1}
    seen = {}
    for p in range(6000):
        x = tuple(traces.permutation_labels_host(4, 2, 11, 0, p))
        seen[x] = seen.get(x, 0) + 1
    # 6 subsets, 1000 expected each, standard deviation 29: three and a half of them
    assert len(seen) == 6 and all(900 <= v <= 1100 for v in seen.values()), seen
    assert traces.permutation_labels_host(9, 4, 3, 5, 0) != traces.permutation_labels_host(9, 4, 3, 6, 0) or \
        traces.permutation_labels_host(9, 4, 3, 5, 1) != traces.permutation_labels_host(9, 4, 3, 6, 1)        # rows draw independently


def test_permutation_counts():
    rng = np.random.RandomState(2)
    same = traces.compare_cohorts_host(lists([rng.randint(0, 1000, 300), rng.randint(0, 1000, 200)]), ((0, 1),), (0.5,), permutations=200, seed=1)
    assert 10 < same.perm_ge_ks[0] < 190 and 10 < same.perm_ge_u[0] < 190 and same.summary.tolist() == [1, 1, 500, 200]
    moved = traces.compare_cohorts_host(lists([rng.randint(0, 1000, 300), rng.randint(0, 1000, 200) + 150]), ((0, 1),), (0.5,), permutations=200, seed=1)
    assert moved.perm_ge_ks[0] == moved.perm_ge_u[0] == 0 and moved.ks_gap[0] > 0 and moved.superiority()[0] > 0.5
    assert moved.p_value("ks")[0] == 1.0 / 201.0 and 0 < same.p_value(0)[0] <= 1.0
    row = moved.table()[0]
    assert row["pair"] == (0, 1) and row["p_ks"] == 1.0 / 201.0 and row["p_u"] == 1.0 / 201.0 and "p_shift_p50" in row
    small = traces.compare_cohorts_host(lists([[1, 2, 3], [2, 3, 4]]), ((0, 1),), (0.5,), permutations=10, max_pool=5)
    assert small.perm_ge_ks[0] == -1 and small.summary.tolist() == [1, 0, 0, 10]


# ---- 4. device = restatement ----------------------------------------------------------------------------------------------
def same(dev, want, tag=None):
    for k in traces.CohortComparison.FIELDS:
        assert np.array_equal(getattr(dev, k), getattr(want, k)), (k, tag)
    assert dev.same_as(want)


def check(eng, pairs=PAIRS, probs=PROBS, permutations=0, seed=0, max_pool=0, d=None, tag=None):
    dev = eng.compare_cohorts(pairs, probs, permutations, seed, max_pool)
    d = eng.distributions(probs) if d is None else d
    same(dev, traces.compare_cohorts_host(d, pairs, probs, permutations, seed, max_pool), tag)
    t = eng.compare_timing()
    assert set(t) == {"observed", "permutations"} and all(v >= 0 for v in t.values())
    return dev


def run_case(lib, tmp_path, name, seed, n, concurrency, expect):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    group, names = traces.groups_from_table(table)
    G = len(names)
    eng.set_row_groups(group, G)
    eng.set_row_cohorts(td.service_cohorts(table, rows, group, G - 1), 3)
    eng.stitch()
    eng.attribute(**td.EVERY)
    d = eng.distributions(PROBS)
    full = check(eng, permutations=70, seed=5, d=d, tag=name)
    assert full.summary[0] == full.summary[1] > 0 and full.summary[3] == 70 and ((full.perm_ge_ks >= 0) == ((full.n_a > 0) & (full.n_b > 0))).all()
    assert (full.perm_ge_ks <= 70).all() and (full.perm_ge_q <= 70).all()
    pooled = np.sort((full.n_a + full.n_b)[(full.n_a > 0) & (full.n_b > 0)])
    limit = int(pooled[len(pooled) // 2])
    assert pooled[0] <= limit < pooled[-1]
    part = check(eng, permutations=70, seed=5, max_pool=limit, d=d, tag=(name, "max_pool"))
    both = (part.n_a > 0) & (part.n_b > 0)
    assert (both & (part.perm_ge_ks >= 0)).any() and (both & (part.perm_ge_ks < 0)).any() and 0 < part.summary[1] < part.summary[0]
    assert np.array_equal(part.perm_ge_ks[part.perm_ge_ks >= 0], full.perm_ge_ks[part.perm_ge_ks >= 0])     # rows draw independently
    assert eng.distributions(PROBS).same_as(d)
    eng.close()


@pytest.mark.parametrize("name,seed,n,concurrency,expect", td.CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in td.CASES])
def test_device_equals_host_restatement(emu_lib, tmp_path, name, seed, n, concurrency, expect):
    run_case(emu_lib, tmp_path, name, seed, n, concurrency, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,n,concurrency,expect", td.CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in td.CASES])
def test_device_equals_host_restatement_gpu(tmp_path, name, seed, n, concurrency, expect):
    run_case(None, tmp_path, name, seed, n, concurrency, expect)


# ---- 5. edge shapes on a table written out by hand --------------------------------------------------------------------------
def run_edges(lib):
    # one item against one: two roots of their own, one in either cohort (the table's first four rows say nothing)
    eng, st, rows, group = td.hand_engine(lib, [(1000, 1010, False), (2000, 2030, False)], np.zeros(6, dtype=np.int32), 1)
    eng.set_row_cohorts(np.array([-1, -1, -1, -1, 0, 1], dtype=np.int32), 2)
    eng.attribute(**td.EVERY)
    c = check(eng, ((0, 1), (1, 0)), (0.0, 0.5, 1.0), permutations=65, seed=3)
    assert c.n_a.tolist() == [1] * 8 and c.ks_gap.tolist() == [1] * 4 + [-1] * 4 and c.ks_at.tolist() == [10] * 8 and c.u2.tolist() == [2] * 4 + [0] * 4
    assert (c.quantile_shift[:4] == 20).all() and (c.quantile_shift[4:] == -20).all() and (c.perm_ge_ks == 65).all() and (c.perm_ge_u == 65).all()
    eng.close()
    # every value the same on both sides: one run
    n = 4 + 70
    eng, st, rows, group = td.hand_engine(lib, [(1000 + 7 * i, 1000 + 7 * i + 5, False) for i in range(70)], np.zeros(n, dtype=np.int32), 1)
    eng.set_row_cohorts(np.array([-1] * 4 + [i % 2 for i in range(70)], dtype=np.int32), 2)
    eng.attribute(start_min=1000, **td.EVERY)
    c = check(eng, ((0, 1),), PROBS, permutations=64, seed=9)
    assert c.n_a.tolist() == [35] * 4 and c.ks_gap.tolist() == [0] * 4 and c.ks_at.tolist() == [5] * 4 and c.u2.tolist() == [35 * 35] * 4
    assert (c.perm_ge_ks == 64).all() and (c.perm_ge_q == 64).all() and (c.quantile_shift == 0).all()
    eng.close()
    # a few hundred rows in two groups, group 1 absent from cohort 1; n_perm of 1, 64 and 65; one cohort more that nobody is in
    extra = [(1000 + 7 * i, 1000 + 7 * i + (i * 37) % 1500, False) for i in range(256)] + [(100 + 150 * i, 100 + 150 * i + 90 + i, True) for i in range(40)]
    n = 4 + len(extra)
    label = (np.arange(n, dtype=np.int32) % 3) - 1
    group = np.where(label == 1, 0, np.arange(n) % 2).astype(np.int32)
    eng, st, rows, group = td.hand_engine(lib, extra, group, 2)
    eng.set_row_cohorts(label, 3)
    eng.attribute(**td.EVERY)
    d = eng.distributions(PROBS)
    for n_perm in (1, 64, 65):
        c = check(eng, ((0, 1), (1, 2)), PROBS, permutations=n_perm, seed=7, d=d, tag=n_perm)
        r = c.row(0, 0, 1)
        assert c.n_a[r] > 0 and c.n_b[r] == 0 and c.ks_at[r] == EMPTY and c.perm_ge_ks[r] == -1 and c.summary[3] == n_perm
        assert (c.n_b[c.row(1, 0, 0):] == 0).all() and (c.perm_ge_u[c.row(1, 0, 0):] == -1).all()
        assert c.summary[0] == c.summary[1] == int(((c.n_a > 0) & (c.n_b > 0)).sum()) >= 4
    check(eng, ((0, 1),), (), permutations=3, d=d)                # no probs
    eng.close()
    # durations up to 2^60 beside a negative trace latency
    big = 1 << 60
    extra = [(1000 + 7 * i, 1000 + 7 * i + (big >> (i % 50)), False) for i in range(150)] + [(500, 100, False), (700, 650, False)] + \
            [(100 + 150 * i, 100 + 150 * i + 90, True) for i in range(40)]
    n = 4 + len(extra)
    eng, st, rows, group = td.hand_engine(lib, extra, (np.arange(n) % 3).astype(np.int32), 3)
    eng.set_row_cohorts((np.arange(n) % 3 - 1).astype(np.int32), 2)
    a = eng.attribute()
    c = check(eng, ((0, 1), (1, 0)), (0.0, 0.5, 1.0), permutations=65, seed=1)
    assert a.n_selected == st.n_trees and st.tree_latency.min() == -400 and np.abs(c.quantile_shift).max() > (1 << 40) and c.summary[0] == c.summary[1] > 0
    eng.close()


def test_edge_shapes(emu_lib):
    run_edges(emu_lib)


def test_edge_shapes_lane_threaded(emu_lib):
    """One host thread per lane (TW_EMU_LANES=1, workgroups of 256): the ballots, shuffles and leaders' atomics of the rank kernels
    and the 64 permutations of a wavefront of k_cmp_perm run as they are written, without a GPU."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "import test_compare as t\n"
            "t.run_edges(%r)\n"
            "print('lanes ok')\n") % (os.path.dirname(here), here, emu_lib)
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "lanes ok" in out.stdout, out.stderr[-2000:]


@pytest.mark.gpu
def test_edge_shapes_gpu():
    run_edges(None)


# ---- 6. state and arguments -------------------------------------------------------------------------------------------------
def run_errors(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table)
    G = len(names)
    label = td.service_cohorts(table, rows, group, G - 1)
    eng = td.truth_engine(lib, units, n_traces, rows)

    def error(code, *a, **kw):
        with pytest.raises(EngineError) as ex:
            eng.compare_cohorts(*a, **kw)
        assert ex.value.code == code and {-4: "TW_ERR_STATE", -1: "TW_ERR_ARG", -2: "TW_ERR_UNSUPPORTED"}[code] in str(ex.value)

    eng.set_row_groups(group, G)
    eng.set_row_cohorts(label, 3)
    error(-4)                                                     # before a stitch
    eng.stitch(0)
    error(-4)                                                     # before attribute()
    eng.attribute(**td.EVERY)
    first = check(eng, permutations=20, seed=4)                   # builds the items itself
    before = eng.distributions(PROBS)
    again = eng.compare_cohorts(PAIRS, PROBS, 20, 4)
    same(again, first)                                            # two calls in a row
    assert eng.distributions(PROBS).same_as(before)
    other = eng.compare_cohorts(PAIRS, PROBS, 20, 5)              # another seed: other draws, the same observed statistics
    assert all(np.array_equal(getattr(other, k), getattr(first, k)) for k in ("n_a", "n_b", "ks_gap", "ks_at", "u2", "quantile_shift"))
    assert any(not np.array_equal(getattr(other, k), getattr(first, k)) for k in ("perm_ge_ks", "perm_ge_u", "perm_ge_q"))
    for bad in ((), [(0, 1)] * 65, ((0, 3),), ((-1, 0),), ((1, 1),)):
        error(-1, bad)
    for bad in ((-0.1,), (1.5,), (0.5, float("nan")), [0.5] * 9):
        error(-1, PAIRS, bad)
    error(-1, PAIRS, PROBS, -1)
    error(-1, PAIRS, PROBS, 65537)
    error(-1, PAIRS, PROBS, 5, 0, -1)
    with pytest.raises(ValueError):
        eng.compare_cohorts((0, 1, 2))
    same(eng.compare_cohorts(PAIRS, PROBS, 20, 4), first)         # a refused call leaves everything as it was
    assert eng.compare_cohorts([(0, 1)] * 64, [0.5] * 8, 0).quantile_shift.shape == (64 * (3 * G + 1), 8)     # the limits are allowed
    eng.set_row_cohorts(np.where(label < 0, -1, (label + 1) % 3).astype(np.int32), 3)     # 0 1 2 -> 1 2 0, -1 stays
    moved = check(eng, permutations=0)                            # the comparison follows the new labels
    assert not np.array_equal(moved.n_a, first.n_a) and (moved.perm_ge_ks == -1).all() and moved.summary[1:].tolist() == [0, 0, 0]
    eng.set_row_cohorts(np.full(len(group), -1, dtype=np.int32), (1 << 24) // (3 * G + 1) + 1)
    error(-2)                                                     # more than 2^24 segments
    eng.set_row_cohorts(None, 1)
    error(-1)                                                     # one cohort: every pair names a label outside it
    eng.set_row_cohorts(label, 3)
    same(eng.compare_cohorts(PAIRS, PROBS, 20, 4), first)
    eng.stitch(0)                                                 # a new stitch drops the attribution
    error(-4)
    eng.attribute(**td.EVERY)
    same(eng.compare_cohorts(PAIRS, PROBS, 20, 4), first)
    eng.load([u.arrays for u in units])                           # a load drops everything
    error(-4)
    eng.close()


def test_state_and_argument_errors(emu_lib, tmp_path):
    run_errors(emu_lib, tmp_path)


@pytest.mark.gpu
def test_state_and_argument_errors_gpu(tmp_path):
    run_errors(None, tmp_path)   # (all refused on the host: nothing malformed reaches the device)


# ---- 7. the command line ----------------------------------------------------------------------------------------------------
def test_cli_compare_out(emu_lib, tmp_path, capsys):
    from traceweaver_amd import executor
    from traceweaver_amd.ingest import open_directory

    synth.write_jaeger_corpus(str(tmp_path / "corpus"), 11, 400, app=synth.HOTEL_APP, concurrency=2.5)
    runs, text = {}, {}
    lat = ["--query_percentile", "0.5", "--quantiles", "0.5,0.9,1", "--cohort_service", "search"]
    cmp_flags = ["--compare_out", str(tmp_path / "cmp.npz"), "--compare_pairs", "0,1;1,0", "--permutations", "30", "--compare_seed", "8"]
    for tag, extra in (("plain", lat + ["--latency_out", str(tmp_path / "lat.npz")]),
                       ("compare", lat + ["--latency_out", str(tmp_path / "lat2.npz"), "--attribute_out", str(tmp_path / "attr.npz")] + cmp_flags)):
        out = str(tmp_path / tag) + "/"
        executor.main(["--absolute_path", str(tmp_path / "corpus"), "--cache_rate", "0", "--fix", "2", "--results_directory", out,
                       "--test_name", "gen", "--load_level", "7", "--engine_library", emu_lib] + extra)
        runs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        text[tag] = capsys.readouterr().out
    assert len(runs["plain"]) == 5 and runs["plain"] == runs["compare"]                           # the five pickles, byte for byte
    lat1, lat2 = np.load(str(tmp_path / "lat.npz")), np.load(str(tmp_path / "lat2.npz"))
    assert all(np.array_equal(lat1[k], lat2[k]) for k in lat1.files) and "Cohort comparison" not in text["plain"]
    z, attr = np.load(str(tmp_path / "cmp.npz")), np.load(str(tmp_path / "attr.npz"))
    # the same engine calls by hand
    corpus, _ = open_directory(str(tmp_path / "corpus"), lib_path=emu_lib, first_span=synth.HOTEL_APP["root_op"], fix=None, cache=False)
    units, skipped, n_traces = corpus.units()
    table = corpus.span_table()
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(emu_lib, units, n_traces, rows)
    group, names = traces.groups_from_table(table, corpus)
    eng.set_row_groups(group, len(names))
    of = group == names.index("search")
    ops, inverse = np.unique(table["op_name"][of], return_inverse=True)
    label = np.full(len(group), -1, dtype=np.int32)
    label[of] = inverse
    assert len(ops) >= 2
    eng.set_row_cohorts(label, len(ops))
    eng.stitch()
    eng.attribute(percentile=0.5)
    c = eng.compare_cohorts(((0, 1), (1, 0)), (0.5, 0.9, 1.0), 30, 8)
    for k in traces.CohortComparison.FIELDS:
        assert np.array_equal(z[k], getattr(c, k)), k
    assert z["pairs"].tolist() == [[0, 1], [1, 0]] and z["probs"].tolist() == [0.5, 0.9, 1.0] and z["n_perm"] == 30 and z["n_groups"] == len(names)
    assert z["metrics"].tolist() == list(traces.METRICS) and z["group_names"].tolist() == attr["group_names"].tolist()
    # (every trace of this corpus holds both operations of `search`, so all of them lie in cohort 0: the sizes and the sentinels of an
    # absent side are what the file holds; parts 4 and 5 compare populated cohorts)
    assert c.n_a.sum() > 0 and z["summary"].tolist() == [0, 0, 0, 30]
    eng.close()
    g = int(attr["summary"][4])
    lines = [x for x in text["compare"].splitlines() if x.startswith("Cohort ")]
    assert g >= 0 and len(lines) == 3 and lines[0].startswith("Cohort comparison: 2 pairs, %d segments" % c.summary[0])
    assert lines[1].startswith("Cohort 0 against 1, %s span latency" % names[g]) and lines[2].startswith("Cohort 1 against 0, ")
    base = ["--absolute_path", "x", "--fix", "2", "--results_directory", str(tmp_path) + "/", "--engine_library", emu_lib, "--cache_rate", "0"]
    ok = ["--latency_out", "l.npz", "--cohort_service", "search", "--compare_out", "c.npz"]
    for extra in (ok[2:], ok[:2] + ok[4:], ok[4:], ok + ["--compare_pairs", "0"], ok + ["--compare_pairs", "0,0"], ok + ["--compare_pairs", "a,1"],
                  ok + ["--compare_pairs", "0,1,2"], ok + ["--compare_pairs", "0,-1"], ok + ["--permutations", "-1"], ok + ["--permutations", "65537"],
                  ok + ["--quantiles", ",".join(["0.5"] * 9)]):
        with pytest.raises(SystemExit):
            executor.main(base + extra)
    with pytest.raises(SystemExit):                                # a cohort the service does not have
        executor.main(["--absolute_path", str(tmp_path / "corpus"), "--cache_rate", "0", "--fix", "2", "--results_directory", str(tmp_path / "no") + "/",
                       "--test_name", "gen", "--load_level", "7", "--engine_library", emu_lib, "--latency_out", str(tmp_path / "no.npz"),
                       "--cohort_service", "search", "--compare_out", str(tmp_path / "no_c.npz"), "--compare_pairs", "0,99"])
