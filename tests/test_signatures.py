"""Engine.signatures (tw_trace_signatures, csrc/tw_sig.h): the stitched traces grouped by call-graph signature.  The yardstick is
traces.signatures_host, the definitions of include/traceweaver_amd.h restated with dictionaries of tuples; part 1 checks it on a
forest written out by hand, the rest compares the device with it, np.array_equal on every field of TraceSignatures.FIELDS.
Corpora, cases and helpers are those of tests/test_stitch.py and tests/test_attribute.py.  CPU tier: host-emulation build (an LDS
table of 12 rows: the packed, the single-tree and the rocprim route all occur; one lane per workgroup, and once one host thread
per lane); the HIP library under -m gpu.

The generated corpora have one call graph each, and a service with two callers is never a unit, so with the rows grouped by
service every whole trace has the same signature and the two modes agree.  The shapes therefore come from the groups, which are
the caller's to choose: besides the services, the rows are labelled by their start time alone (start % 2, every eleventh row -1),
which gives a few dozen shapes per corpus and -- the label says nothing about the service -- edges that the levels do not imply."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_attribute as ta
import test_stitch as ts
from traceweaver_amd import synth, traces
from traceweaver_amd.engine import Engine, EngineError

W, U, X = traces.WHOLE, traces.UNASSIGNED, traces.EXACT
FLAG_QUERIES = ((1, 0), (0, 0), (1, 2))


def same(got, want, tag=None):
    for k in traces.TraceSignatures.FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), (k, tag)
        assert getattr(got, k).dtype == getattr(want, k).dtype, (k, tag)


# ---- 1. the restatement on a forest written out by hand -------------------------------------------------------------------
A, B, C, D = 0, 1, 2, 3
S, K = 1, 2          # server / client row
# (kind, group, link); client rows carry group 0, which must not count
HAND = [
    # tree 0: A -> B, C; B -> D
    (S, A, -1), (K, 0, 0), (S, B, 1), (K, 0, 0), (S, C, 3), (K, 0, 2), (S, D, 5),
    # tree 1 (root 7): the same services per level, rows in another order, D under C
    (S, A, -1), (K, 0, 7), (S, C, 8), (K, 0, 9), (S, D, 10), (K, 0, 7), (S, B, 12),
    # tree 2 (root 14): tree 0 with a second C
    (S, A, -1), (K, 0, 14), (S, B, 15), (K, 0, 14), (S, C, 17), (K, 0, 14), (S, C, 19), (K, 0, 16), (S, D, 21),
    # tree 3 (root 23): tree 0 with D one level up
    (S, A, -1), (K, 0, 23), (S, B, 24), (K, 0, 23), (S, C, 26), (K, 0, 23), (S, D, 28),
    # tree 4 (root 30): its only server row has group -1; tree 5 (row 32): an absent row
    (S, -1, -1), (K, 0, 30), (0, 0, -1),
    # tree 6 (root 33): a fragment rooted at a client row
    (K, 0, -1), (S, B, 33),
    # tree 7 (root 35): a row of group -1 between A and D
    (S, A, -1), (K, 0, 35), (S, -1, 36), (K, 0, 37), (S, D, 38),
    # tree 8 (root 40): tree 0 again
    (S, A, -1), (K, 0, 40), (S, B, 41), (K, 0, 40), (S, C, 43), (K, 0, 42), (S, D, 45),
]
HAND_ROOTS = [0, 7, 14, 23, 30, 32, 33, 35, 40]
HAND_LATENCY = [100, 250, 50, 70, 10, 5, 20, 30, 400]
HAND_FLAGS = {0: W, 7: W, 14: W, 23: W, 30: W, 32: 0, 33: 0, 35: W, 40: W}


def hand(mode, need=1, skip=0, reference=None):
    lat = dict(zip(HAND_ROOTS, HAND_LATENCY))
    rows, base = [], 0
    for r, (kind, g, link) in enumerate(HAND):
        if r in lat:
            base = 1000 * r
            rows.append((base, base + lat[r], link))
        else:
            rows.append((base + 1, base + 2, link))
    st, link, start, end = ta.forest(rows, HAND_FLAGS)
    assert st.tree_root.tolist() == HAND_ROOTS and st.tree_latency.tolist() == HAND_LATENCY
    kind, group = [x[0] for x in HAND], [x[1] for x in HAND]
    return traces.signatures_host(st, link, kind, group, 4, mode, need, skip, reference), st, np.array(kind)


def test_host_levels_by_hand():
    s, st, kind = hand("levels")
    assert np.array_equal(s.row_level[kind == 1], st.depth[kind == 1] >> 1) and (s.row_level[kind != 1] == -1).all()
    assert s.row_level[[0, 2, 4, 6, 34, 37, 39]].tolist() == [0, 1, 1, 2, 0, 1, 2]       # row 34: the server child of a client root
    assert s.tree_class.tolist() == [0, 0, 1, 2, 3, -1, -1, 4, 0] and s.tree_items.tolist() == [4, 4, 5, 4, 0, 0, 1, 2, 4]
    assert s.class_rep.tolist() == [0, 2, 3, 4, 7] and s.class_trees.tolist() == [3, 1, 1, 1, 1] and s.n_classes == 5
    assert s.class_off.tolist() == [0, 4, 8, 12, 12, 14]
    assert s.signature(0) == ((0, 0, A, 1), (1, 0, B, 1), (1, 0, C, 1), (2, 0, D, 1))
    assert s.signature(1) == ((0, 0, A, 1), (1, 0, B, 1), (1, 0, C, 2), (2, 0, D, 1))    # one entry's count
    assert s.signature(2) == ((0, 0, A, 1), (1, 0, B, 1), (1, 0, C, 1), (1, 0, D, 1))    # the level of one service
    assert s.signature(3) == () and len(s.entries(3)) == 0                               # group -1 alone: the empty signature
    assert s.signature(4) == ((0, 0, A, 1), (2, 0, D, 1))                                # the row between them counts as a level
    assert s.class_latency_sum.tolist() == [750, 50, 70, 10, 30] and s.class_latency_min.tolist() == [100, 50, 70, 10, 30]
    assert s.class_latency_max.tolist() == [400, 50, 70, 10, 30]
    assert s.summary.tolist() == [7, 5, 23, 14, -1, -1] and (s.tree_same == 255).all()
    t = s.table(["a", "b", "c", "d"])
    assert [r["class"] for r in t] == [0, 1, 2, 3, 4] and t[0]["trees"] == 3 and t[0]["mean_latency"] == 250.0 and t[0]["min_latency"] == 100
    assert t[0]["signature"] == [(0, None, "a", 1), (1, None, "b", 1), (1, None, "c", 1), (2, None, "d", 1)] and t[0]["share"] == 3.0 / 7.0
    with pytest.raises(IndexError):
        s.entries(5)


def test_host_edges_by_hand():
    s, _, _ = hand("edges")
    assert s.tree_class.tolist() == [0, 1, 2, 3, 4, -1, -1, 5, 0] and s.class_rep.tolist() == [0, 1, 2, 3, 4, 7]     # trees 0 and 1 part
    assert s.signature(0) == ((0, -1, A, 1), (1, A, B, 1), (1, A, C, 1), (2, B, D, 1))
    assert s.signature(1) == ((0, -1, A, 1), (1, A, B, 1), (1, A, C, 1), (2, C, D, 1))
    assert s.signature(5) == ((0, -1, A, 1), (2, -1, D, 1))                              # the caller of D has group -1
    assert s.class_trees.tolist() == [2, 1, 1, 1, 1, 1] and s.class_latency_sum[0] == 500 and s.summary.tolist() == [7, 6, 23, 18, -1, -1]


def test_host_eligibility_by_hand():
    s, _, _ = hand("levels", need=0)                              # every tree: the absent row joins the empty signature's class
    assert s.tree_class.tolist() == [0, 0, 1, 2, 3, 3, 4, 5, 0] and s.class_rep.tolist() == [0, 2, 3, 4, 6, 7]
    assert s.signature(4) == ((0, 0, B, 1),) and s.class_trees[3] == 2 and s.class_latency_min[3] == 5 and s.summary[:4].tolist() == [9, 6, 24, 15]
    s, _, _ = hand("edges", need=0)
    assert s.signature(5) == ((0, -1, B, 1),) and s.tree_class[6] == 5                   # a client root is no caller
    ref, _, _ = hand("levels")
    r = ref.by_root()
    assert sorted(r) == [0, 7, 14, 23, 30, 35, 40]
    r[7] = r[14]                                                  # a reference that differs at root 7 and lacks root 40
    del r[40]
    s, _, _ = hand("levels", need=0, reference=r)
    assert s.tree_same.tolist() == [1, 0, 1, 1, 1, 255, 255, 1, 255] and s.summary[4:].tolist() == [6, 5]
    c = traces.compare_signatures(s, ref)
    assert c["tree_same"].tolist() == [1, 1, 1, 1, 1, 255, 255, 1, 1] and c["compared"] == 7 and c["share"] == 1.0


# ---- 2. device = restatement ----------------------------------------------------------------------------------------------
def blind_groups(rows):
    """Labels that say nothing about the service: start % 2, every eleventh row not counted."""
    start = np.asarray(rows[4])
    return np.where(start % 11 == 0, -1, start % 2).astype(np.int32), 2


def check(eng, st, link, rows, group, n_groups, mode, need, skip, tag=None, **kw):
    dev = eng.signatures(mode, need, skip, **kw)
    ref = kw.pop("reference", None)
    want = traces.signatures_host(st, link, rows[3], group, n_groups, mode, need, skip)
    want.tree_same, want.summary = dev.tree_same, np.concatenate([want.summary[:4], dev.summary[4:]])   # (the comparison: part 5)
    same(dev, want, tag)
    assert np.array_equal(dev.tree_root, st.tree_root)
    return dev


def check_forest(eng, st, link, rows, groupings, seen, tag):
    for group, G in groupings:
        eng.set_row_groups(group, G)
        for need, skip in FLAG_QUERIES:
            n = [check(eng, st, link, rows, group, G, mode, need, skip, (tag, G, mode, need, skip)) for mode in (0, 1)]
            assert n[1].n_classes >= n[0].n_classes and np.array_equal(n[0].row_level, n[1].row_level)
            seen["repeated"] = max(seen["repeated"], int((n[0].class_trees >= 2).sum()))
            seen["parted"] = seen["parted"] or n[1].n_classes > n[0].n_classes
    kind = np.asarray(rows[3])
    assert np.array_equal(n[0].row_level[kind == 1], st.depth[kind == 1] >> 1)


def run_case(lib, tmp_path, name, seed, n, concurrency, expect, seen):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    groupings = [traces.groups_from_table(table), blind_groups(rows)]
    groupings[0] = (groupings[0][0], len(groupings[0][1]))
    arrays = [u.arrays for u in units]
    par = [r["parent"] for r in eng.results(2, fields=("parent",))]
    check_forest(eng, eng.stitch(), ta.links_of(arrays, par, rows), rows, groupings, seen, (name, "pass 2"))
    check_forest(eng, eng.stitch(truth=True), ta.links_of(arrays, [u.true_parent for u in units], rows), rows, groupings, seen, (name, "truth"))
    t = eng.signatures_timing()
    assert set(t) == {"items", "sort", "classes"} and all(v >= 0 for v in t.values())
    eng.close()


CASES = ts.CASES[:4]      # (the fifth is the hotel corpus again; its two passes take a minute on the device)
assert [c[0] for c in CASES] == ["hotel", "media", "alibaba", "fanout"]


def run_cases(lib, tmp_path, cases=CASES):
    seen = {"repeated": 0, "parted": False}
    for c in cases:
        run_case(lib, tmp_path, *c, seen=seen)
    return seen


def test_device_equals_host_restatement(emu_lib, tmp_path):
    seen = run_cases(emu_lib, tmp_path)
    assert seen["repeated"] >= 3 and seen["parted"]               # some forest has three classes of two trees and more; one parts in mode 1


@pytest.mark.gpu
def test_device_equals_host_restatement_gpu(tmp_path):
    seen = run_cases(None, tmp_path)
    assert seen["repeated"] >= 3 and seen["parted"]


# ---- 3. sort routes and sizes -----------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 300, 600)      # items of the first trees: either side of a wavefront, of the LDS table of either build (12 / 512)
N_DISTINCT = 300


def sized_table():
    """One service of 8 + 300 requests with one call each, as pass-0 parents; request i's callee rows hang under its call.  Trees
    0..6 hold SIZES items of seven groups in turn (the request row itself is not counted), tree 7 one group 300 times (one entry of
    count 300), the 300 others two items each whose groups no other tree has."""
    n = len(SIZES) + 1 + N_DISTINCT
    u, tp = synth.make_unit(3, n, shape="single")
    callees = [[(j * 5 + i) % 7 for j in range(k)] for i, k in enumerate(SIZES)] + [[7] * 300] + [[8 + i % 20, 28 + i // 20] for i in range(N_DISTINCT)]
    kind = [1] * n + [2] * n
    link = [-1] * (2 * n)
    group = [-1] * len(SIZES) + [7] + [(i % 3) - 1 for i in range(N_DISTINCT)] + [-1] * n
    for i, gs in enumerate(callees):
        for g in gs:
            kind.append(1)
            link.append(n + int(tp[0][i]))
            group.append(g)
    m = len(kind)
    start = 1000 + 3 * np.arange(m, dtype=np.int64)
    start[:n] = np.arange(n)
    rows = ([np.arange(n, dtype=np.int32)], [[np.arange(n, 2 * n, dtype=np.int32)]], np.array(link, dtype=np.int32), np.array(kind, dtype=np.uint8),
            start, start + 1 + (np.arange(m) * 37) % 500)
    return u, tp, rows, np.array(group, dtype=np.int32), 28 + (N_DISTINCT + 19) // 20


def sized_engine(lib):
    u, tp, rows, group, G = sized_table()
    eng = Engine(0, lib_path=lib)
    eng.load([u])
    eng.set_span_rows(*rows)
    eng.set_parents([tp])
    eng.set_row_groups(group, G)
    st = eng.stitch(0)
    return eng, st, ta.links_of([u], [tp], rows), rows, group, G


def run_sizes(lib, modes=(0, 1)):
    eng, st, link, rows, group, G = sized_engine(lib)
    n = len(SIZES) + 1 + N_DISTINCT
    assert st.n_trees == n and st.tree_root.tolist() == list(range(n))
    for mode in modes:
        d = check(eng, st, link, rows, group, G, mode, 1, 0, ("sizes", mode))
        assert d.tree_items[:8].tolist() == list(SIZES) + [301] and d.n_classes == n and d.tree_class.tolist() == list(range(n))
        assert d.signature(7) == ((0, 0 if mode == 0 else -1, 7, 1), (1, 0 if mode == 0 else 7, 7, 300))
        assert np.diff(d.class_off)[:8].tolist() == [0, 1, 7, 7, 7, 7, 7, 2]
    eng.close()


def test_sort_routes_and_sizes(emu_lib):
    run_sizes(emu_lib)


@pytest.mark.gpu
def test_sort_routes_and_sizes_gpu():
    run_sizes(None)


def in_subprocess(call, env):
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "import test_signatures as t\n"
            "%s\n"
            "print('child ok')\n") % (os.path.dirname(here), here, call)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stderr[-2000:]


def test_sizes_lane_threaded(emu_lib):
    """One host thread per lane (TW_EMU_LANES=1, workgroups of 256): the ballots and shuffles of k_sig_sign run as they are written,
    64 lanes to a wavefront, without a GPU."""
    in_subprocess("t.run_sizes(%r, (1,))" % emu_lib, dict(TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256"))


# ---- 4. hash collisions -----------------------------------------------------------------------------------------------------
def test_two_hash_bits(emu_lib, tmp_path, monkeypatch):
    """TW_SIG_HASH_BITS=2: 308 distinct signatures in four buckets; the exact comparison returns the classes of the restatement."""
    monkeypatch.setenv("TW_SIG_HASH_BITS", "2")
    run_sizes(emu_lib)
    run_cases(emu_lib, tmp_path, CASES[1:2])


@pytest.mark.gpu
def test_two_hash_bits_gpu(tmp_path, monkeypatch):
    monkeypatch.setenv("TW_SIG_HASH_BITS", "2")
    run_sizes(None)
    run_cases(None, tmp_path, CASES[1:2])


# ---- 5. comparison with the reference set -----------------------------------------------------------------------------------
def leaf_calls(units, rows):
    """(unit, endpoint, callee rows) of an endpoint whose callees make no call of their own: the server row under each of its calls
    is no request of any unit."""
    row_link, kind = np.asarray(rows[2]), np.asarray(rows[3])
    callee_of = np.full(len(row_link), -1, dtype=np.int64)
    server = np.flatnonzero((kind == 1) & (row_link >= 0))
    callee_of[row_link[server]] = server
    requests = np.concatenate([np.asarray(u.in_rows) for u in units])
    for k, u in enumerate(units):
        for e, out in enumerate(u.out_rows):
            callee = callee_of[np.asarray(out)]
            if (callee >= 0).all() and not np.isin(callee, requests).any():
                return k, e, callee
    raise AssertionError("no endpoint with leaf callees")


def run_compare(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    group, G = blind_groups(rows)
    arrays = [u.arrays for u in units]
    truth = [np.array(u.true_parent, dtype=np.int32) for u in units]
    eng = Engine(0, lib_path=lib)
    eng.load(arrays)
    eng.set_truth(truth, [u.in_trace for u in units], n_traces)
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, G)
    tlink = ta.links_of(arrays, truth, rows)

    def error(code, f, *a, **kw):
        with pytest.raises(EngineError) as ex:
            f(*a, **kw)
        assert ex.value.code == code

    for mode in (0, 1):
        tt = eng.stitch(truth=True)
        error(-4 if mode == 0 else -1, eng.signatures, mode, compare=True)      # no reference set yet / one of the other mode
        true = check(eng, tt, tlink, rows, group, G, mode, 1, 0, keep_reference=True)
        ref = true.by_root()
        assert true.n_classes >= 5

        def compare(par, zeros, tag):
            eng.set_parents(par)
            st = eng.stitch(0)
            link = ta.links_of(arrays, par, rows)
            dev = check(eng, st, link, rows, group, G, mode, 1, 0, tag, compare=True)
            want = traces.signatures_host(st, link, rows[3], group, G, mode, 1, 0, ref)
            same(dev, want, tag)
            c = traces.compare_signatures(dev, true)                                  # (e)
            assert np.array_equal(c["tree_same"], dev.tree_same) and [c["compared"], c["same"]] == dev.summary[4:].tolist()
            whole = (st.tree_flags & W) != 0
            assert (dev.tree_same[whole] != 255).all() and (dev.tree_same[~whole] == 255).all() and whole.sum() == n_traces
            assert sorted(st.tree_root[dev.tree_same == 0].tolist()) == sorted(zeros), tag
            return st, dev

        st, dev = compare(truth, [], "a")                                             # (a) the true parents as pass 0
        assert dev.summary[4:].tolist() == [n_traces, n_traces]
        k, e, callee = leaf_calls(units, rows)
        label, root = group[callee], tt.root[np.asarray(units[k].in_rows)]
        x = truth[k][e]
        i = 0
        j = next(j for j in range(1, len(x)) if label[x[j]] != label[x[i]] and min(label[x[j]], label[x[i]]) >= 0 and root[i] != root[j])
        swapped = [p.copy() for p in truth]
        swapped[k][e][[i, j]] = swapped[k][e][[j, i]]
        compare(swapped, [root[i], root[j]], "b")                                     # (b) a call swapped between two shapes
        j = next(j for j in range(1, len(x)) if label[x[j]] == label[x[i]] and root[i] != root[j])
        swapped = [p.copy() for p in truth]
        swapped[k][e][[i, j]] = swapped[k][e][[j, i]]
        st, dev = compare(swapped, [], "c")                                           # (c) ... between two requests of one shape
        at = np.searchsorted(st.tree_root, [root[i], root[j]])
        assert (st.tree_flags[at] & X == 0).all() and (dev.tree_same[at] == 1).all() and st.counts[3] == n_traces - 2
    # (d) the set survived the stitches above; new row groups and new row maps drop it
    eng.set_row_groups(group, G)
    error(-4, eng.signatures, 1, compare=True)
    eng.signatures(1, keep_reference=True)
    eng.signatures(1, compare=True)
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, G)
    eng.stitch(0)
    error(-4, eng.signatures, 1, compare=True)
    eng.close()


def test_comparison(emu_lib, tmp_path):
    run_compare(emu_lib, tmp_path)


@pytest.mark.gpu
def test_comparison_gpu(tmp_path):
    run_compare(None, tmp_path)


# ---- 6. state and argument errors -------------------------------------------------------------------------------------------
def deep_chain(levels):
    """One service whose request i + 1 is the callee of request i's call: a single trace `levels` server rows deep."""
    u, tp = synth.make_unit(3, levels, shape="single")
    link = np.full(2 * levels, -1, dtype=np.int32)
    link[1:levels] = levels + np.asarray(tp[0][:-1])
    kind = np.array([1] * levels + [2] * levels, dtype=np.uint8)
    start = np.arange(2 * levels, dtype=np.int64)
    return u, tp, ([np.arange(levels, dtype=np.int32)], [[np.arange(levels, 2 * levels, dtype=np.int32)]], link, kind, start, start + 1)


def run_errors(lib):
    eng, st, link, rows, group, G = sized_engine(lib)

    def error(code, f, *a, **kw):
        with pytest.raises(EngineError) as ex:
            f(*a, **kw)
        assert ex.value.code == code and {-4: "TW_ERR_STATE", -1: "TW_ERR_ARG", -2: "TW_ERR_UNSUPPORTED"}[code] in str(ex.value)

    error(-1, eng.signatures, 2)
    error(-1, eng.signatures, -1)
    error(-4, eng.signatures, compare=True)
    # the two-call sizing by hand: sizes first, then the copy without new kernel time
    import ctypes
    from traceweaver_amd import _ffi
    q = _ffi.SigQuery(0, 1, 0, 0, 0)
    summary = np.zeros(6, dtype=np.int64)
    assert eng._lib.tw_trace_signatures(eng._h, ctypes.byref(q), None, summary.ctypes.data_as(ctypes.c_void_p)) == 0
    want = traces.signatures_host(st, link, rows[3], group, G, 0, 1, 0)
    assert summary.tolist() == want.summary.tolist() and summary[3] > 0
    t0 = eng.signatures_timing()
    entries = np.zeros((int(summary[3]), 4), dtype=np.int32)
    out = _ffi.Signatures(*([None] * 10 + [entries.ctypes.data_as(ctypes.c_void_p)]))
    assert eng._lib.tw_trace_signatures(eng._h, ctypes.byref(q), ctypes.byref(out), None) == 0
    assert np.array_equal(entries, want.class_entries) and eng.signatures_timing() == t0
    eng.set_row_groups(group, (1 << 20) + 1)
    error(-2, eng.signatures)                                     # more groups than the key holds
    eng.set_row_groups(group, 1 << 20)
    check(eng, st, link, rows, group, 1 << 20, 1, 1, 0)
    eng.run_pass1()                                               # a new pass drops the forest
    error(-4, eng.signatures)
    eng.stitch(0)
    eng.signatures()
    eng.set_span_rows(*rows)                                      # new row maps drop the forest and the groups
    error(-4, eng.signatures)
    eng.stitch(0)
    error(-4, eng.signatures)                                     # ... a forest, but no groups
    eng.set_row_groups(group, G)
    check(eng, st, link, rows, group, G, 0, 1, 0)
    eng.load([sized_table()[0]])                                  # a load drops everything
    error(-4, eng.signatures)
    eng.close()
    fresh = Engine(0, lib_path=lib)
    error(-4, fresh.signatures)                                   # before anything
    fresh.close()


def test_state_and_argument_errors(emu_lib):
    run_errors(emu_lib)


@pytest.mark.gpu
def test_state_and_argument_errors_gpu():
    run_errors(None)   # (all refused on the host: nothing malformed reaches the device)


def run_deep(lib, limit):
    """A server row at level `limit` does not fit the key: refused; one level less is served."""
    for levels in (limit + 1, limit):
        u, tp, rows = deep_chain(levels)
        eng = Engine(0, lib_path=lib)
        eng.load([u])
        eng.set_span_rows(*rows)
        eng.set_parents([tp])
        group = np.zeros(2 * levels, dtype=np.int32)
        eng.set_row_groups(group, 1)
        st = eng.stitch(0)
        assert st.n_trees == 1 and st.depth.max() == 2 * levels - 1
        if levels <= limit:
            s = check(eng, st, ta.links_of([u], [tp], rows), rows, group, 1, 1, 1, 0)
            assert s.row_level.max() == levels - 1 and s.n_classes == 1 and len(s.entries(0)) == levels
            assert s.entries(0)[-1].tolist() == [levels - 1, 0, 0, 1] and s.entries(0)[0].tolist() == [0, -1, 0, 1]
        else:
            with pytest.raises(EngineError) as ex:
                eng.signatures()
            assert ex.value.code == -2 and "TW_ERR_UNSUPPORTED" in str(ex.value)
        eng.close()


def test_level_beyond_the_key(emu_lib):
    """The host build keeps 6 bits of level (the HIP build 16: a chain that deep costs the stitch's quadratic rank sort of one
    131072-row tree, seconds on either machine), so that the refusal is reached with 65 levels."""
    run_deep(emu_lib, 64)


@pytest.mark.gpu
def test_deep_chain_gpu():
    """65 levels are nothing special for the HIP build's 16 bits: served, and equal to the restatement."""
    u, tp, rows = deep_chain(65)
    eng = Engine(0)
    eng.load([u])
    eng.set_span_rows(*rows)
    eng.set_parents([tp])
    group = np.zeros(130, dtype=np.int32)
    eng.set_row_groups(group, 1)
    s = check(eng, eng.stitch(0), ta.links_of([u], [tp], rows), rows, group, 1, 1, 1, 0)
    assert s.row_level.max() == 64 and len(s.entries(0)) == 65
    eng.close()


# ---- 7. the command line ----------------------------------------------------------------------------------------------------
def test_cli_signatures_out(emu_lib, reference_root, tmp_path, capsys):
    """--signatures_out on the shipped hotel corpus: both sides in the file, the predicted side equal to the same engine calls by
    hand; the shape accuracy lies in [0, 1] and is recorded, and no lower than the exact share: a trace with the true rows under
    the true root has the true call graph whenever its links are the true ones, which the host checks first."""
    from traceweaver_amd import executor
    from traceweaver_amd.ingest import REFERENCE_FIX, open_directory

    rel = "data/hotel_reservation/hotel_load100/"
    base = ["--relative_path", rel, "--compressed", "0", "--cache_rate", "0", "--fix", "2", "--test_name", "hotel_test", "--load_level", "100",
            "--compress_factor", "1", "--repeat_factor", "1", "--execute_parallel", "0", "--clear_cache", "1", "--predictor_indices", "10",
            "--project_root", reference_root, "--engine_library", emu_lib, "--fit", "device"]
    runs = {}
    for tag, extra in (("plain", []), ("levels", ["--signatures_out", str(tmp_path / "levels.npz")]),
                       ("edges", ["--signatures_out", str(tmp_path / "edges.npz"), "--signature_mode", "edges", "-v"])):
        out = str(tmp_path / tag) + "/"
        executor.main(base + ["--results_directory", out] + extra)
        runs[tag] = ({f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}, capsys.readouterr().out)
    assert runs["plain"][0] == runs["levels"][0] == runs["edges"][0] and len(runs["plain"][0]) == 5      # the pickles, byte for byte
    assert "Call graphs" not in runs["plain"][1] and "Call graphs (levels):" in runs["levels"][1] and "Shape accuracy:" in runs["edges"][1]
    first_span, fix = REFERENCE_FIX[2]
    corpus, _ = open_directory(os.path.join(reference_root, rel), lib_path=emu_lib, first_span=first_span, fix=fix, cache=False)
    units, skipped, n_traces = corpus.units()
    table = corpus.span_table()
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table, corpus)
    for mode in traces.SIGNATURE_MODES:
        z = np.load(str(tmp_path / (mode + ".npz")))
        assert str(z["mode"]) == mode and z["group_names"].tolist() == [str(x) for x in names]
        # the true side against the restatement; the predicted side's comparison against compare_signatures
        arrays, truth = [u.arrays for u in units], [u.true_parent for u in units]
        eng = Engine(0, lib_path=emu_lib)
        eng.load(arrays)
        eng.set_truth(truth, [u.in_trace for u in units], n_traces)
        eng.set_span_rows(*rows)
        tt = eng.stitch(truth=True)
        eng.close()
        want = traces.signatures_host(tt, ta.links_of(arrays, truth, rows), rows[3], group, len(names), mode)
        for k in traces.TraceSignatures.FIELDS:
            assert np.array_equal(z["true_" + k], getattr(want, k)), k
        assert want.n_eligible == n_traces and np.array_equal(z["true_tree_root"], tt.tree_root)
        pred = traces.TraceSignatures(*[z[k] for k in traces.TraceSignatures.FIELDS], mode=traces.SIGNATURE_MODES.index(mode), tree_root=z["tree_root"])
        c = traces.compare_signatures(pred, want)
        assert np.array_equal(c["tree_same"], pred.tree_same) and c["compared"] == pred.summary[4] == n_traces
        acc = float(z["shape_accuracy"])
        assert 0.0 <= acc <= 1.0 and acc == c["share"]
        print("hotel_load100, %s: %d call graphs among the predicted traces, %d among the true ones; shape accuracy %.4f" % (mode, pred.n_classes, want.n_classes, acc))
    bad = ["--results_directory", str(tmp_path) + "/", "--signatures_out", "s.npz"]
    for extra in (["--cache_rate", "0.1"], ["--predictor_indices", "3"], ["--signature_mode", "paths"]):
        with pytest.raises(SystemExit):
            executor.main([x for x in base if x not in extra[:1]] + bad + extra)
