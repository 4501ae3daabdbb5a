"""Engine.extract_traces (tw_extract_traces / tw_get_extracted, csrc/tw_extr.h): trees of the stitched forest handed out as a packed
sub-forest -- every selected tree in pre-order with local parent indices.  The yardstick is traces.extract_host, the definitions of
include/traceweaver_amd.h restated with sorted() and a recursion over children(); part 1 checks it on the forest written out by hand in
tests/test_signatures.py, the rest compares the device with it, np.array_equal and equal dtype on every field of
ExtractedTraces.FIELDS, and applies properties that do not lean on the restatement to every device result.  Corpora, cases and helpers
are those of tests/test_stitch.py, test_attribute.py, test_signatures.py, test_profiles.py and test_filter.py.  CPU tier: host-emulation
build (four trees to a wavefront, a tree of more than 12 rows alone: both routes occur; one lane per workgroup, and once one host thread
per lane); the HIP library under -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_attribute as ta
import test_filter as tf
import test_profiles as tp
import test_signatures as tg
import test_stitch as ts
from traceweaver_amd import synth, traces
from traceweaver_amd.engine import Engine, EngineError
from traceweaver_amd.traces import clause

W, M, CONF = traces.WHOLE, traces.MATCH, traces.CONFIDENT
X = traces.ExtractedTraces


def cap_of(lib):
    """kExtrCap / kExtrTrees of the build: the emulation build has the tiny values."""
    return (12, 4) if lib else (256, 16)


def same(got, want, tag=None):
    for k in X.FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), (k, tag)
        assert getattr(got, k).dtype == getattr(want, k).dtype == X.DTYPES.get(k, np.int64), (k, tag)


def with_flags(st, flags):
    return traces.StitchedTraces(st.root, st.depth, st.tree_off, st.tree_rows, st.tree_root, st.tree_latency, np.asarray(flags, dtype=np.uint8), st.counts)


# ---- 2. properties that do not lean on the restatement ----------------------------------------------------------------------------
def check_properties(x, st, link, start, end, tag=None):
    link, start = np.asarray(link), np.asarray(start)
    assert len(x.out_off) == x.n_trees + 1 and x.out_off[0] == 0 and x.out_off[-1] == len(x.row) == x.summary[2], tag
    for j in range(x.n_trees):
        t = x.trace(j)
        n = len(t["row"])
        k = t["tree"]
        assert n == t["subtree"][0] and t["parent"][0] == -1 and t["row"][0] == t["root"] == st.tree_root[k] and t["latency"] == st.tree_latency[k], (tag, j)
        assert t["start_time"] == start[t["root"]], (tag, j)
        idx = np.arange(n)
        assert (t["parent"][1:] < idx[1:]).all() and (t["parent"][1:] >= 0).all(), (tag, j)
        assert np.array_equal(t["row"][t["parent"][1:]], link[t["row"][1:]]) and link[t["row"][0]] == -1, (tag, j)
        assert np.array_equal(np.sort(t["row"]), np.sort(st.tree_rows[int(st.tree_off[k]):int(st.tree_off[k + 1])])), (tag, j)
        assert np.array_equal(t["depth"][1:], t["depth"][t["parent"][1:]] + 1) and t["depth"][0] == 0, (tag, j)
        below = np.ones(n, dtype=np.int64)
        for i in range(n - 1, 0, -1):                              # (a parent stands before its children: one sweep from the end)
            below[t["parent"][i]] += below[i]
        assert np.array_equal(below, t["subtree"]), (tag, j)
        kids = [[] for _ in range(n)]
        for i in range(1, n):
            kids[t["parent"][i]].append(i)
        for i in range(n):
            keys = [(int(t["start"][c]), int(t["row"][c])) for c in kids[i]]
            assert keys == sorted(keys) and kids[i] == x.children(j, i), (tag, j, i)
        if x.has_times:
            r = t["root"]
            assert t["path_time"].sum() == max(int(end[r]), int(start[r])) - int(start[r]), (tag, j)


# ---- 1. the restatement on the forest written out by hand -------------------------------------------------------------------------
def hand_forest():
    """The HAND forest of tests/test_signatures.py, rows and latencies as hand() of tests/test_filter.py builds them."""
    lat = dict(zip(tg.HAND_ROOTS, tg.HAND_LATENCY))
    rows, base = [], 0
    for r, (kind, g, link) in enumerate(tg.HAND):
        if r in lat:
            base = 1000 * r
            rows.append((base, base + lat[r], link))
        else:
            rows.append((base + 1, base + 2, link))
    st, link, start, end = ta.forest(rows, tg.HAND_FLAGS)
    return st, link, start, end, [x[0] for x in tg.HAND], [x[1] for x in tg.HAND]


def test_host_by_hand():
    st, link, start, end, kind, group = hand_forest()
    host = lambda **q: traces.extract_host(st, link, kind, start, end, group, **q)
    # trees 0 .. 8: latencies 100, 250, 50, 70, 10, 5, 20, 30, 400; trees 5 and 6 are no whole traces.  Every non-root row of a tree
    # starts at the same time, so siblings stand in row order.  Tree 0 (rows 0 .. 6): the second call of the root, row 3, comes
    # after the whole subtree of the first, rows 1, 2, 5, 6 -- the pre-order is not the row order
    x = host(mode="list", trees=[0, 1, 2])
    assert x.out_off.tolist() == [0, 7, 14, 23] and x.summary.tolist() == [9, 3, 23, 9, 0, 0]
    assert x.trace(0)["row"].tolist() == [0, 1, 2, 5, 6, 3, 4]
    assert x.trace(0)["parent"].tolist() == [-1, 0, 1, 2, 3, 0, 5] and x.trace(0)["subtree"].tolist() == [7, 4, 3, 2, 1, 2, 1]
    assert x.trace(0)["depth"].tolist() == [0, 1, 2, 3, 4, 1, 2]
    # tree 1 (root 7): A -> C -> D under the first call, B under the second
    assert x.trace(1)["row"].tolist() == [7, 8, 9, 10, 11, 12, 13]
    assert x.trace(1)["parent"].tolist() == [-1, 0, 1, 2, 3, 0, 5] and x.trace(1)["subtree"].tolist() == [7, 4, 3, 2, 1, 2, 1]
    # tree 2 (root 14): three calls under the root; D (rows 21, 22) hangs under B (row 16) and so comes before the second call
    assert x.trace(2)["row"].tolist() == [14, 15, 16, 21, 22, 17, 18, 19, 20]
    assert x.trace(2)["parent"].tolist() == [-1, 0, 1, 2, 3, 0, 5, 0, 7] and x.trace(2)["subtree"].tolist() == [9, 4, 3, 2, 1, 2, 1, 2, 1]
    assert x.children(2, 0) == [1, 5, 7] and x.children(2, 2) == [3] and x.children(2, 8) == []
    assert x.trace(2)["kind"].tolist() == [1, 2, 1, 2, 1, 2, 1, 2, 1] and x.trace(2)["group"].tolist() == [0, 0, 1, 0, 3, 0, 2, 0, 2]
    assert x.trace(2)["start"].tolist() == [14000] + [14001] * 8 and x.trace(2)["end"].tolist() == [14050] + [14002] * 8
    assert x.sel_latency.tolist() == [100, 250, 50] and x.sel_start.tolist() == [0, 7000, 14000] and x.sel_flags.tolist() == [1, 1, 1]
    assert len(x.self_time) == len(x.path_time) == 0 and not x.has_times
    check_properties(x, st, link, start, end, "hand")
    # the selections
    x = host(mode="top", order="slowest", limit=3)
    assert x.sel_tree.tolist() == [8, 1, 0] and x.summary.tolist() == [7, 3, 21, 7, 0, 0] and x.sel_root.tolist() == [40, 7, 0]
    assert host(mode="top", order="fastest").sel_tree.tolist() == [4, 7, 2, 3, 0, 1, 8]
    assert host(mode="top", order="fastest", need_flags=0).sel_tree.tolist() == [5, 4, 6, 7, 2, 3, 0, 1, 8]
    assert host(mode="top", order="tree", limit=2, need_flags=0, skip_flags=W).sel_tree.tolist() == [5, 6]
    x = host(mode="quantiles", probs=(0.0, 0.5, 1.0))              # of seven: indices 0, 3, 6
    assert x.sel_tree.tolist() == [4, 3, 8] and x.summary[:2].tolist() == [7, 3]
    assert host(mode="quantiles", probs=(0.5, 0.5)).sel_tree.tolist() == [3, 3]
    assert host(mode="quantiles", probs=(0.5,), need_flags=W | M).n_trees == 0          # no tree carries the bit: n = 0 selects nothing
    x = host(mode="list", trees=[6, 6, 5])                         # a fragment twice and the absent row: the flags are not applied
    assert x.sel_tree.tolist() == [6, 6, 5] and x.out_off.tolist() == [0, 2, 4, 5] and x.row.tolist() == [33, 34, 33, 34, 32]
    assert x.parent.tolist() == [-1, 0, -1, 0, -1] and x.kind.tolist() == [2, 1, 2, 1, 0] and x.sel_flags.tolist() == [0, 0, 0] and x.summary[0] == 9
    # the match bit of a filter, as the device holds it
    f = traces.filter_host(st, link, kind, start, end, group, 4, [clause("latency", 100, None)])
    marked = tf.with_match(st, f)
    x = traces.extract_host(marked, link, kind, start, end, group, mode="top", order="tree", need_flags=W | M)
    assert x.sel_tree.tolist() == [0, 1, 8] and x.sel_flags.tolist() == [W | M] * 3 and x.summary[0] == 3
    # times of an attribution; the single-tree route counts by the build's table
    attr = traces.attribute_host(st, link, start, end, np.array(group, dtype=np.int32), 4)
    x = traces.extract_host(st, link, kind, start, end, None, mode="list", trees=[2], attribution=attr, single_rows=8)
    assert x.summary.tolist() == [9, 1, 9, 9, 1, 1] and x.group.tolist() == [-1] * 9 and x.path_time.sum() == 50
    assert np.array_equal(x.self_time, attr.self_time[x.row])
    check_properties(x, st, link, start, end, "hand, times")
    text = x.render(0, ["a", "b", "c", "d"]).splitlines()
    assert text[0].startswith("trace 0: tree 2, root row 14, 9 rows, latency 50 us") and len(text) == 10 and text[2].lstrip().startswith("* ")
    for bad in (dict(mode=3), dict(mode="top", order=3), dict(mode="top", limit=-1), dict(mode="quantiles", probs=(1.5,)), dict(mode="quantiles", probs=(-0.1,)),
                dict(mode="quantiles", probs=(float("nan"),)), dict(mode="quantiles", probs=[0.5] * 33), dict(mode="list", trees=[9]), dict(mode="list", trees=[-1]),
                dict(mode="nosuch")):
        with pytest.raises(ValueError):
            host(**bad)


# ---- 3. device = restatement on solved corpora --------------------------------------------------------------------------------------
PROBS = (0.0, 0.5, 0.95, 0.99, 1.0)


def queries(match_trees):
    out = [dict(mode="top", order=o, limit=k) for o in traces.EXTRACT_ORDERS for k in (0, 1, 7)]
    return out + [dict(mode="quantiles", probs=PROBS), dict(mode="list", trees=list(match_trees)[::-1])]


def check_queries(eng, lib, st, link, rows, group, attr_host, qs, flag_queries, tag, seen=None):
    kind, start, end = rows[3], np.asarray(rows[4]), np.asarray(rows[5])
    for need, skip in flag_queries:
        for q in qs:
            dev = eng.extract_traces(need_flags=need, skip_flags=skip, **q)
            want = traces.extract_host(st, link, kind, start, end, group, need_flags=need, skip_flags=skip, attribution=attr_host, single_rows=cap_of(lib)[0], **q)
            same(dev, want, (tag, need, skip, q))
            check_properties(dev, st, link, start, end, (tag, need, skip, q))
            if seen is not None:
                seen.append(dev)


def check_forest(eng, lib, st, link, rows, group, G, tag, score=False):
    """Every mode on the forest last stitched: without row groups and attribution, with both, and with the MATCH bit of a filter (and,
    on a forest of a pass, the CONFIDENT bit of score_traces) named."""
    kind, start, end = rows[3], np.asarray(rows[4]), np.asarray(rows[5])
    eng.set_row_groups(group, G)
    mid = int(np.median(st.tree_latency[(st.tree_flags & W) != 0]))
    f = eng.filter_traces([clause("latency", mid, None)])
    assert 0 < f.n_matched < f.n_eligible, tag
    flags = st.tree_flags | (M * f.tree_match)
    if score:
        conf = eng.score_traces(0.0)
        flags = flags | (CONF * (conf.tree_confident != 0)).astype(np.uint8)
    marked = with_flags(st, flags)
    seen = []
    check_queries(eng, lib, marked, link, rows, group, None, queries(f.match_trees), ((W, 0), (0, 0)), (tag, "no times"), seen)
    assert all(not x.has_times for x in seen) and len({x.n_trees for x in seen}) > 3
    eng.attribute()
    attr_host = traces.attribute_host(st, link, start, end, group, G)
    flag_queries = ((W, 0), (W | M, 0), (W, M)) + (((W | CONF, 0), (W | M | CONF, 0)) if score else ())
    seen = []
    check_queries(eng, lib, marked, link, rows, group, attr_host, queries(f.match_trees), flag_queries, (tag, "times"), seen)
    assert all(x.has_times for x in seen)
    by = {(x.n_eligible, x.n_trees) for x in seen}
    assert (f.n_matched, f.n_matched) in by and (f.n_eligible - f.n_matched, 7) in by, (tag, by)
    t = eng.extract_timing()
    assert list(t) == ["select", "trees", "copies"] and all(v >= 0 for v in t.values())


def run_case(lib, tmp_path, name, seed, n, concurrency, expect):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    arrays = [u.arrays for u in units]
    par = [r["parent"] for r in eng.results(2, fields=("parent",))]
    group, names = traces.groups_from_table(table)
    check_forest(eng, lib, eng.stitch(), ta.links_of(arrays, par, rows), rows, group, len(names), (name, "pass 2"), score=True)
    check_forest(eng, lib, eng.stitch(truth=True), ta.links_of(arrays, [u.true_parent for u in units], rows), rows, group, len(names), (name, "truth"))
    eng.close()


@pytest.mark.parametrize("name,seed,n,concurrency,expect", ts.CASES[:4], ids=[c[0] for c in ts.CASES[:4]])
def test_device_equals_host_restatement(emu_lib, tmp_path, name, seed, n, concurrency, expect):
    run_case(emu_lib, tmp_path, name, seed, n, concurrency, expect)


GPU_CASE = ts.CASES[1]
assert GPU_CASE[0] == "media"


@pytest.mark.gpu
def test_device_equals_host_restatement_gpu(tmp_path):
    run_case(None, tmp_path, *GPU_CASE)


# ---- 4. shapes at which the kernel can go wrong ------------------------------------------------------------------------------------
def shape_rows(request):
    return 2 + sum(1 if c[0] == "leaf" else shape_rows(c[2]) for c in request)


def shape_table(specs):
    """One service with one call per request, as pass-0 parents (as sized_table and deep_chain of tests/test_signatures.py).  A server row
    hangs under a client row only, so a tree is made of requests: specs[i] is the root request of tree i, a request the list of what
    hangs under its call -- ("leaf", start) a callee row, ("req", start, request) another request of the service.  Requests are
    numbered tree by tree, so the trees stand in the order of the specs; starts count from the tree's base."""
    count = lambda request: 1 + sum(count(c[2]) for c in request if c[0] == "req")
    n = sum(count(s) for s in specs)
    u, tp_ = synth.make_unit(3, n, shape="single")
    call = lambda i: n + int(tp_[0][i])
    kind, link, start = [1] * n + [2] * n, [-1] * (2 * n), [0] * (2 * n)
    free = [0]

    def place(request, under, s, base):
        i = free[0]
        free[0] += 1
        link[i], start[i], start[call(i)] = under, s, s + 1
        for c in request:
            if c[0] == "leaf":
                kind.append(1)
                link.append(call(i))
                start.append(base + c[1])
            else:
                place(c[2], call(i), base + c[1], base)

    for t, spec in enumerate(specs):
        place(spec, -1, 100000 * (t + 1), 100000 * (t + 1) + 2)
    m = len(kind)
    start = np.array(start, dtype=np.int64)
    rows = ([np.arange(n, dtype=np.int32)], [[np.arange(n, 2 * n, dtype=np.int32)]], np.array(link, dtype=np.int32), np.array(kind, dtype=np.uint8),
            start, start + 1 + (np.arange(m) * 37) % 500)
    return u, tp_, rows, (np.arange(m) % 5).astype(np.int32) - 1, 4


def star(k, start=lambda j: 3 * j):
    return [("leaf", start(j)) for j in range(k)]


def chain(requests):
    """`requests` requests, each the only callee of the one above: 2 * requests rows, each the parent of the next."""
    out = []
    for _ in range(requests - 1):
        out = [("req", 5, out)]
    return out


STAR_SIZES = (0, 1, 63, 64, 65, 300, 600)
SMALL = [star(0), star(1), star(2)]
# under the root's call, by start: a chain of 6 rows, a leaf, chains of 4 and 2 rows -- 15 rows; and the same shape within 9 rows
STAR_OF_CHAINS = [("req", 50, chain(1)), ("leaf", 20), ("req", 30, chain(2)), ("req", 10, chain(3))]
STAR_OF_CHAINS_SMALL = [("req", 5, chain(1)), ("leaf", 3), ("req", 1, chain(2))]
# the stars either side of a wavefront and of kExtrCap in either build (12 / 256); a large tree between small ones, so that a wavefront's
# group of trees straddles it; chains deeper than the lanes and than the table; stars of chains (subtree sizes differ among siblings);
# stars whose order is decided by the row (one start time) and by the start against the row (the starts descend)
SHAPES = ([("star %d" % k, star(k)) for k in STAR_SIZES] + [("small", x) for x in SMALL] + [("between", star(300))] + [("small", x) for x in SMALL] +
          [("chain 70", chain(35)), ("chain 300", chain(150)), ("star of chains", STAR_OF_CHAINS), ("small star of chains", STAR_OF_CHAINS_SMALL),
           ("one start", star(40, lambda j: 7)), ("descending", star(40, lambda j: 1000 - j))] + [("small", x) for x in SMALL])
AT = {name: i for i, (name, _) in enumerate(SHAPES) if name != "small"}


def run_shapes(lib):
    specs = [x for _, x in SHAPES]
    eng, st, link, rows, group, G = tp.table_engine(lib, shape_table(specs))
    cap, per = cap_of(lib)
    kind, start, end = rows[3], np.asarray(rows[4]), np.asarray(rows[5])
    sizes = np.diff(st.tree_off)
    assert st.n_trees == len(specs) and sizes.tolist() == [shape_rows(x) for x in specs]
    b = AT["between"]
    assert sizes[b] == 302 and sizes[b - 1] == sizes[b + 3] == 4 and sizes[AT["chain 70"]] == 70 and sizes[AT["chain 300"]] == 300
    assert sizes[AT["star of chains"]] == 15 and sizes[AT["small star of chains"]] == 9
    big = int((sizes > cap).sum())
    listed = [b, b - 1, b, AT["star 63"], AT["star of chains"], AT["chain 300"], 0, AT["chain 70"]]
    attr_host = None
    for times in (False, True):
        if times:
            eng.attribute()
            attr_host = traces.attribute_host(st, link, start, end, group, G)
        seen = []
        qs = [dict(mode="top", order="tree"), dict(mode="top", order="slowest"), dict(mode="top", order="fastest", limit=per),
              dict(mode="top", order="tree", limit=per + 1), dict(mode="top", order="tree", limit=1), dict(mode="top", order="tree", need_flags=W | M),
              dict(mode="quantiles", probs=(0.0, 1.0, 0.5)), dict(mode="list", trees=listed)]
        for q in qs:
            q = dict(q)
            need = q.pop("need_flags", W)
            check_queries(eng, lib, st, link, rows, group, attr_host, [q], ((need, 0),), ("shapes", times), seen)
        assert [x.n_trees for x in seen] == [len(specs), len(specs), per, per + 1, 1, 0, 3, 8]
        # both routes: the trees beyond the table alone, the others in groups
        assert seen[0].summary.tolist() == [len(specs), len(specs), int(sizes.sum()), 602, big, int(times)] and 0 < big < len(specs)
        assert seen[7].summary[4] == int((sizes[listed] > cap).sum()) >= 3 and seen[5].summary.tolist() == [0, 0, 0, 0, 0, int(times)]
        assert seen[4].summary[4] == 0                              # (the first tree has two rows)
        # the chain: each row the parent of the next; the stars of chains: the subtrees under the call in the order of their starts
        c = seen[0].trace(AT["chain 300"])
        assert c["parent"].tolist() == list(range(-1, 299)) and c["subtree"].tolist() == list(range(300, 0, -1)) and c["depth"].tolist() == list(range(300))
        for name, want in (("star of chains", [6, 1, 4, 2]), ("small star of chains", [4, 1, 2])):
            s = seen[0].trace(AT[name])
            assert s["subtree"].tolist()[:2] == [2 + sum(want), 1 + sum(want)] and [int(s["subtree"][i]) for i in seen[0].children(AT[name], 1)] == want
        # one start time: by row; descending starts: against the rows
        a, d = seen[0].trace(AT["one start"]), seen[0].trace(AT["descending"])
        assert (np.diff(a["row"][2:]) > 0).all() and (np.diff(a["start"][2:]) == 0).all()
        assert (np.diff(d["row"][2:]) < 0).all() and (np.diff(d["start"][2:]) > 0).all()
    eng.close()


def test_shapes(emu_lib):
    run_shapes(emu_lib)


@pytest.mark.gpu
def test_shapes_gpu():
    run_shapes(None)


def test_shapes_lane_threaded(emu_lib):
    """One host thread per lane (TW_EMU_LANES=1, workgroups of 256): the LDS adds, ballots and shuffles of k_extr_trees and
    k_extr_sizes run as they are written, 64 lanes to a wavefront and four wavefronts to a workgroup, without a GPU."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "import test_extract as t\n"
            "t.run_shapes(%r)\n"
            "print('child ok')\n") % (os.path.dirname(here), here, emu_lib)
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stderr[-2000:]


# ---- 5. state and arguments ---------------------------------------------------------------------------------------------------------
def refused(code, call, *args, **kw):
    with pytest.raises(EngineError) as ex:
        call(*args, **kw)
    assert ex.value.code == code and {-1: "TW_ERR_ARG", -4: "TW_ERR_STATE"}[code] in str(ex.value), str(ex.value)


def read_again(eng, x):
    """tw_get_extracted once more, with buffers of the sizes the result has."""
    import ctypes
    from traceweaver_amd import _ffi

    cols = {k: np.zeros(len(getattr(x, k)), dtype=getattr(x, k).dtype) for k in X.FIELDS[:-1]}
    out = _ffi.Extracted(*[cols[k].ctypes.data_as(ctypes.c_void_p) if len(cols[k]) else None for k in X.FIELDS[:-1]])
    rc = eng._lib.tw_get_extracted(eng._h, ctypes.byref(out))
    return rc, X(x.summary, **cols)


def run_state(lib, tmp_path):
    import ctypes
    from traceweaver_amd import _ffi

    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 120, 1.2)
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table)
    eng = Engine(0, lib_path=lib)
    eng.load([u.arrays for u in units])
    refused(-4, eng.extract_traces)                               # before the row maps, before a stitch
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    eng.set_span_rows(*rows)
    refused(-4, eng.extract_traces)
    none = _ffi.Extracted()
    assert eng._lib.tw_get_extracted(eng._h, ctypes.byref(none)) == -4           # no result yet
    st = eng.stitch(truth=True)
    link = ta.links_of([u.arrays for u in units], [u.true_parent for u in units], rows)
    kind, start, end = rows[3], np.asarray(rows[4]), np.asarray(rows[5])
    x = eng.extract_traces("top", "slowest", 5)                   # neither row groups nor an attribution are resident
    same(x, traces.extract_host(st, link, kind, start, end, None, "top", "slowest", 5, single_rows=cap_of(lib)[0]), "no groups")
    assert (x.group == -1).all() and not x.has_times and x.n_trees == 5
    rc, y = read_again(eng, x)
    assert rc == 0
    same(y, x, "twice")
    # the times of a result that holds none
    buf = np.zeros(len(x.row), dtype=np.int64)
    for k in ("self_time", "path_time"):
        out = _ffi.Extracted(**{k: buf.ctypes.data_as(ctypes.c_void_p)})
        assert eng._lib.tw_get_extracted(eng._h, ctypes.byref(out)) == -4 and b"times" in eng._lib.tw_last_error(eng._h)
    # every argument error leaves the result readable
    for bad in (dict(mode=3), dict(mode=-1), dict(mode="top", order=3), dict(mode="top", order=-1), dict(mode="top", limit=-1), dict(mode="quantiles", probs=(1.5,)),
                dict(mode="quantiles", probs=(-0.5,)), dict(mode="quantiles", probs=(float("nan"),)), dict(mode="quantiles", probs=[0.5] * 33),
                dict(mode="list", trees=[st.n_trees]), dict(mode="list", trees=[0, -1])):
        refused(-1, eng.extract_traces, **bad)
    q = _ffi.ExtractQuery(1, 0, 2, 0, 0, 0, (1 << 20) + 1, None, (ctypes.c_int32 * 1)(0))
    assert eng._lib.tw_extract_traces(eng._h, ctypes.byref(q), None) == -1
    q = _ffi.ExtractQuery(1, 0, 1, 0, 0, -1, 0, None, None)
    assert eng._lib.tw_extract_traces(eng._h, ctypes.byref(q), None) == -1
    rc, y = read_again(eng, x)
    assert rc == 0
    same(y, x, "after the refusals")
    # the result answers the query as the flags stood: a filter, new row groups and an attribution leave it
    eng.set_row_groups(group, len(names))
    f = eng.filter_traces([clause("latency", int(np.median(st.tree_latency)), None)])
    eng.attribute()
    rc, y = read_again(eng, x)
    assert rc == 0
    same(y, x, "after a filter")
    # another extraction replaces it; LIST of the filter's trees
    z = eng.extract_traces("list", trees=f.match_trees[::-1])
    attr_host = traces.attribute_host(st, link, start, end, group, len(names))
    same(z, traces.extract_host(tf.with_match(st, f), link, kind, start, end, group, "list", trees=f.match_trees[::-1], attribution=attr_host,
                                single_rows=cap_of(lib)[0]), "list")
    assert z.has_times and (z.sel_flags & M).all()
    # ... and it goes with the forest
    eng.stitch(truth=True)
    assert eng._lib.tw_get_extracted(eng._h, ctypes.byref(none)) == -4
    assert eng.extract_traces("top", "tree", 1, need_flags=W | M).n_trees == 0       # (a new forest without the bit)
    return eng, units, rows, st


def test_state_and_arguments(emu_lib, tmp_path):
    eng, units, rows, st = run_state(emu_lib, tmp_path)
    # a forest of a pass: score_traces rewrites the CONFIDENT bit and leaves the result; a new pass drops the forest and the result
    eng.run_pass1()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    refused(-4, eng.extract_traces)
    st = eng.stitch()
    x = eng.extract_traces("top", "fastest", 3)
    eng.score_traces(0.0)
    rc, y = read_again(eng, x)
    assert rc == 0
    same(y, x, "after score_traces")
    eng.run_pass1()
    import ctypes
    from traceweaver_amd import _ffi
    assert eng._lib.tw_get_extracted(eng._h, ctypes.byref(_ffi.Extracted())) == -4
    eng.load([u.arrays for u in units])
    refused(-4, eng.extract_traces)
    eng.close()


@pytest.mark.gpu
def test_state_and_arguments_gpu(tmp_path):
    run_state(None, tmp_path)[0].close()


# ---- 6. Jaeger round trip -------------------------------------------------------------------------------------------------------------
def test_jaeger_round_trip(emu_lib, tmp_path):
    from traceweaver_amd.ingest import open_directory

    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, emu_lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table)
    eng = ts.solve(emu_lib, units, n_traces, rows)
    eng.set_row_groups(group, len(names))
    eng.stitch()
    eng.attribute()
    x = eng.extract_traces("top", "slowest", 20)
    twice = eng.extract_traces("list", trees=[int(x.sel_tree[0])] * 2)
    eng.close()
    assert x.n_trees == 20 and x.has_times
    out = str(tmp_path / "jaeger")
    paths = traces.write_jaeger(out, x, corpus, table)
    assert len(paths) == len(set(paths)) == 20 and sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in paths)
    span_id = [corpus.string(s) for s in table["span_id"]]
    # (a) the files as JSON
    for j, p in enumerate(paths):
        t = x.trace(j)
        doc = json.load(open(p))
        assert list(doc) == ["data"] and len(doc["data"]) == 1
        tr = doc["data"][0]
        assert tr["traceID"] == "tw-" + span_id[t["root"]] and len(tr["spans"]) == t["subtree"][0]
        for i, sp in enumerate(tr["spans"]):
            r = int(t["row"][i])
            tags = {g["key"]: g["value"] for g in sp["tags"]}
            assert sp["spanID"] == span_id[r] and sp["startTime"] == table["start"][r] and sp["duration"] == table["duration"][r]
            assert sp["operationName"] == corpus.string(table["op_name"][r])
            assert tr["processes"][sp["processID"]]["serviceName"] == corpus.string(table["service"][r])
            assert tags["span.kind"] == {1: "server", 2: "client"}[int(t["kind"][i])] and tags["tw.hop"] == {1: "observed", 2: "predicted"}[int(t["kind"][i])]
            assert tags["tw.self_us"] == t["self_time"][i] and tags["tw.path_us"] == t["path_time"][i]
            if i == 0:
                assert sp["references"] == []
            else:
                assert sp["references"] == [{"refType": "CHILD_OF", "traceID": tr["traceID"], "spanID": span_id[int(t["row"][t["parent"][i]])]}]
    # (b) the project's loader reads them as it reads a corpus: the reloaded parent column is the extracted one
    again, _ = open_directory(out, lib_path=emu_lib, max_traces=0, cache=False, first_span=None, fix=None)
    t2 = again.span_table()
    assert again.counts()["traces"] == 20 and len(t2["span_id"]) == len(x.row)
    at = {again.string(s): k for k, s in enumerate(t2["span_id"])}
    assert len(at) == len(x.row)
    for j in range(20):
        t = x.trace(j)
        ids = [span_id[int(r)] for r in t["row"]]
        got = [int(t2["parent"][at[s]]) for s in ids]
        assert got == [-1 if p < 0 else at[ids[p]] for p in t["parent"].tolist()], j
    # duplicates of a list do not collide
    dup = traces.write_jaeger(str(tmp_path / "dup"), twice, corpus, table)
    assert len(set(dup)) == 2 and dup[1].endswith("-1.json")


# ---- 7. the command line ------------------------------------------------------------------------------------------------------------
def test_cli_traces_out(emu_lib, tmp_path, capsys):
    """--traces_out with each selector writes what extract_host gives for the same query on the run's forest, which the run's
    --stitch_out and --attribute_out files hold."""
    from collections import namedtuple

    from traceweaver_amd import executor
    from traceweaver_amd.ingest import REFERENCE_FIX, open_directory

    d = str(tmp_path / "corpus")
    synth.write_jaeger_corpus(d, 11, 300, app=synth.HOTEL_APP, concurrency=2.5)
    base = ["--absolute_path", d, "--cache_rate", "0", "--fix", "2", "--test_name", "gen", "--load_level", "7", "--engine_library", emu_lib]
    f = lambda name: str(tmp_path / name)
    runs = {"top": ["--traces_out", f("top"), "--traces_top", "5", "--traces_format", "npz", "--attribute_out", f("a.npz"), "--stitch_out", f("s.npz"), "-v"],
            "default": ["--traces_out", f("default"), "--traces_format", "npz", "--profiles_out", f("p.npz")],
            "quantiles": ["--traces_out", f("quantiles"), "--traces_quantiles", "0.5,0.99", "--traces_format", "npz"]}
    text = {}

    def run(tag, extra):
        executor.main(base + ["--results_directory", f("out_" + tag) + "/"] + extra)
        text[tag] = capsys.readouterr().out

    for tag, extra in runs.items():
        run(tag, extra)
    expr = "latency>=%d" % int(np.median(np.load(f("s.npz"))["tree_latency"]))          # (the forest is the same in every run)
    run("matched", ["--traces_out", f("matched"), "--traces_matched", "1", "--trace_filter", expr, "--filter_out", f("f.npz")])
    first_span, fix = REFERENCE_FIX[2]
    corpus, _ = open_directory(d, lib_path=emu_lib, first_span=first_span, fix=fix, max_traces=1001)
    table = corpus.span_table()
    group, names = traces.groups_from_table(table, corpus)
    z, a, flt = np.load(f("s.npz")), np.load(f("a.npz")), np.load(f("f.npz"))
    st = traces.StitchedTraces(*[z[k] for k in traces.StitchedTraces.FIELDS])
    times = namedtuple("Times", "self_time path_time")(a["self_time"], a["path_time"])
    host = lambda stitched=st, attribution=None, **q: traces.extract_host(stitched, a["link"], z["row_kind"], z["row_start"], z["row_end"], group,
                                                                          attribution=attribution, single_rows=12, **q)

    def written(tag, want):
        got = np.load(os.path.join(f(tag), "traces.npz"))
        for k in X.FIELDS:
            assert np.array_equal(got[k], getattr(want, k)) and got[k].dtype == getattr(want, k).dtype, (tag, k)
        assert got["group_names"].tolist() == [str(x) for x in names]
        return want

    top = written("top", host(mode="top", order="slowest", limit=5, attribution=times))
    assert top.n_trees == 5 and top.has_times
    assert "Extracted traces: 5 of %d eligible, %d rows, with self and path times -> %s" % (top.n_eligible, top.summary[2], f("top")) in text["top"].splitlines()
    assert top.render(0, [str(x) for x in names]) in text["top"] and top.render(2, [str(x) for x in names]) in text["top"]
    # without a selector: the 20 slowest; the times of --profiles_out's attribution, which are every row's
    assert written("default", host(mode="top", order="slowest", limit=20, attribution=times)).n_trees == 20
    q = written("quantiles", host(mode="quantiles", probs=(0.5, 0.99)))
    assert q.n_trees == 2 and not q.has_times and "trace 0:" not in text["quantiles"]
    # the matched traces as Jaeger files: one per trace, named by the root's span
    marked = with_flags(st, st.tree_flags | (M * flt["tree_match"]))
    m = host(marked, mode="top", order="tree", need_flags=W | M)
    assert 0 < m.n_trees == flt["summary"][1] < m.n_eligible + 1 and m.n_trees < int(((st.tree_flags & W) != 0).sum())
    assert sorted(os.listdir(f("matched"))) == sorted("tw-%s.json" % corpus.string(table["span_id"][r]) for r in m.sel_root)
    for j in (0, m.n_trees - 1):
        doc = json.load(open(os.path.join(f("matched"), "tw-%s.json" % corpus.string(table["span_id"][m.sel_root[j]]))))
        assert [s["spanID"] for s in doc["data"][0]["spans"]] == [corpus.string(table["span_id"][r]) for r in m.trace(j)["row"]]
    # refusals
    for extra in (["--traces_out", f("x"), "--traces_matched", "1"], ["--traces_top", "3"], ["--traces_out", f("x"), "--traces_top", "3", "--traces_quantiles", "0.5"],
                  ["--traces_out", f("x"), "--traces_quantiles", "0.5,1.5"], ["--traces_out", f("x"), "--traces_top", "-1"], ["--traces_out", f("x"), "--cache_rate", "0.1"],
                  ["--traces_out", f("x"), "--predictor_indices", "3"]):
        with pytest.raises(SystemExit):
            executor.main([x for x in base if x not in ("--cache_rate", "0")] + (["--cache_rate", "0"] if "--cache_rate" not in extra else []) +
                          ["--results_directory", f("refused") + "/"] + extra)
    assert not os.path.exists(f("x"))
