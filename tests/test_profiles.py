"""Engine.class_profiles (tw_class_profiles, csrc/tw_prof.h): the aggregate trace of every call-graph class -- per signature entry the
rows, durations, self and critical-path times and start offsets of the trees of the class that the attribution selected.  The
yardstick is traces.class_profiles_host, the definitions of include/traceweaver_amd.h restated with dictionaries from the host
results of signatures_host and attribute_host; part 1 checks it on the forest written out by hand in tests/test_signatures.py, the
rest compares the device with it, np.array_equal and equal dtype on every field of ClassProfiles.FIELDS.  Corpora, cases and helpers
are those of tests/test_stitch.py, tests/test_attribute.py and tests/test_signatures.py.  CPU tier: host-emulation build (an LDS
table of 8 entries: the table and the global cells both occur; one lane per workgroup, and once one host thread per lane); the HIP
library under -m gpu."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_attribute as ta
import test_signatures as tg
import test_stitch as ts
from traceweaver_amd import synth, traces
from traceweaver_amd.engine import Engine, EngineError

I64 = np.iinfo(np.int64)


def same(got, want, tag=None):
    for k in traces.ClassProfiles.FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), (k, tag)
        assert getattr(got, k).dtype == getattr(want, k).dtype == np.int64, (k, tag)


def check_invariants(p, sig, tag=None):
    """What holds for every profile: rows = count * counted, and the sums that two fields share."""
    counted = np.repeat(p.class_counted, np.diff(sig.class_off))
    assert np.array_equal(p.rows, sig.class_entries[:, 3].astype(np.int64) * counted), tag
    assert np.array_equal(p.class_off, sig.class_off) and np.array_equal(p.class_entries, sig.class_entries) and p.mode == sig.mode
    assert (p.path_rows <= p.rows).all() and (p.path_trees <= np.minimum(p.path_rows, counted)).all() and ((p.path_trees > 0) == (p.path_rows > 0)).all()
    assert ((p.span_min == I64.max) == (p.rows == 0)).all() and ((p.span_max == I64.min) == (p.rows == 0)).all()
    s = p.summary.tolist()
    assert s[0] == p.class_counted.sum() and s[1] == (p.class_counted > 0).sum() and s[2] == p.rows.sum() and s[3] == (p.rows > 0).sum()
    assert s[0] + s[4] == (sig.tree_class >= 0).sum()
    assert np.array_equal(p.class_path_time, np.add.reduceat(np.append(p.path_time, 0), sig.class_off[:-1]) * (np.diff(sig.class_off) > 0))


# ---- 1. the restatement on the forest written out by hand ---------------------------------------------------------------------
def hand(mode, percentile=0.0, sig_need=1, attr_need=traces.WHOLE, attr_skip=traces.UNASSIGNED):
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
    sig = traces.signatures_host(st, link, kind, group, 4, mode, sig_need, 0)
    attr = traces.attribute_host(st, link, start, end, group, 4, percentile, need_flags=attr_need, skip_flags=attr_skip)
    p = traces.class_profiles_host(st, sig, attr, link, kind, start, end, group)
    check_invariants(p, sig)
    return p, sig, attr


def test_host_by_hand():
    # levels: class 0 = trees 0, 1, 8 (latencies 100, 250, 400), entries A, B, C, D.  Every row but a root is [base + 1, base + 2]: the
    # root's walk takes its first client row, so in trees 0 and 8 the path is A, B, D and in tree 1 (D under C) it is A, C, D
    p, sig, attr = hand("levels")
    assert attr.tree_selected.tolist() == [1, 1, 1, 1, 1, 0, 0, 1, 1]
    assert p.class_counted.tolist() == [3, 1, 1, 1, 1] and p.class_latency.tolist() == [750, 50, 70, 10, 30]
    assert p.rows.tolist() == [3, 3, 3, 3, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1] and p.rows[:4].tolist() == (sig.entries(0)[:, 3] * 3).tolist()
    assert p.span_time[0] == 750 and p.offset[0] == 0 and p.span_min[0] == 100 and p.span_max[0] == 400
    assert p.span_time[1:4].tolist() == [3, 3, 3] and p.offset[1:4].tolist() == [3, 3, 3] and p.span_min[1] == p.span_max[1] == 1
    assert p.path_rows[:4].tolist() == [3, 2, 1, 3] and p.path_trees[:4].tolist() == [3, 2, 1, 3]
    assert p.path_time[:4].tolist() == [747, 0, 0, 3] and p.self_time[0] == 747      # a root's own time: its duration less [1, 2]
    assert p.class_top_entry.tolist() == [0, 4, 8, -1, 12] and p.class_path_time.tolist() == [750, 50, 70, 0, 30]
    assert p.summary.tolist() == [7, 5, 23, 14, 0, 0]
    assert p.entry(1) == {"entry": 1, "class": 0, "level": 1, "caller": 0, "group": tg.B, "count": 1, "rows": 3, "span_time": 3, "span_min": 1,
                          "span_max": 1, "self_time": 1, "path_time": 0, "path_rows": 2, "path_trees": 2, "offset": 3}
    assert [e["entry"] for e in p.profile(0)] == [0, 1, 2, 3] and p.profile(3) == []
    t = p.table(["a", "b", "c", "d"])
    assert [r["class"] for r in t] == [0, 1, 2, 3, 4] and t[0]["counted"] == 3 and t[0]["mean_latency"] == 250.0
    assert t[0]["top"] == (0, None, "a") and t[0]["top_share"] == 747.0 / 750.0 and t[0]["top_trees"] == 1.0 and t[3]["top"] is None
    with pytest.raises(IndexError):
        p.entry(14)
    # edges: trees 0 and 1 part, class 0 = trees 0 and 8
    p, sig, _ = hand("edges")
    assert p.class_counted.tolist() == [2, 1, 1, 1, 1, 1] and p.rows[:4].tolist() == [2, 2, 2, 2] and p.rows[:4].tolist() == (sig.entries(0)[:, 3] * 2).tolist()
    assert p.span_time[0] == 500 and p.offset[0] == 0 and p.class_latency[0] == 500 and p.class_top_entry[0] == 0
    assert p.path_rows[:4].tolist() == [2, 2, 0, 2] and p.path_rows[4:8].tolist() == [1, 0, 1, 1]
    assert p.summary.tolist() == [7, 6, 23, 18, 0, 0] and p.table()[0]["top"] == (0, -1, tg.A)


def test_host_selection_by_hand():
    # percentile 0.5: of the seven whole trees the four slowest (3, 0, 1, 8) are selected; trees 2, 4 and 7 keep a class but count nowhere
    p, sig, attr = hand("levels", 0.5)
    assert attr.tree_selected.tolist() == [1, 1, 0, 1, 0, 0, 0, 0, 1]
    assert p.class_counted.tolist() == [3, 0, 1, 0, 0] and p.rows.tolist() == [3] * 4 + [0] * 4 + [1] * 4 + [0] * 2
    assert p.span_time[0] == 750 and p.offset[0] == 0 and p.class_top_entry.tolist() == [0, -1, 8, -1, -1]
    assert p.span_min[4] == I64.max and p.span_max[4] == I64.min
    assert p.summary.tolist() == [4, 2, 16, 8, 3, 0] and [r["class"] for r in p.table()] == [0, 2]
    p, _, _ = hand("edges", 0.5)
    assert p.class_counted.tolist() == [2, 1, 0, 1, 0, 0] and p.rows[:4].tolist() == [2] * 4 and p.summary.tolist() == [4, 3, 16, 12, 3, 0]
    # every tree has a class (need_flags = 0 on the signature side only): the two fragments are classed but not selected
    p, sig, _ = hand("levels", sig_need=0)
    assert sig.tree_class.tolist() == [0, 0, 1, 2, 3, 3, 4, 5, 0] and p.class_counted.tolist() == [3, 1, 1, 1, 0, 1]
    assert p.rows.tolist() == [3] * 4 + [1, 1, 2, 1] + [1] * 4 + [0] + [1] * 2 and p.summary.tolist() == [7, 5, 23, 14, 2, 0]
    # ... and the other way round: every tree selected (need_flags = 0 on the attribution's side only), the fragments have no class
    p, sig, attr = hand("levels", attr_need=0, attr_skip=0)
    assert attr.tree_selected.tolist() == [1] * 9 and p.class_counted.tolist() == [3, 1, 1, 1, 1] and p.summary.tolist() == [7, 5, 23, 14, 0, 2]


def test_table_cells_mirror_the_header():
    text = open(os.path.join(os.path.dirname(os.path.abspath(traces.__file__)), "csrc", "tw_prof.h")).read()
    assert [int(x) for x in re.findall(r"^#define TW_PROF_TABLE_CELLS (\d+)", text, flags=re.M)] == [traces.PROFILE_TABLE_CELLS]


# ---- 2. device = restatement ----------------------------------------------------------------------------------------------
PERCENTILES = (0.0, 0.5)


def check(eng, st, link, rows, group, n_groups, mode, need, skip, attr_host, tag=None, **query):
    """signatures(mode, need, skip) and class_profiles() on the forest last stitched and attributed against the restatement."""
    sig = eng.signatures(mode, need, skip)
    dev = eng.class_profiles()
    want_sig = traces.signatures_host(st, link, rows[3], group, n_groups, mode, need, skip)
    want = traces.class_profiles_host(st, want_sig, attr_host, link, rows[3], rows[4], rows[5], group)
    same(dev, want, tag)
    check_invariants(dev, sig, tag)
    return dev


def note(seen, p):
    counted = np.repeat(p.class_counted, np.diff(p.class_off))
    seen["counted"] = max(seen["counted"], int(p.class_counted.max()) if p.n_classes else 0)
    seen["off_path_trees"] = seen["off_path_trees"] or bool(((p.path_trees > 0) & (p.path_trees < counted)).any())
    seen["off_path_rows"] = seen["off_path_rows"] or bool(((p.path_rows > 0) & (p.path_rows < p.rows)).any())
    seen["unselected"] = seen["unselected"] or p.summary[4] > 0


def check_forest(eng, st, link, rows, groupings, seen, tag):
    start, end = np.asarray(rows[4]), np.asarray(rows[5])
    for group, G in groupings:
        eng.set_row_groups(group, G)
        for pct in PERCENTILES:
            attr = eng.attribute(pct)
            attr_host = traces.attribute_host(st, link, start, end, group, G, pct)
            assert np.array_equal(attr.tree_selected, attr_host.tree_selected)
            for need, skip in tg.FLAG_QUERIES:
                for mode in (0, 1):
                    note(seen, check(eng, st, link, rows, group, G, mode, need, skip, attr_host, (tag, G, pct, mode, need, skip)))
    t = eng.profiles_timing()
    assert list(t) == ["sweep", "classes", "copies"] and all(v >= 0 for v in t.values())


def run_case(lib, tmp_path, name, seed, n, concurrency, expect, seen):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    groupings = [traces.groups_from_table(table), tg.blind_groups(rows)]
    groupings[0] = (groupings[0][0], len(groupings[0][1]))
    arrays = [u.arrays for u in units]
    par = [r["parent"] for r in eng.results(2, fields=("parent",))]
    check_forest(eng, eng.stitch(), ta.links_of(arrays, par, rows), rows, groupings, seen, (name, "pass 2"))
    check_forest(eng, eng.stitch(truth=True), ta.links_of(arrays, [u.true_parent for u in units], rows), rows, groupings, seen, (name, "truth"))
    eng.close()


def run_cases(lib, tmp_path, cases):
    seen = {"counted": 0, "off_path_trees": False, "off_path_rows": False, "unselected": False}
    for c in cases:
        run_case(lib, tmp_path, *c, seen=seen)
    # what the test is about occurred: a class of three counted trees and more, an entry that is on the path in some of its class'
    # counted trees only, one with rows on and off the path, a class with trees that the attribution did not select
    assert seen["counted"] >= 3 and seen["off_path_trees"] and seen["off_path_rows"] and seen["unselected"], seen


def test_device_equals_host_restatement(emu_lib, tmp_path):
    run_cases(emu_lib, tmp_path, tg.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("half", (0, 1))
def test_device_equals_host_restatement_gpu(tmp_path, half):
    run_cases(None, tmp_path, tg.CASES[2 * half:2 * half + 2])


# ---- 3. sizes and routes ------------------------------------------------------------------------------------------------------
N_PAIRS = 400     # distinct two-item classes of the wide table, two trees each: 800 entries, beyond the LDS table of either build


def wide_table(n_pairs=N_PAIRS):
    """One service of 2 * N_PAIRS requests with one call each, as pass-0 parents: every tree is the request row (group a), its call and
    one callee row (group b) -- three rows, two items, each inside the one above it, so that all three are on the critical path; the
    neighbours 2 c and 2 c + 1 share the pair (a, b) = (c % 20, 20 + c // 20): two lanes of a wavefront meet on every cell."""
    n = 2 * n_pairs
    u, tp = synth.make_unit(3, n, shape="single")
    pair = np.arange(n) // 2
    kind = np.array([1] * n + [2] * n + [1] * n, dtype=np.uint8)
    link = np.concatenate([np.full(2 * n, -1), n + np.asarray(tp[0])]).astype(np.int32)
    group = np.concatenate([pair % 20, np.full(n, -1), 20 + pair // 20]).astype(np.int32)
    base = 1000 * np.arange(n, dtype=np.int64)
    call = base[np.argsort(np.asarray(tp[0]))]                    # (the request whose call x is: the call lies inside it)
    start = np.concatenate([base, call + 10, base + 20])
    end = np.concatenate([base + 900, call + 800, base + 21 + (np.arange(n) * 37) % 500])
    rows = ([np.arange(n, dtype=np.int32)], [[np.arange(n, 2 * n, dtype=np.int32)]], link, kind, start, end)
    return u, tp, rows, group, 20 + (n_pairs + 19) // 20


def table_engine(lib, table):
    u, tp, rows, group, G = table
    eng = Engine(0, lib_path=lib)
    eng.load([u])
    eng.set_span_rows(*rows)
    eng.set_parents([tp])
    eng.set_row_groups(group, G)
    st = eng.stitch(0)
    return eng, st, ta.links_of([u], [tp], rows), rows, group, G


def run_sizes(lib, modes=(0, 1)):
    """sized_table of tests/test_signatures.py: trees of 0, 1, 63, 64, 65, 300 and 600 items, either side of a wavefront and of the
    LDS table of either build; tree 7 puts 300 rows into one cell; 300 classes of two items: many cells with one row each."""
    eng, st, link, rows, group, G = table_engine(lib, tg.sized_table())
    attr = eng.attribute()
    attr_host = traces.attribute_host(st, link, rows[4], rows[5], group, G)
    n = len(tg.SIZES) + 1 + tg.N_DISTINCT
    for mode in modes:
        p = check(eng, st, link, rows, group, G, mode, 1, 0, attr_host, ("sizes", mode))
        assert p.n_classes == n and (p.class_counted == 1).all() and p.summary[:2].tolist() == [n, n]
        a = int(p.class_off[7])
        assert p.rows[a:a + 2].tolist() == [1, 300] and p.path_trees[a] == 1
        assert p.summary[2] == sum(tg.SIZES) + 301 + 2 * tg.N_DISTINCT + (np.arange(tg.N_DISTINCT) % 3 > 0).sum()
    eng.close()


def run_wide(lib, n_pairs=N_PAIRS):
    eng, st, link, rows, group, G = table_engine(lib, wide_table(n_pairs))
    assert st.n_trees == 2 * n_pairs and (np.diff(st.tree_off) == 3).all()
    attr = eng.attribute()
    attr_host = traces.attribute_host(st, link, rows[4], rows[5], group, G)
    for mode in (0, 1):
        p = check(eng, st, link, rows, group, G, mode, 1, 0, attr_host, ("wide", mode))
        assert p.n_entries == 2 * n_pairs and (n_pairs < N_PAIRS or p.n_entries > traces.PROFILE_TABLE_CELLS)   # the HIP build's route onto the global cells
        assert p.n_classes == n_pairs and (p.class_counted == 2).all() and (p.rows == 2).all() and (p.path_trees == 2).all()
        # of a request's 900 us its call covers 790; the callee, a leaf, is on the path for all of its duration
        assert (p.path_time[0::2] == 220).all() and np.array_equal(p.path_time[1::2], p.span_time[1::2]) and (p.offset[1::2] == 40).all()
    eng.close()


def test_sizes_and_routes(emu_lib):
    run_sizes(emu_lib)
    run_wide(emu_lib)


@pytest.mark.gpu
def test_sizes_and_routes_gpu():
    run_sizes(None)
    run_wide(None)


def test_sizes_lane_threaded(emu_lib):
    """One host thread per lane (TW_EMU_LANES=1, workgroups of 256): the ballots, shuffles and exchanges of k_prof_rows and
    k_prof_trees run as they are written, 64 lanes to a wavefront and four wavefronts on one LDS table, without a GPU.  (The wide table
    with 16 pairs: two lanes of a wavefront on every cell, all of them on the path.)"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "import test_profiles as t\n"
            "t.run_sizes(%r, (1,))\n"
            "t.run_wide(%r, 16)\n"
            "print('child ok')\n") % (os.path.dirname(here), here, emu_lib, emu_lib)
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stderr[-2000:]


# ---- 4. state -------------------------------------------------------------------------------------------------------------------
def run_state(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table)
    G = len(names)
    arrays = [u.arrays for u in units]
    eng = ts.solve(lib, units, n_traces)

    def refused():
        with pytest.raises(EngineError) as ex:
            eng.class_profiles()
        assert ex.value.code == -4 and "TW_ERR_STATE" in str(ex.value)

    def both(mode=0):
        eng.attribute(0.5)
        eng.signatures(mode)
        return eng.class_profiles()

    refused()                                                     # before anything
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, G)
    st = eng.stitch()
    refused()                                                     # a forest, neither stage
    eng.attribute(0.5)
    refused()                                                     # ... before signatures
    eng.stitch()
    eng.signatures()
    refused()                                                     # ... before an attribution on this forest
    first = both()
    assert first.n_counted > 0 and first.summary[4] > 0
    link = ta.links_of(arrays, [r["parent"] for r in eng.results(2, fields=("parent",))], rows)
    attr_host = traces.attribute_host(st, link, rows[4], rows[5], group, G, 0.5)
    # the two-call pattern: the second call copies what is resident and runs no kernel
    t0 = eng.profiles_timing()
    again = eng.class_profiles()
    assert again.same_as(first) and eng.profiles_timing() == t0
    import ctypes
    summary = np.zeros(6, dtype=np.int64)
    assert eng._lib.tw_class_profiles(eng._h, None, summary.ctypes.data_as(ctypes.c_void_p)) == 0 and np.array_equal(summary, first.summary)
    # the call drops nothing: the other consumers answer what they answered before it
    d, s = eng.distributions((0.5, 0.9), (1000, 5000)), eng.signatures()
    assert eng.class_profiles().same_as(first)
    assert eng.distributions((0.5, 0.9), (1000, 5000)).same_as(d) and eng.signatures().same_as(s) and eng.profiles_timing() == t0
    # a signature call with another query replaces the result: the profile is computed again, for it
    eng.signatures(1, 0, 0)
    other = check(eng, st, link, rows, group, G, 1, 0, 0, attr_host, "another query")
    assert other.mode == 1 and other.summary[0] == first.summary[0]
    assert both().same_as(first)
    for event in ("stitch", "set_row_groups", "score_traces", "attribute", "run_pass1", "load"):
        if event == "stitch":
            eng.stitch()
        elif event == "set_row_groups":
            eng.set_row_groups(group, G)
        elif event == "score_traces":
            eng.score_traces(0.0)                                 # drops the signature result
        elif event == "attribute":
            eng.attribute(0.0)                                    # another selection: not refused, computed again
            assert eng.class_profiles().n_counted > first.n_counted
            continue
        elif event == "run_pass1":
            eng.run_pass1()
        else:
            eng.load(arrays)
            eng.run_pass1()
            eng.fit_mixtures(seed=0)
            eng.run_pass2()
            eng.set_span_rows(*rows)
        refused()
        if event == "set_row_groups":
            eng.signatures()
            refused()                                             # the signatures alone do not bring it back
        if event == "run_pass1":
            eng.fit_mixtures(seed=0)
            eng.run_pass2()
        if event in ("run_pass1", "load"):
            eng.set_row_groups(group, G)
            eng.stitch()
        assert both().same_as(first), event                       # both stages rerun: the engine answers again, and the same
    eng.close()


def test_state(emu_lib, tmp_path):
    run_state(emu_lib, tmp_path)


@pytest.mark.gpu
def test_state_gpu(tmp_path):
    run_state(None, tmp_path)   # (all refused on the host: nothing malformed reaches the device)


# ---- 5. the command line --------------------------------------------------------------------------------------------------------
def test_cli_profiles_out(emu_lib, tmp_path, capsys):
    """--profiles_out on the generated hotel corpus of test_cli_stitch_out: the pickles stay as they are; the predicted side equals
    the same engine calls made by hand on the links the run's own --attribute_out file holds, the true side the restatement."""
    from traceweaver_amd import executor
    from traceweaver_amd.ingest import REFERENCE_FIX, open_directory

    synth.write_jaeger_corpus(str(tmp_path / "corpus"), 11, 400, app=synth.HOTEL_APP, concurrency=2.5)
    base = ["--absolute_path", str(tmp_path / "corpus"), "--cache_rate", "0", "--fix", "2", "--test_name", "gen", "--load_level", "7",
            "--engine_library", emu_lib]
    query = ["--query_percentile", "0.5", "--signature_mode", "edges"]
    runs, text = {}, {}
    for tag, extra in (("plain", []), ("profiles", ["--profiles_out", str(tmp_path / "prof.npz"), "--attribute_out", str(tmp_path / "attr.npz"),
                                                     "--stitch_out", str(tmp_path / "traces.npz")] + query),
                       ("alone", ["--profiles_out", str(tmp_path / "alone.npz")] + query)):
        out = str(tmp_path / tag) + "/"
        executor.main(base + ["--results_directory", out] + extra)
        runs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        text[tag] = capsys.readouterr().out
    assert len(runs["plain"]) == 5 and runs["plain"] == runs["profiles"] == runs["alone"]        # the five pickles, byte for byte
    z, alone = np.load(str(tmp_path / "prof.npz")), np.load(str(tmp_path / "alone.npz"))
    assert sorted(z.files) == sorted(alone.files) and all(np.array_equal(z[k], alone[k]) for k in z.files)
    assert str(z["mode"]) == "edges"
    first_span, fix = REFERENCE_FIX[2]
    corpus, _ = open_directory(str(tmp_path / "corpus"), lib_path=emu_lib, first_span=first_span, fix=fix, cache=False)
    units, skipped, n_traces = corpus.units()
    table = corpus.span_table()
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table, corpus)
    assert z["group_names"].tolist() == [str(x) for x in names]
    arrays, truth = [u.arrays for u in units], [u.true_parent for u in units]
    # the run's parent arrays, read off the links of its attribution file
    link = np.load(str(tmp_path / "attr.npz"))["link"]
    par = []
    for u in units:
        request = {int(r): i for i, r in enumerate(u.in_rows)}
        p = np.full((u.arrays.E, u.arrays.n_in), -1, dtype=np.int32)
        for e, per in enumerate(u.out_rows):
            for x, r in enumerate(per):
                if link[r] >= 0:
                    p[e, request[int(link[r])]] = x
        par.append(p)
    eng = Engine(0, lib_path=emu_lib)
    eng.load(arrays)
    eng.set_truth(truth, [u.in_trace for u in units], n_traces)
    eng.set_span_rows(*rows)
    eng.set_parents(par)
    eng.set_row_groups(group, len(names))
    st = eng.stitch(0)
    s = np.load(str(tmp_path / "traces.npz"))
    assert st.same_as(traces.StitchedTraces(*[s[k] for k in traces.StitchedTraces.FIELDS]))  # the forest the run stitched
    sig = eng.signatures("edges")
    eng.attribute(0.5)
    pred = eng.class_profiles()
    tt = eng.stitch(truth=True)
    eng.close()
    for k in traces.ClassProfiles.FIELDS + ("class_off", "class_entries"):
        assert np.array_equal(z[k], getattr(pred, k)), k
    tlink = ta.links_of(arrays, truth, rows)
    want = traces.class_profiles_host(tt, traces.signatures_host(tt, tlink, rows[3], group, len(names), "edges"),
                                      traces.attribute_host(tt, tlink, rows[4], rows[5], group, len(names), 0.5), tlink, rows[3], rows[4], rows[5], group)
    for k in traces.ClassProfiles.FIELDS + ("class_off", "class_entries"):
        assert np.array_equal(z["true_" + k], getattr(want, k)), k
    assert want.n_counted == n_traces - int(0.5 * n_traces)
    # the printed lines: the counts, then the largest classes with their top entry
    lines = text["profiles"].splitlines()
    head = [x for x in lines if x.startswith("Class profiles (edges):")]
    assert head == ["Class profiles (edges): %d traces of %d call graphs counted, %d rows in %d entries; true traces: %d of %d"
                    % (pred.summary[0], pred.summary[1], pred.summary[2], pred.summary[3], want.summary[0], want.summary[1])]
    t = pred.table([str(x) for x in names])
    assert 0 < len(t) and "Class profiles" not in text["plain"]
    at = lines.index(head[0])
    for k, row in enumerate(t[:3]):
        lv, cg, g = row["top"]
        assert lines[at + 1 + k] == "  class %d: %d traces, mean %.1f us; on the path most: L%d %s>%s, %.1f %% of the path time, in %.1f %% of the traces" % (
            row["class"], row["counted"], row["mean_latency"], lv, cg, g, 100.0 * row["top_share"], 100.0 * row["top_trees"])
    bad = [x for x in base if x not in ("--cache_rate", "0")] + ["--results_directory", str(tmp_path) + "/", "--profiles_out", "p.npz"]
    for extra in (["--cache_rate", "0.1"], ["--cache_rate", "0", "--predictor_indices", "3"], ["--cache_rate", "0", "--query_percentile", "1"]):
        with pytest.raises(SystemExit):
            executor.main(bad + extra)
