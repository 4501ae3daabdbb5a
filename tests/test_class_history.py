"""Engine.class_history_* (tw_class_history_reset / _push / _match / _merge / _info / _get, csrc/tw_chist.h): the call-graph classes
of batch after batch kept in a catalogue on the device -- ids that hold across batches, per-class and per-entry figures that add up
across them.  The yardstick is traces.class_history_host, a dict keyed by the signature tuple with Python integers; part 1 checks
the restatement by hand, the rest compares the device with it, np.array_equal on every field of ClassHistory.FIELDS.  Corpora, cases
and helpers are those of tests/test_stitch.py, test_signatures.py, test_profiles.py and test_history.py.  CPU tier: host-emulation
build (a hash table of 8 slots at first, so a few dozen classes refill it several times; one lane per workgroup, and once one host
thread per lane); the HIP library, whose table starts with 1024 slots, under -m gpu."""
import os

import numpy as np
import pytest

import test_attribute as ta  # noqa: F401  (test_distributions imports it by this name)
import test_distributions as td
import test_history as th
import test_profiles as tp
import test_signatures as tg
import test_stitch as ts
from traceweaver_amd import synth, traces
from traceweaver_amd.engine import Engine
from traceweaver_amd.traces import ClassHistory, ClassProfiles, TraceSignatures

MAX, MIN = traces.INT64_MAX, traces.INT64_MIN
SLOTS_EMU, SLOTS_GPU = 8, 1024                                    # kChistSlots of csrc/tw_chist.h under TW_TILE_SMALL / in the HIP build
ADDITIVE = ("trees", "latency_sum", "counted", "latency") + tuple(f for f in ClassHistory.ENTRY_FIELDS if f not in ("span_min", "span_max"))
error = th.error


def same(dev, want, tag=None, fields=ClassHistory.FIELDS):
    assert dev.mode == want.mode, tag
    for k in fields:
        got, exp = getattr(dev, k), getattr(want, k)
        assert got.dtype == exp.dtype and np.array_equal(got, exp), (k, tag)


def i64(x):
    return np.array(x, dtype=np.int64)


# ---- 1. the restatement by hand ---------------------------------------------------------------------------------------------
A = ((0, -1, 0, 1), (1, 0, 1, 2))
B = ((0, -1, 0, 1), (1, 0, 1, 3))                                  # A but for the last entry's count
C = ((0, -1, 2, 1),)
NONE = ()                                                         # the empty signature: a class like any other
LONG = tuple((lv, -1 if lv == 0 else (lv - 1) % 3, lv % 3, 1 + lv % 2) for lv in range(70))   # more entries than a wavefront has lanes
G, NAMES = 3, ["a", "b", "c"]


def batch(sigs, trees, lsum, lmin, lmax, counted, latency, cells, mode=1):
    """A signature result and its class profile from literals: cells = the nine entry fields in the order of PROFILE_ENTRY_FIELDS."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    entries = np.array([e for s in sigs for e in s], dtype=np.int32).reshape(-1, 4)
    nc, none = len(sigs), np.zeros(0, dtype=np.int32)
    sig = TraceSignatures(none, none, i64([]), np.zeros(0, dtype=np.uint8), np.arange(nc, dtype=np.int32), i64(trees), i64(lsum), i64(lmin), i64(lmax), off,
                          entries, [sum(trees), nc, 0, len(entries), -1, -1], mode)
    prof = ClassProfiles(*([i64(c) for c in cells] + [i64(counted), i64(latency), i64([0] * nc), i64([-1] * nc), [0] * 6]), class_off=off, class_entries=entries,
                         mode=mode)
    return sig, prof


def hand_parts():
    p0 = batch([A, C], [3, 1], [30, 7], [5, 7], [20, 7], [2, 1], [25, 7],
               [[2, 4, 1], [10, 40, 7], [4, 6, 7], [6, 15, 7], [3, 30, 7], [10, 12, 7], [2, 1, 1], [2, 1, 1], [0, 8, 0]])
    p1 = batch([B, A], [1, 2], [9, 50], [9, 1], [9, 49], [1, 2], [9, 50],
               [[1, 3, 2, 4], [5, 9, 20, 10], [5, 2, 3, 1], [5, 4, 17, 5], [1, 9, 2, 10], [5, 0, 1, 30], [1, 0, 1, 2], [1, 0, 1, 2], [0, 3, 0, 6]])
    p2 = batch([C, A], [100, 100], [1000, 1000], [-5, -5], [999, 999], [1, 1], [4, 6],                   # pushed with what = 2: no trees, no latencies
               [[1, 1, 2], [4, 2, 4], [4, 2, 1], [4, 2, 3], [4, 1, 4], [4, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 2]])
    return [p0 + (3, 5), p1 + (3, 2), p2 + (2, 9)]


HAND_WANT = dict(
    class_off=[0, 2, 3, 5], trees=[5, 1, 1], latency_sum=[80, 7, 9], latency_min=[1, 7, 9], latency_max=[49, 7, 9], counted=[5, 2, 1], latency=[81, 11, 9],
    first_epoch=[2, 5, 2], last_epoch=[9, 9, 2], seen=[3, 2, 1],
    rows=[5, 10, 2, 1, 3], span_time=[32, 54, 11, 5, 9], span_min=[2, 1, 4, 5, 2], span_max=[17, 15, 7, 5, 4], self_time=[6, 44, 11, 1, 9],
    path_time=[11, 42, 11, 5, 0], path_rows=[3, 3, 2, 1, 0], path_trees=[3, 3, 2, 1, 0], offset=[0, 16, 0, 0, 3],
    class_path_time=[53, 11, 5], class_top_entry=[1, 2, 3])
HAND_MAPS = ([0, 1], [2, 0], [1, 0])
HAND_SUMMARIES = ([2, 2, 3, 3, 1, 2], [1, 3, 2, 5, 2, 2], [0, 3, 0, 5, 3, 2])


def check_hand(h):
    for k, v in HAND_WANT.items():
        assert getattr(h, k).tolist() == v and getattr(h, k).dtype == np.int64, k
    assert [h.signature(k) for k in range(3)] == [A, C, B] and h.class_entries.dtype == np.int32 and h.mode == 1
    t = h.table(NAMES)
    assert [r["id"] for r in t] == [0, 1, 2] and [r["trees"] for r in t] == [5, 1, 1]             # the tie of 1 and 2 by id
    assert t[0] == {"id": 0, "trees": 5, "share": 5.0 / 7, "mean_latency": 16.0, "min_latency": 1, "max_latency": 49, "first_epoch": 2, "last_epoch": 9,
                    "seen": 3, "top_entry": 1, "top": (1, "a", "b"), "top_share": 42.0 / 53, "signature": [(0, -1, "a", 1), (1, "a", "b", 2)]}
    assert t[2]["top"] == (0, -1, "a") and t[2]["top_share"] == 1.0 and t[1]["signature"] == [(0, -1, "c", 1)]
    assert h.entries(2).tolist() == [list(e) for e in B] and [r["rows"] for r in h.profile(0)] == [5, 10] and h.profile(2)[1]["entry"] == 4
    by = h.by_signature()
    assert set(by) == {A, B, C} and by[A]["trees"] == 5 and by[A]["top_entry"] == 1 and by[C]["top_entry"] == 0 and by[B]["rows"] == [1, 3]


def source(sig, prof, what, n_groups=G):
    """A part as Engine.class_history_merge takes it: the figures that `what` leaves out are None."""
    c = ClassHistory.from_batch(sig, prof if what & 2 else None, n_groups)
    if not what & 1:
        c.trees = c.latency_sum = c.latency_min = c.latency_max = None
    return c


def catalogue(sigs, mode=1, n_groups=G, **figures):
    off = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    return ClassHistory(off, np.array([e for s in sigs for e in s], dtype=np.int32).reshape(-1, 4), mode=mode, n_groups=n_groups,
                        **{k: i64(v) for k, v in figures.items()})


BAD_SOURCES = [
    ("two equal classes", lambda: catalogue([A, C, A])),
    ("two equal classes, one of them long", lambda: catalogue([LONG, NONE, LONG])),
    ("two empty classes", lambda: catalogue([NONE, B, NONE])),
    ("descending entries", lambda: catalogue([(A[1], A[0])])),
    ("a repeated key", lambda: catalogue([(A[0], A[0])])),
    ("g >= G", lambda: catalogue([((0, -1, 3, 1),)])),
    ("cg >= G", lambda: catalogue([((1, 3, 0, 1),)])),
    ("cg below -1", lambda: catalogue([((1, -2, 0, 1),)])),
    ("a negative level", lambda: catalogue([((-1, -1, 0, 1),)])),
    ("a level beyond 2^16", lambda: catalogue([((1 << 16, -1, 0, 1),)])),
    ("a count of 0", lambda: catalogue([((0, -1, 0, 0),)])),
    ("another mode", lambda: catalogue([((0, 0, 0, 1),)], mode=0)),
    ("another n_groups", lambda: catalogue([C], n_groups=4)),
]


def test_host_by_hand():
    parts = hand_parts()
    check_hand(traces.class_history_host(parts))
    # the same parts as merge sources give the same catalogue; a what = 2 part adds no trees
    merged = traces.class_history_host([(source(s, p, w), None, 0, e) for s, p, w, e in parts])
    same(merged, traces.class_history_host(parts))
    only = traces.class_history_host(parts[2:])
    assert only.trees.tolist() == [0, 0] and only.latency_min.tolist() == [MAX] * 2 and only.latency_max.tolist() == [MIN] * 2 and only.counted.tolist() == [1, 1]
    assert only.seen.tolist() == [1, 1] and only.table()[0]["mean_latency"] is None
    # a merged catalogue keeps its epochs and seen; the empty and the long class
    again = traces.class_history_host([(merged, None, 0, 77), (catalogue([NONE, LONG], trees=[4, 2]), None, 0, 1)])
    assert again.first_epoch.tolist() == [2, 5, 2, 1, 1] and again.last_epoch.tolist() == [9, 9, 2, 1, 1] and again.seen.tolist() == [3, 2, 1, 1, 1]
    assert again.class_off.tolist() == [0, 2, 3, 5, 5, 75] and again.class_top_entry.tolist() == [1, 2, 3, -1, -1] and again.signature(3) == ()
    # a mode-0 catalogue holds cg = 0
    flat = traces.class_history_host([(catalogue([((0, 0, 1, 2),)], mode=0, trees=[1]), None, 0, 0)])
    assert flat.mode == 0 and flat.n_classes == 1
    first = (catalogue([A, C]), None, 0, 0)
    for tag, bad in BAD_SOURCES:
        with pytest.raises(ValueError):
            traces.class_history_host([first, (bad(), None, 0, 0)])
    for what in (0, 4):
        with pytest.raises(ValueError):
            traces.class_history_host([parts[0][:2] + (what, 0)])
    off = catalogue([A, C])
    off.class_off = i64([1, 2, 3])
    for bad in ([], [(off, None, 0, 0)]):
        with pytest.raises(ValueError):
            traces.class_history_host(bad)


# ---- 2. by hand through merge -------------------------------------------------------------------------------------------------
EMPTY_INFO = dict(classes=0, entries=0, pushes=0, mode=0, groups=0, capacity=0)


def run_by_hand(lib, slots):
    """The same parts through tw_class_history_merge on an engine that never saw a batch."""
    import ctypes

    eng = Engine(0, lib_path=lib)
    assert eng.class_history_info() == EMPTY_INFO
    parts = hand_parts()
    for (s, p, w, e), ids, summary in zip(parts, HAND_MAPS, HAND_SUMMARIES):
        class_map, got = eng.class_history_merge(source(s, p, w), e)
        assert class_map.tolist() == ids and class_map.dtype == np.int32 and got.tolist() == summary
    h = eng.class_history()
    check_hand(h)
    same(h, traces.class_history_host(parts))
    assert h.n_groups == G
    # the sizes first: a call without outputs
    sizes = np.zeros(6, dtype=np.int64)
    assert eng._lib.tw_class_history_get(eng._h, None, sizes.ctypes.data_as(ctypes.c_void_p)) == 0
    assert sizes.tolist() == [3, 5, 3, 1, G, slots]
    assert eng.class_history_info() == dict(classes=3, entries=5, pushes=3, mode=1, groups=G, capacity=slots)
    # the empty signature, one of 70 entries, and B again, which differs from A in one count
    extra = catalogue([NONE, LONG, B], trees=[4, 2, 1], rows=list(range(70)) + [6, 7], path_rows=[0] * 69 + [1, 0, 0], path_time=[3] * 72)
    class_map, summary = eng.class_history_merge(extra, 1)
    assert class_map.tolist() == [3, 4, 2] and summary.tolist() == [2, 5, 70, 75, 4, 3]
    h = eng.class_history()
    want = traces.class_history_host(parts + [(extra, None, 0, 1)])
    same(h, want)
    assert h.signature(3) == () and h.signature(4) == LONG and h.class_top_entry.tolist() == [1, 2, 3, -1, 74] and h.rows[3:5].tolist() == [1 + 6, 3 + 7]
    assert h.trees.tolist() == [5, 1, 2, 4, 2] and h.seen.tolist() == [3, 2, 2, 1, 1] and h.first_epoch.tolist() == [2, 5, 1, 1, 1]
    # the catalogue read back and merged into an empty one is the catalogue; its epochs and seen are the store's
    other = Engine(0, lib_path=lib)
    class_map, summary = other.class_history_merge(h, 1000)
    assert class_map.tolist() == list(range(5)) and summary.tolist() == [5, 5, 75, 75, 1, 5]
    same(other.class_history(), h)
    other.close()
    t = eng.class_history_timing()
    assert list(t) == ["lookup", "insert", "accumulate"] and all(v >= 0 for v in t.values())
    eng.close()


def test_by_hand(emu_lib):
    run_by_hand(emu_lib, SLOTS_EMU)


@pytest.mark.gpu
def test_by_hand_gpu():
    run_by_hand(None, SLOTS_GPU)


# ---- 3. growth --------------------------------------------------------------------------------------------------------------------
BITS = 12


def generated(ids, n_groups=G):
    """Class i = the entries (level b, 0, b mod G, 1 + bit b of i) over the low BITS bits of i: distinct classes by construction,
    all of one length.  Figures that tell the classes and the entries apart."""
    ids = [int(i) for i in ids]
    sigs = [tuple((b, 0, b % n_groups, 1 + (i >> b & 1)) for b in range(BITS)) for i in ids]
    cell = np.array([i * 100 + b for i in ids for b in range(BITS)], dtype=np.int64)
    return catalogue(sigs, mode=0, n_groups=n_groups, trees=[i + 1 for i in ids], latency_sum=[7 * i for i in ids], latency_min=[i - 5 for i in ids],
                     latency_max=[i + 5 for i in ids], counted=[1] * len(ids), latency=[3 * i for i in ids], rows=cell, span_min=-cell, span_max=cell,
                     path_time=cell % 17, path_rows=cell % 3)


def run_growth(lib, n, slots):
    """Three merges of n generated classes each; consecutive parts share half their classes."""
    assert 2 * n < 1 << BITS
    rng = np.random.RandomState(n)
    eng = Engine(0, lib_path=lib)
    parts, held, caps = [], {}, []
    for p in range(3):
        ids = rng.permutation(np.arange(p * n // 2, p * n // 2 + n))                              # (the source order is not the order of the ids)
        src = generated(ids)
        parts.append((src, None, 0, p))
        before = eng.class_history_info()["classes"]
        class_map, summary = eng.class_history_merge(src, p)
        fresh = [k for k, i in enumerate(ids.tolist()) if i not in held]
        assert len(fresh) == (n if p == 0 else n // 2) and summary.tolist() == [len(fresh), before + len(fresh), BITS * len(fresh),
                                                                                BITS * (before + len(fresh)), p + 1, n]
        assert class_map[fresh].tolist() == list(range(before, before + len(fresh)))               # the new ids in source order
        for k, i in enumerate(ids.tolist()):                                                     # a class held before keeps its id, growth or not
            assert held.setdefault(i, int(class_map[k])) == class_map[k]
        caps.append(eng.class_history_info()["capacity"])
    h = eng.class_history()
    same(h, traces.class_history_host(parts), n)
    assert caps[0] >= 2 * n and caps[-1] >= 4 * n and caps[-1] > caps[0] >= slots and h.n_classes == 2 * n    # the table was refilled
    assert all(h.signature(k) == generated([i]).signature(0) for i, k in list(held.items())[::7])
    assert h.seen.tolist().count(2) == n and h.seen.max() == 2
    eng.close()


def test_growth(emu_lib):
    run_growth(emu_lib, 40, SLOTS_EMU)


@pytest.mark.gpu
def test_growth_gpu():
    run_growth(None, 700, SLOTS_GPU)


# ---- 4. device chain = restatement ----------------------------------------------------------------------------------------------
def check_chain(eng, mode, tag):
    """On a stitched forest with row groups: signatures -> attribute(every tree) -> class_profiles -> push, twice."""
    eng.class_history_reset()
    sig = eng.signatures(mode)
    eng.attribute(**td.EVERY)
    prof = eng.class_profiles()
    class_map, summary = eng.class_history_push(3, 1)
    nc, ne = sig.n_classes, len(sig.class_entries)
    assert class_map.tolist() == list(range(nc)) and summary.tolist() == [nc, nc, ne, ne, 1, nc], tag   # the ids are the batch's class numbers
    h = eng.class_history()
    assert np.array_equal(h.class_off, sig.class_off) and np.array_equal(h.class_entries, sig.class_entries) and h.mode == sig.mode, tag
    for f, want in (("trees", sig.class_trees), ("latency_sum", sig.class_latency_sum), ("latency_min", sig.class_latency_min), ("latency_max", sig.class_latency_max),
                    ("counted", prof.class_counted), ("latency", prof.class_latency), ("class_path_time", prof.class_path_time),
                    ("class_top_entry", prof.class_top_entry)) + tuple((f, getattr(prof, f)) for f in ClassHistory.ENTRY_FIELDS):
        assert np.array_equal(getattr(h, f), want) and getattr(h, f).dtype == want.dtype, (f, tag)
    assert (h.first_epoch == 1).all() and (h.last_epoch == 1).all() and (h.seen == 1).all()
    same(h, traces.class_history_host([(sig, prof, 3, 1)]), tag)
    # the same batch again under another epoch: what adds up doubles, minima and maxima stay, no class is new
    assert np.array_equal(eng.class_history_match(), class_map)
    class_map, summary = eng.class_history_push(3, 7)
    assert class_map.tolist() == list(range(nc)) and summary.tolist() == [0, nc, 0, ne, 2, nc], tag
    twice = eng.class_history()
    for f in ADDITIVE + ("class_path_time",):
        assert np.array_equal(getattr(twice, f), 2 * getattr(h, f)), (f, tag)
    for f in ("class_off", "class_entries", "latency_min", "latency_max", "span_min", "span_max", "class_top_entry", "first_epoch"):
        assert np.array_equal(getattr(twice, f), getattr(h, f)), (f, tag)
    assert (twice.last_epoch == 7).all() and (twice.seen == 2).all()
    same(twice, traces.class_history_host([(sig, prof, 3, 1), (sig, prof, 3, 7)]), tag)
    assert eng.signatures(mode).same_as(sig) and eng.class_profiles().same_as(prof)                # the resident batch is as it was
    return twice


def run_chain(lib, tmp_path, case):
    name, seed, n, concurrency, _ = case
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    group, names = traces.groups_from_table(table)
    eng.set_row_groups(group, len(names))
    eng.stitch()
    got = [check_chain(eng, mode, (name, mode)) for mode in (0, 1)]
    assert got[1].n_classes >= got[0].n_classes >= 1 and got[0].n_groups == len(names)
    eng.close()


def run_chain_on_table(lib, modes=(0, 1)):
    """The same on the sized table of tests/test_signatures.py (no solve): classes of 0 to 600 items, 308 classes."""
    eng, st, link, rows, group, n_groups = tp.table_engine(lib, tg.sized_table())
    for mode in modes:
        assert check_chain(eng, mode, ("sized", mode)).n_classes == len(tg.SIZES) + 1 + tg.N_DISTINCT
    eng.close()


@pytest.mark.parametrize("case", tg.CASES, ids=[c[0] for c in tg.CASES])
def test_device_chain_equals_restatement(emu_lib, tmp_path, case):
    run_chain(emu_lib, tmp_path, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", tg.CASES, ids=[c[0] for c in tg.CASES])
def test_device_chain_equals_restatement_gpu(tmp_path, case):
    run_chain(None, tmp_path, case)


def test_chain_on_the_sized_table(emu_lib):
    run_chain_on_table(emu_lib)


@pytest.mark.gpu
def test_chain_on_the_sized_table_gpu():
    run_chain_on_table(None)


# ---- 5. a partition gives back the whole --------------------------------------------------------------------------------------
def without_seen(by):
    """by_signature() less `seen`, which counts pushes: a class in both halves of a partition was pushed twice."""
    return {s: {k: v for k, v in f.items() if k != "seen"} for s, f in by.items()}


def run_partition(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    group, names = traces.groups_from_table(table)
    eng.set_row_groups(group, len(names))
    st = eng.stitch()
    W, CF = traces.WHOLE, traces.CONFIDENT
    for mode in (0, 1):
        # the signature side: the confident whole traces and the others partition the whole traces
        eng.class_history_reset()
        eng.score_traces(2.0)
        halves = [eng.signatures(mode, W | CF, 0), None]
        eng.class_history_push(1, 3)
        halves[1] = eng.signatures(mode, W, CF)
        eng.class_history_push(1, 3)
        assert 0 < halves[0].n_eligible and 0 < halves[1].n_eligible
        parted = eng.class_history()
        eng.class_history_reset()
        whole = eng.signatures(mode, W, 0)
        assert whole.n_eligible == halves[0].n_eligible + halves[1].n_eligible
        eng.class_history_push(1, 3)
        one = eng.class_history()
        assert without_seen(parted.by_signature()) == without_seen(one.by_signature()), mode
        assert parted.seen.max() == 2 and (one.seen == 1).all() and one.trees.sum() == whole.n_eligible
        # the profile side: the signatures once, then the two attributions of a split at the median tree start, profiles only
        eng.attribute(**td.EVERY)
        full = eng.class_profiles()
        eng.class_history_reset()
        eng.class_history_push(1, 0)
        starts = np.sort(np.asarray(rows[4])[st.tree_root])
        T = int(starts[len(starts) // 2])
        for window in (dict(start_max=T), dict(start_min=T)):
            a = eng.attribute(**dict(td.EVERY, **window))
            assert 0 < a.n_selected < st.n_trees
            eng.class_profiles()
            class_map, summary = eng.class_history_push(2, 0)
            assert class_map.tolist() == list(range(whole.n_classes)) and summary[0] == 0
        h = eng.class_history()
        for f, want in (("counted", full.class_counted), ("latency", full.class_latency), ("class_path_time", full.class_path_time),
                        ("class_top_entry", full.class_top_entry), ("trees", whole.class_trees), ("latency_sum", whole.class_latency_sum),
                        ("latency_min", whole.class_latency_min), ("latency_max", whole.class_latency_max)) + \
                tuple((f, getattr(full, f)) for f in ClassHistory.ENTRY_FIELDS):
            assert np.array_equal(getattr(h, f), want), (f, mode)
        assert (h.seen == 3).all()
    eng.close()


def test_partition_gives_back_the_whole(emu_lib, tmp_path):
    run_partition(emu_lib, tmp_path)


@pytest.mark.gpu
def test_partition_gives_back_the_whole_gpu(tmp_path):
    run_partition(None, tmp_path)


# ---- 6. across loads ----------------------------------------------------------------------------------------------------------
def run_across_loads(lib, tmp_path):
    name, _, n, concurrency, _ = td.CASES[0]
    eng = Engine(0, lib_path=lib)
    parts, order, old_c = [], None, 0
    for k, seed in enumerate((5, 6)):
        corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path / ("load%d" % k), lib, name, seed, n, concurrency)
        rows = traces.rows_from_units(units, table)
        eng.load([u.arrays for u in units])                       # a load, new row maps, passes, a stitch: the catalogue outlives them all
        eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
        eng.run_pass1()
        eng.fit_mixtures(seed=0)
        eng.run_pass2()
        eng.set_span_rows(*rows)
        group, names = traces.groups_from_table(table, corpus)
        if order is None:
            order = names
        else:                                                     # the caller keeps the group numbering stable: the first corpus' order
            assert sorted(names) == sorted(order)
            group = np.array([order.index(x) for x in names], dtype=np.int32)[group]
        eng.set_row_groups(group, len(names))
        eng.stitch()
        sig = eng.signatures(1)
        eng.attribute(**td.EVERY)
        prof = eng.class_profiles()
        parts.append((sig, prof, 3, k))
        match = eng.class_history_match()
        assert match.dtype == np.int32 and len(match) == sig.n_classes and (k > 0 or (match == -1).all())
        class_map, summary = eng.class_history_push(3, k)
        assert np.array_equal(class_map[match >= 0], match[match >= 0])
        fresh = class_map[match < 0]
        assert fresh.tolist() == list(range(old_c, old_c + len(fresh))) and summary[0] == len(fresh) and summary[1] == old_c + len(fresh)
        old_c = int(summary[1])
    assert (match >= 0).any() and eng.class_history_match().min() >= 0
    want = traces.class_history_host(parts)
    before, info = eng.class_history(), eng.class_history_info()
    same(before, want)
    assert before.seen.max() == 2 and info["pushes"] == 2

    def intact(event):
        assert eng.class_history_info() == info, event
        same(eng.class_history(), before, event)

    # whatever drops the batch's stages leaves the catalogue alone (the events of test_stitch.run_residency)
    for event in ("score_traces", "set_row_cohorts", "set_row_groups", "stitch", "set_span_rows", "scale_load", "run_pass1", "load"):
        if event == "score_traces":
            eng.score_traces(0.0)
        elif event == "set_row_cohorts":
            eng.set_row_cohorts((np.asarray(table["trace"]) % 2).astype(np.int32), 2)
        elif event == "set_row_groups":
            eng.set_row_groups(np.where(group >= 0, 0, -1).astype(np.int32), 1)
        elif event == "stitch":
            eng.stitch()
        elif event == "set_span_rows":
            eng.set_span_rows(*rows)
        elif event == "run_pass1":
            eng.run_pass1()
        elif event == "scale_load":
            eng.scale_load([2] * len(units))
        else:
            eng.load([u.arrays for u in units])
        intact(event)
        if event != "set_row_cohorts":                            # ... while the signature result it would be fed from is gone
            error(-4, eng.class_history_match)
    eng.close()


def test_across_loads(emu_lib, tmp_path):
    run_across_loads(emu_lib, tmp_path)


@pytest.mark.gpu
def test_across_loads_gpu(tmp_path):
    run_across_loads(None, tmp_path)


# ---- 7. two hash bits -----------------------------------------------------------------------------------------------------------
def test_two_hash_bits(emu_lib, tmp_path, monkeypatch):
    """TW_SIG_HASH_BITS=2: every class in one of four buckets; the exact comparison alone separates them, the results are the same."""
    monkeypatch.setenv("TW_SIG_HASH_BITS", "2")
    run_growth(emu_lib, 40, SLOTS_EMU)
    run_chain(emu_lib, tmp_path, tg.CASES[1])


@pytest.mark.gpu
def test_two_hash_bits_gpu(tmp_path, monkeypatch):
    monkeypatch.setenv("TW_SIG_HASH_BITS", "2")
    run_growth(None, 700, SLOTS_GPU)
    run_chain(None, tmp_path, tg.CASES[1])


# ---- 8. refusals leave the catalogue alone ----------------------------------------------------------------------------------
def run_refusals(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table)
    eng = ts.solve(lib, units, n_traces)
    error(-4, eng.class_history)                                  # get on an empty catalogue
    error(-4, eng.class_history_push)                             # no signature result: before the rows, before a stitch, before signatures()
    error(-4, eng.class_history_match)
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, len(names))
    eng.stitch()
    error(-4, eng.class_history_push, 1)
    sig = eng.signatures(1)
    for what in (0, 4, -1):
        error(-1, eng.class_history_push, what)
    error(-4, eng.class_history_push, 2)                          # what & 2 without a class profile
    assert eng.class_history_info() == EMPTY_INFO and (eng.class_history_match() == -1).all()
    class_map, summary = eng.class_history_push()                 # the default falls back to the signature result alone
    assert summary[0] == sig.n_classes and eng.class_history().counted.sum() == 0
    eng.attribute(**td.EVERY)
    prof = eng.class_profiles()
    eng.class_history_push(2, 4)
    before, info = eng.class_history(), eng.class_history_info()
    same(before, traces.class_history_host([(sig, None, 1, 0), (sig, prof, 2, 4)]))
    n_groups = len(names)

    def intact(tag):
        assert eng.class_history_info() == info, tag
        assert eng.class_history().same_as(before), tag

    held = before.signature(int(np.argmax(np.diff(before.class_off))))
    assert len(held) >= 2
    bad = [(t, f) for t, f in BAD_SOURCES if t not in ("g >= G", "cg >= G", "another n_groups")] + [
        ("g = G", lambda: catalogue([((0, -1, n_groups, 1),)], n_groups=n_groups)),
        ("cg = G", lambda: catalogue([((1, n_groups, 0, 1),)], n_groups=n_groups)),
        ("one group more", lambda: catalogue([C], n_groups=n_groups + 1)),
        ("a class the catalogue holds, twice", lambda: catalogue([held, C, held], n_groups=n_groups)),
        ("a new class twice, behind one the catalogue holds", lambda: catalogue([held, LONG, C, LONG], n_groups=n_groups))]
    assert n_groups >= G
    for tag, make in bad:
        src = make()
        if tag in dict(BAD_SOURCES):                              # (the sources of part 1, over this catalogue's groups)
            src.n_groups = n_groups
        error(-1, eng.class_history_merge, src)
        intact(tag)
    for off in ([1, 2], [0, 2, 1], [0, 1]):                       # class_off: does not start at 0, decreases, does not end at the entries
        src = catalogue([C, C][:len(off) - 1] if off != [0, 2, 1] else [A, NONE], n_groups=n_groups)
        src.class_off = i64(off)
        if off == [0, 1]:
            src.class_entries = np.array(A, dtype=np.int32)
        error(-1, eng.class_history_merge, src)
        intact(off)
    with pytest.raises(ValueError):
        eng.class_history_merge(catalogue([C], n_groups=n_groups, trees=[1, 2]))
    eng.set_row_groups(np.where(group >= 0, 0, -1).astype(np.int32), 1)                                   # a batch over other groups, of the other mode
    eng.stitch()
    eng.signatures(1)
    error(-1, eng.class_history_push, 1)
    eng.set_row_groups(group, n_groups)
    eng.stitch()
    eng.signatures(0)
    error(-1, eng.class_history_push, 1)
    intact("push")
    # a merge that is accepted after all of them: the catalogue still takes what fits
    class_map, summary = eng.class_history_merge(catalogue([LONG, held], n_groups=n_groups, trees=[1, 1]), 9)
    assert class_map.tolist() == [info["classes"], int(np.argmax(np.diff(before.class_off)))] and summary[0] == 1
    eng.class_history_reset()
    assert eng.class_history_info() == EMPTY_INFO
    error(-4, eng.class_history)
    eng.class_history_push(1)                                     # the mode is open again
    assert eng.class_history_info()["mode"] == 0 and eng.class_history_info()["groups"] == n_groups
    eng.close()


def test_refusals_leave_the_catalogue_alone(emu_lib, tmp_path):
    run_refusals(emu_lib, tmp_path)


@pytest.mark.gpu
def test_refusals_leave_the_catalogue_alone_gpu(tmp_path):
    run_refusals(None, tmp_path)   # (every source is refused by the check kernel or by the comparison: nothing out of range is indexed with)


# ---- 9. one host thread per lane ------------------------------------------------------------------------------------------------
def test_lane_threaded(emu_lib):
    """One host thread per lane (TW_EMU_LANES=1, workgroups of 256): the rounds per distinct class, the lock-step probes and the
    ballots of k_chist_lookup run as they are written, 64 lanes to a wavefront, and the lanes of k_chist_insert claim their slots
    by compare-and-swap beside one another, without a GPU.  (Growth, and the chain on the sized table in mode 1.)"""
    call = "import test_class_history as c\nc.run_growth(%r, 40, c.SLOTS_EMU)\nc.run_chain_on_table(%r, (1,))\nc.run_by_hand(%r, c.SLOTS_EMU)" % ((emu_lib,) * 3)
    tg.in_subprocess(call, dict(TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256"))


# ---- 10. files and the command line -------------------------------------------------------------------------------------------
def test_npz_round_trip(emu_lib, tmp_path):
    eng = Engine(0, lib_path=emu_lib)
    for s, p, w, e in hand_parts():
        eng.class_history_merge(source(s, p, w), e)
    h = eng.class_history()
    path = str(tmp_path / "classes.npz")
    traces.write_class_history_npz(path, h, NAMES)
    back, names = traces.read_class_history_npz(path)
    assert names == NAMES and back.same_as(h) and back.n_groups == G
    eng.class_history_reset()
    eng.class_history_merge(back)
    assert eng.class_history().same_as(h)
    eng.close()
    with pytest.raises(ValueError):
        traces.write_class_history_npz(path, h, NAMES[:2])


def test_cli_class_history(emu_lib, tmp_path, capsys):
    from traceweaver_amd import executor

    synth.write_jaeger_corpus(str(tmp_path / "corpus"), 11, 400, app=synth.HOTEL_APP, concurrency=2.5)
    store = str(tmp_path / "classes.npz")

    def run(tag, extra):
        out = str(tmp_path / tag) + "/"
        executor.main(["--absolute_path", str(tmp_path / "corpus"), "--cache_rate", "0", "--fix", "2", "--results_directory", out,
                       "--test_name", "gen", "--load_level", "7", "--engine_library", emu_lib] + extra)
        return {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}, capsys.readouterr().out

    prof = ["--profiles_out", str(tmp_path / "p.npz"), "--query_percentile", "0.5"]
    plain = run("plain", prof)
    first = run("first", prof + ["--class_history", store, "--class_history_epoch", "3"])
    one, names = traces.read_class_history_npz(store)
    z = np.load(str(tmp_path / "p.npz"))
    assert np.array_equal(one.class_entries, z["class_entries"]) and np.array_equal(one.counted, z["class_counted"]) and np.array_equal(one.rows, z["rows"])
    assert names == z["group_names"].tolist() and (one.first_epoch == 3).all() and (one.seen == 1).all() and one.mode == 0
    line = "Class history: %d call graphs in this run, %d of them new; %d held over %d traces"
    assert line % (one.n_classes, one.n_classes, one.n_classes, one.trees.sum()) in first[1]
    second = run("second", prof + ["--class_history", store, "--class_history_epoch", "5"])
    two, _ = traces.read_class_history_npz(store)
    assert line % (one.n_classes, 0, one.n_classes, 2 * one.trees.sum()) in second[1]
    assert np.array_equal(two.trees, 2 * one.trees) and np.array_equal(two.rows, 2 * one.rows) and np.array_equal(two.class_entries, one.class_entries)
    assert (two.first_epoch == 3).all() and (two.last_epoch == 5).all() and (two.seen == 2).all()
    assert plain[0] == first[0] == second[0] and len(plain[0]) == 5 and "Class history" not in plain[1]   # the five pickles, byte for byte
    # beside --signatures_out alone the classes are kept without profiles, in a store of their own mode
    edges = str(tmp_path / "edges.npz")
    run("sig", ["--signatures_out", str(tmp_path / "s.npz"), "--signature_mode", "edges", "--class_history", edges])
    e, _ = traces.read_class_history_npz(edges)
    assert e.mode == 1 and e.counted.sum() == 0 and e.trees.sum() == one.trees.sum()
    with pytest.raises(SystemExit) as ex:                          # a store of the other signature mode
        run("mode", prof + ["--class_history", edges])
    assert "edges signatures" in str(ex.value)
    foreign = ClassHistory(*[getattr(one, k) for k in ClassHistory.FIELDS], mode=0, n_groups=one.n_groups)
    traces.write_class_history_npz(str(tmp_path / "foreign.npz"), foreign, ["nobody%d" % g for g in range(one.n_groups)])
    with pytest.raises(SystemExit) as ex:                          # a store of other services
        run("other", prof + ["--class_history", str(tmp_path / "foreign.npz")])
    assert "nobody0" in str(ex.value) and "the store holds the services" in str(ex.value)
    base = ["--absolute_path", "x", "--fix", "2", "--results_directory", str(tmp_path) + "/", "--engine_library", emu_lib]
    for extra in (["--class_history", "c.npz"], ["--profiles_out", "p.npz", "--class_history_epoch", "2"],
                  ["--profiles_out", "p.npz", "--class_history", "c.npz", "--cache_rate", "0.5"]):            # the refusals of --stitch_out
        with pytest.raises(SystemExit):
            executor.main(base + extra)
