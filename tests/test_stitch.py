"""Engine.stitch (tw_stitch_traces, csrc/tw_stitch.h): the per-service parent arrays joined with the observed hops of
the span table into whole traces.  Inputs are generated (synth.write_jaeger_corpus / write_alibaba_corpus), ingested with
ingest.open_directory, all units loaded as one batch, both passes run.  Everything is integer: device against the numpy
restatement traces.stitch_host with np.array_equal.  CPU tier: host-emulation build (tiny LDS capacity, so that the
packed, the single-tree and the global-memory route of k_stitch_group all occur); the HIP library under -m gpu."""
import os
import pickle

import numpy as np
import pytest

from traceweaver_amd import synth, traces
from traceweaver_amd.engine import Engine, EngineError

JAEGER = {"hotel": synth.HOTEL_APP, "media": synth.MEDIA_APP, "fanout": synth.FANOUT_APP}
CORPORA = ("hotel", "media", "fanout", "alibaba")


def make_corpus(tmp_path, lib, name, seed=5, n=300, concurrency=1.5):
    from traceweaver_amd.ingest import open_directory

    d = str(tmp_path / ("corpus_" + name))
    if name == "alibaba":
        synth.write_alibaba_corpus(d, seed, n, concurrency=concurrency)
        kw = dict(first_span=None, fix="rpc_twins")
    else:
        synth.write_jaeger_corpus(d, seed, n, app=JAEGER[name], concurrency=concurrency)
        kw = dict(first_span=JAEGER[name]["root_op"], fix=None)
    corpus, _ = open_directory(d, lib_path=lib, max_traces=0, cache=False, **kw)
    units, skipped, n_traces = corpus.units()
    return corpus, units, skipped, n_traces, corpus.span_table()


def solve(lib, units, n_traces, rows=None):
    eng = Engine(0, lib_path=lib)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    eng.run_pass1()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    if rows is not None:
        eng.set_span_rows(*rows)
    return eng


def assert_same(got, want):
    for k in traces.StitchedTraces.FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), k


def trace_roots(table, n_traces):
    """Row of the root span of every trace of the table."""
    r = np.flatnonzero(table["parent"] < 0)
    out = np.full(n_traces, -1, dtype=np.int64)
    out[table["trace"][r]] = r
    assert len(r) == n_traces and (out >= 0).all()
    return out


def check_truth_is_the_corpus(eng, table, n_traces):
    st = eng.stitch(truth=True)
    roots = trace_roots(table, n_traces)
    assert st.n_trees == n_traces and np.array_equal(st.tree_root, np.sort(roots))
    assert np.array_equal(st.root, roots[table["trace"]])
    assert np.all(st.tree_flags == (traces.WHOLE | traces.EXACT))
    assert st.counts.tolist() == [n_traces, 0, 0, n_traces]
    assert np.array_equal(np.diff(st.tree_off), np.bincount(table["trace"], minlength=n_traces)[table["trace"][st.tree_root]])
    end = table["start"] + table["duration"]
    for k in (0, st.n_trees // 2, st.n_trees - 1):
        t = st.trace(k)
        assert t["whole"] and t["exact"] and list(t["rows"]) == sorted(t["rows"], key=lambda r: (table["start"][r], r))
        assert t["latency"] == end[t["rows"]].max() - table["start"][t["root"]]
    return st


def check_against_host(eng, units, rows, pass_=None, truth=True):
    which = 2 if pass_ is None else pass_
    par = [r["parent"] for r in eng.results(which, fields=("parent",))]
    st = eng.stitch(pass_)
    host = traces.stitch_host([u.arrays for u in units], par, *rows, truth=[u.true_parent for u in units] if truth else None)
    assert_same(st, host)
    return st, par


# ---- 1. the true assignment stitches to the corpus --------------------------------------------------------------------
def run_truth(lib, tmp_path, name):
    corpus, units, skipped, n_traces, table = make_corpus(tmp_path, lib, name)
    assert not any(skipped.values()), skipped
    rows = traces.rows_from_units(units, table)
    eng = Engine(0, lib_path=lib)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    eng.set_span_rows(*rows)
    st = check_truth_is_the_corpus(eng, table, n_traces)
    assert_same(st, traces.stitch_host([u.arrays for u in units], [u.true_parent for u in units], *rows, truth=[u.true_parent for u in units]))
    eng.close()


@pytest.mark.parametrize("name", CORPORA)
def test_truth_stitches_to_the_corpus(emu_lib, tmp_path, name):
    run_truth(emu_lib, tmp_path, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CORPORA)
def test_truth_stitches_to_the_corpus_gpu(tmp_path, name):
    run_truth(None, tmp_path, name)


# ---- 2. / 3. device = host restatement; agreement with tw_evaluate -----------------------------------------------------
# (name, seed, traces, concurrency): picked on the host build so that some hold wrong assignments and some requests that
# the selection leaves unassigned -- asserted below
CASES = [("hotel", 5, 300, 1.2, "clean"), ("media", 7, 300, 6.0, "wrong"), ("alibaba", 3, 400, 12.0, "wrong"), ("fanout", 9, 300, 25.0, "unassigned"),
         ("hotel", 4, 300, 40.0, "unassigned")]


def run_case(lib, tmp_path, name, seed, n, concurrency, expect):
    corpus, units, skipped, n_traces, table = make_corpus(tmp_path, lib, name, seed, n, concurrency)
    assert not any(skipped.values()), skipped
    rows = traces.rows_from_units(units, table)
    eng = solve(lib, units, n_traces, rows)
    st, par = check_against_host(eng, units, rows)
    wrong = sum(int((p != u.true_parent).any(axis=0).sum()) for p, u in zip(par, units))
    unassigned = sum(int((p == -1).any(axis=0).sum()) for p in par)
    print("%s: %d requests wrong, %d with an unassigned endpoint; counts %s" % (name, wrong, unassigned, st.counts.tolist()))
    if expect == "wrong":
        assert wrong > 0
    if expect == "unassigned":
        assert unassigned > 0 and st.counts[2] > 0 and st.counts[1] > 0   # a call no request took roots a fragment
    # 3. the figures tw_evaluate reduces from the same arrays
    _, e2e, flags = eng.evaluate(trace_flags=True)
    assert st.counts[3] == e2e[0]
    k = np.searchsorted(st.tree_root, trace_roots(table, n_traces))
    assert np.array_equal((st.tree_flags[k] & traces.EXACT) // traces.EXACT, 1 - flags[0])
    assert st.counts[0] == n_traces and st.counts[0] + st.counts[1] == st.n_trees
    # pass 1 is no longer resident; the last pass is what stitch() names
    with pytest.raises(EngineError) as ex:
        eng.stitch(1)
    assert ex.value.code == -4
    check_truth_is_the_corpus(eng, table, n_traces)
    eng.close()


@pytest.mark.parametrize("name,seed,n,concurrency,expect", CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in CASES])
def test_device_equals_host_restatement(emu_lib, tmp_path, name, seed, n, concurrency, expect):
    run_case(emu_lib, tmp_path, name, seed, n, concurrency, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,n,concurrency,expect", CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in CASES])
def test_device_equals_host_restatement_gpu(tmp_path, name, seed, n, concurrency, expect):
    run_case(None, tmp_path, name, seed, n, concurrency, expect)


def run_left_out(lib, tmp_path):
    """A service that is not in the batch: its calls are holes, the spans below them come back as fragments."""
    corpus, units, skipped, n_traces, table = make_corpus(tmp_path, lib, "hotel", 5, 300, 2.0)
    gone = [u for u in units if u.service == "search"][0]
    units = [u for u in units if u.service != "search"]
    rows = traces.rows_from_units(units, table)
    eng = solve(lib, units, n_traces, rows)
    st, par = check_against_host(eng, units, rows)
    frag = st.tree_root[(st.tree_flags & traces.WHOLE) == 0]
    untaken = [np.setdiff1d(u.out_rows[e], u.out_rows[e][p[e][p[e] >= 0]]) for u, p in zip(units, par) for e in range(u.arrays.E)]
    want = np.sort(np.concatenate(list(gone.out_rows) + untaken))
    assert np.array_equal(frag, want) and len(frag) >= 2 * 300
    assert st.counts[0] == n_traces
    _, e2e = eng.evaluate()
    assert st.counts[3] == e2e[0]   # the reduction counts a service that was left out as right, and so does bit 2
    truth = eng.stitch(truth=True)
    assert truth.counts.tolist() == [n_traces, 2 * 300, 0, n_traces]
    eng.close()


def test_a_left_out_service_leaves_fragments(emu_lib, tmp_path):
    run_left_out(emu_lib, tmp_path)


@pytest.mark.gpu
def test_a_left_out_service_leaves_fragments_gpu(tmp_path):
    run_left_out(None, tmp_path)


# ---- 4. holes stay holes: a skip-mode batch ----------------------------------------------------------------------------
def run_skip(lib, tmp_path):
    from traceweaver_amd import skipmode
    from traceweaver_amd.ingest import IngestedUnit

    corpus, units, skipped, n_traces, table = make_corpus(tmp_path, lib, "hotel", 11, 400, 1.5)
    u = [x for x in units if x.service == "frontend"][0]
    arr, truth, kept = skipmode.cache_hits(u.arrays, u.true_parent, 0.2, in_trace=u.in_trace)   # as executor.py does
    unit = IngestedUnit(arr, truth, u.in_trace, u.service, u.in_ep, u.out_eps, u.in_rows,
                        [r[kept] if e == 0 else r for e, r in enumerate(u.out_rows)], u.process_id)
    deleted = u.out_rows[0][~kept]
    assert len(deleted) == int(0.2 * 400)
    eng = Engine(0, lib_path=lib)
    plan = skipmode.plan(eng, arr)
    eng.load([arr], skip=[plan])
    eng.set_truth([truth], [unit.in_trace], n_traces)
    eng.run_pass1()
    rows = traces.rows_from_units([unit], table, deleted=deleted)
    eng.set_span_rows(*rows)
    par = eng.results(1, fields=("parent",))[0]["parent"]
    st = eng.stitch()
    assert_same(st, traces.stitch_host([arr], [par], *rows, truth=[truth]))
    skipping = np.flatnonzero(par[0] == -2)
    assert len(skipping) > 0
    first = set(u.out_rows[0].tolist())                           # every row of the first endpoint, deleted ones included
    for i in skipping:                                            # a skip span is a missing link: no call of that endpoint in the tree
        k = int(np.searchsorted(st.tree_root, unit.in_rows[i]))
        assert st.tree_root[k] == unit.in_rows[i] and not first & set(st.trace(k)["rows"].tolist())
    taking = np.flatnonzero(par[0] >= 0)
    call = unit.out_rows[0][par[0][taking]]
    assert np.array_equal(st.root[call], st.root[unit.in_rows[taking]]) and np.array_equal(st.depth[call], st.depth[unit.in_rows[taking]] + 1)
    k = np.searchsorted(st.tree_root, np.sort(deleted))           # the deleted calls: absent, a tree of one row each
    assert np.array_equal(st.tree_root[k], np.sort(deleted)) and np.all(np.diff(st.tree_off)[k] == 1)
    assert np.all(st.depth[table["parent"] >= 0][np.isin(table["parent"][table["parent"] >= 0], deleted)] == 0)
    eng.close()


def test_skip_spans_stay_holes(emu_lib, tmp_path):
    run_skip(emu_lib, tmp_path)


@pytest.mark.gpu
def test_skip_spans_stay_holes_gpu(tmp_path):
    run_skip(None, tmp_path)


# ---- 5. load scaling ---------------------------------------------------------------------------------------------------
def run_scaled(lib, tmp_path):
    from traceweaver_amd import transforms

    corpus, units, skipped, n_traces, table = make_corpus(tmp_path, lib, "hotel", 5, 300, 1.5)
    factors = [3, 2]
    assert len(units) == len(factors)
    eng = Engine(0, lib_path=lib)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    eng.set_span_rows(*traces.rows_from_units(units, table))
    perms = eng.scale_load(factors)
    with pytest.raises(EngineError) as ex:                        # the lists were re-sorted: the row maps are dropped
        eng.stitch(truth=True)
    assert ex.value.code == -4
    host = [transforms.compress_unit(u.arrays, u.true_parent, f) for u, f in zip(units, factors)]
    rows = list(traces.rows_from_units(units, table))
    rows[0] = [u.in_rows[ip] for u, (ip, _, _) in zip(units, perms)]
    rows[1] = [[r[p] for r, p in zip(u.out_rows, ops)] for u, (_, ops, _) in zip(units, perms)]
    eng.set_span_rows(*rows)
    eng.run_pass1()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    par = [r["parent"] for r in eng.results(2, fields=("parent",))]
    assert_same(eng.stitch(), traces.stitch_host([s.arrays for s in host], par, *rows, truth=[s.true_parent for s in host]))
    check_truth_is_the_corpus(eng, table, n_traces)
    eng.close()


def test_after_load_scaling(emu_lib, tmp_path):
    run_scaled(emu_lib, tmp_path)


@pytest.mark.gpu
def test_after_load_scaling_gpu(tmp_path):
    run_scaled(None, tmp_path)


# ---- an assignment handed over by the caller (services solved one after the other, gathered from other ranks) --------------
def run_given(lib, tmp_path):
    corpus, units, skipped, n_traces, table = make_corpus(tmp_path, lib, "media", 7, 300, 6.0)
    rows = traces.rows_from_units(units, table)
    eng = solve(lib, units, n_traces, rows)
    st, par = check_against_host(eng, units, rows)
    other = Engine(0, lib_path=lib)
    other.load([u.arrays for u in units])
    other.set_span_rows(*rows)
    with pytest.raises(EngineError) as ex:
        other.stitch(0)
    assert ex.value.code == -4
    other.set_parents(par)
    got = other.stitch(0)
    want = traces.stitch_host([u.arrays for u in units], par, *rows)
    assert_same(got, want)
    assert got.counts[3] == -1 and np.array_equal(got.tree_flags, st.tree_flags & ~np.uint8(traces.EXACT)) and np.array_equal(got.tree_rows, st.tree_rows)
    twice = [p.copy() for p in par]
    twice[0][0, 1] = twice[0][0, 0] = 0
    with pytest.raises(EngineError) as ex:
        other.set_parents(twice)                                  # a call given to two requests
    assert ex.value.code == -1
    eng.close()
    other.close()


def test_parents_handed_over_by_the_caller(emu_lib, tmp_path):
    run_given(emu_lib, tmp_path)


@pytest.mark.gpu
def test_parents_handed_over_by_the_caller_gpu(tmp_path):
    run_given(None, tmp_path)


# ---- 6. state and argument errors --------------------------------------------------------------------------------------
def test_state_errors(emu_lib, tmp_path):
    corpus, units, skipped, n_traces, table = make_corpus(tmp_path, emu_lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    eng = Engine(0, lib_path=emu_lib)
    eng.load([u.arrays for u in units])

    def state_error(*a, **kw):
        with pytest.raises(EngineError) as ex:
            eng.stitch(*a, **kw)
        assert ex.value.code == -4 and "TW_ERR_STATE" in str(ex.value)

    state_error()                                                 # before set_span_rows
    eng.set_span_rows(*rows)
    state_error()                                                 # before a pass
    state_error(truth=True)                                       # before set_truth
    eng.run_pass1()
    assert eng.stitch().n_trees >= n_traces
    state_error(2)
    eng.load([u.arrays for u in units])                           # a load drops the rows
    eng.run_pass1()
    state_error()
    eng.close()


# ---- 6b. residency: what every event drops of the stages that follow the stitch ----------------------------------------------
# Consumers in the order they are probed after an event: a refused call changes nothing, and no call restores what a later one
# needs (the distributions need the attribution, so they go first; the attribution goes last).
CONSUMERS = ("distributions", "compare", "signatures", "score", "attribute")
EVERY = frozenset(CONSUMERS)
# event -> the consumers that refuse with TW_ERR_STATE afterwards; every other one answers what it answered before the event.
# Taken from the engine as it was before the flags had one owner (tw_engine.hip, "residency of the trace stages").
RESIDENCY = {
    "stitch": {"distributions"},                                  # a new forest: the attribution goes, the reference set stays
    "set_row_groups": {"distributions", "compare"},               # ... the attribution and the reference set go
    "set_row_cohorts": set(),                                     # only the sorted items, which the next call builds again
    "score_traces": set(),                                        # only a resident signature result, see below
    "set_span_rows": EVERY, "run_pass1": EVERY, "load": EVERY, "scale_load": EVERY,
}


def run_residency(lib, tmp_path):
    corpus, units, skipped, n_traces, table = make_corpus(tmp_path, lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    group, names = traces.groups_from_table(table)
    cohort = (np.asarray(table["trace"]) % 2).astype(np.int32)
    W, C = traces.WHOLE, traces.CONFIDENT
    eng = solve(lib, units, n_traces)
    calls = {"distributions": lambda: eng.distributions((0.5, 0.9), (1000, 5000)), "compare": lambda: eng.signatures(compare=True),
             "signatures": lambda: eng.signatures(), "score": lambda: eng.score_traces(0.0), "attribute": lambda: eng.attribute()}

    def resident():
        """Everything set and every stage run: what the consumers answer now."""
        eng.set_span_rows(*rows)
        eng.set_row_groups(group, len(names))
        eng.set_row_cohorts(cohort, 2)
        st = eng.stitch()
        eng.signatures(keep_reference=True)
        before = {k: calls[k]() for k in reversed(CONSUMERS)}
        assert before["compare"].summary[4] > 0 and before["distributions"].summary[0] > 0 and before["attribute"].n_selected > 0
        return st, before

    def probe(before):
        refused = set()
        for k in CONSUMERS:
            try:
                got = calls[k]()
            except EngineError as ex:
                assert ex.code == -4 and "TW_ERR_STATE" in str(ex), (k, str(ex))
                refused.add(k)
            else:
                assert got.same_as(before[k]), k
        return refused

    seen = {}
    for event in ("stitch", "set_row_groups", "set_row_cohorts", "score_traces", "set_span_rows", "run_pass1", "load", "scale_load"):
        st, before = resident()
        if event == "stitch":
            eng.stitch()
        elif event == "set_row_groups":
            eng.set_row_groups(group, len(names))
        elif event == "set_row_cohorts":
            eng.set_row_cohorts(cohort, 2)
        elif event == "score_traces":
            # the same query before and after: the call after must compute again, on the CONFIDENT bits of the new threshold
            sure = eng.signatures(need_flags=W | C)
            conf = eng.score_traces(2.0)
            want = int(((st.tree_flags & W) != 0).astype(np.int64) @ conf.tree_confident.astype(np.int64))
            again = eng.signatures(need_flags=W | C)
            print("signatures(WHOLE | CONFIDENT): %d eligible at threshold 0, %d at 2" % (sure.n_eligible, again.n_eligible))
            assert 0 < again.n_eligible == want < sure.n_eligible
        elif event == "set_span_rows":
            eng.set_span_rows(*rows)
        elif event == "run_pass1":
            eng.run_pass1()
        elif event == "load":
            eng.load([u.arrays for u in units])
        else:
            eng.scale_load([2] * len(units))
        seen[event] = probe(before)
        if event == "load":                                       # back to a solved batch for the last event
            eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
            eng.run_pass1()
    eng.close()
    assert seen == {k: set(v) for k, v in RESIDENCY.items()}, seen


def test_residency_of_the_trace_stages(emu_lib, tmp_path):
    run_residency(emu_lib, tmp_path)


@pytest.mark.gpu
def test_residency_of_the_trace_stages_gpu(tmp_path):
    run_residency(None, tmp_path)


def test_malformed_links_end_in_a_status(emu_lib, tmp_path):
    """Host build only: malformed input is never sent to a GPU on purpose."""
    import time

    corpus, units, skipped, n_traces, table = make_corpus(tmp_path, emu_lib, "hotel", 5, 200, 1.2)
    eng = Engine(0, lib_path=emu_lib)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units])
    in_rows, out_rows, link, kind, start, end = traces.rows_from_units(units, table)
    servers = np.flatnonzero(kind == 1)
    t0 = time.time()
    bad = link.copy()
    bad[servers[0]], bad[servers[1]] = servers[1], servers[0]     # a two-cycle among server rows
    with pytest.raises(EngineError) as ex:
        eng.set_span_rows(in_rows, out_rows, bad, kind, start, end)
        eng.stitch(truth=True)
    assert ex.value.code == -1
    # a cycle the host checks cannot see: a request's observed caller is a call the truth gives to that very request
    u = units[0]
    bad = link.copy()
    bad[u.in_rows[0]] = u.out_rows[0][u.true_parent[0, 0]]
    eng.set_span_rows(in_rows, out_rows, bad, kind, start, end)
    with pytest.raises(EngineError) as ex:
        eng.stitch(truth=True)
    assert ex.value.code == -1 and "cycle" in str(ex.value) and time.time() - t0 < 30
    # a three-cycle never settles: the doubling loop is capped
    a, b = u.in_rows[0], u.in_rows[1]
    ca, cb = u.out_rows[0][u.true_parent[0, 0]], u.out_rows[0][u.true_parent[0, 1]]
    bad = link.copy()
    bad[a], bad[b] = cb, ca                                       # a -> cb -> b -> ca -> a
    eng.set_span_rows(in_rows, out_rows, bad, kind, start, end)
    with pytest.raises(EngineError) as ex:
        eng.stitch(truth=True)
    assert ex.value.code == -1 and time.time() - t0 < 30
    for col, value in ((2, np.full_like(link, len(link))), (3, np.full_like(kind, 3))):
        args = [in_rows, out_rows, link, kind, start, end]
        args[col] = value
        with pytest.raises(EngineError) as ex:
            eng.set_span_rows(*args)
        assert ex.value.code == -1
    eng.close()


# ---- 7. the command line -----------------------------------------------------------------------------------------------
def test_cli_stitch_out(emu_lib, tmp_path, capsys):
    from traceweaver_amd import executor

    synth.write_jaeger_corpus(str(tmp_path / "corpus"), 11, 400, app=synth.HOTEL_APP, concurrency=2.5)
    runs = {}
    for tag, extra in (("plain", []), ("stitch", ["--stitch_out", str(tmp_path / "traces.npz")])):
        out = str(tmp_path / tag) + "/"
        executor.main(["--absolute_path", str(tmp_path / "corpus"), "--cache_rate", "0", "--fix", "2", "--results_directory", out,
                       "--test_name", "gen", "--load_level", "7", "--engine_library", emu_lib] + extra)
        runs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        text = capsys.readouterr().out
    assert len(runs["plain"]) == 5 and runs["plain"] == runs["stitch"]       # the five pickles, byte for byte
    line = [x for x in text.splitlines() if x.startswith("Stitched traces:")]
    assert len(line) == 1
    z = np.load(str(tmp_path / "traces.npz"))
    c = z["counts"].tolist()
    assert line[0] == "Stitched traces: %d whole, %d fragments, %d with unassigned calls; exact vs ground truth: %d of %d" % (c[0], c[1], c[2], c[3], 400)
    acc = pickle.loads([v for k, v in runs["stitch"].items() if k.startswith("accuracy_")][0])
    assert c[3] == round(acc["MaxScoreBatchSubsetWithSkips"] * 400 / 100)
    assert len(z["row_trace_id"]) == len(z["root"]) == len(z["row_span_id"]) and len(z["tree_off"]) == len(z["tree_root"]) + 1
    whole = z["tree_flags"] & 1
    assert int(whole.sum()) == 400 and set(z["row_trace_id"][z["tree_root"][whole == 1]]) == set(z["row_trace_id"])
    k = int(np.flatnonzero((z["tree_flags"] & 4) != 0)[0])                  # an exact tree holds the spans of one trace
    rows = z["tree_rows"][z["tree_off"][k]:z["tree_off"][k + 1]]
    assert len(set(z["row_trace_id"][rows])) == 1 and len(rows) == 11
