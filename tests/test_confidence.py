"""Engine.decisions / Engine.score_traces (tw_get_decisions, tw_score_traces, csrc/tw_conf.h): the margin of every request's
decision, its reduction over the stitched trees, the calibration table and the CONFIDENT bit of the attribution query.  The
yardsticks are traces.decisions_host and traces.confidence_host, the definitions of include/traceweaver_amd.h restated in
numpy; part 1 checks them on values written out by hand, part 2 the decisions against the independent oracle, the rest
compares the device with the restatement -- np.array_equal on every output, the doubles as the integers they are stored as, so
that NaN and the infinities count.  Corpora and cases are those of tests/test_stitch.py.  CPU tier: host-emulation build; the
HIP library under -m gpu."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import parity
import test_attribute as ta
import test_stitch as ts
from conftest import REPO
from traceweaver_amd import synth, traces
from traceweaver_amd.engine import Engine, EngineError

W, U, X, C = traces.WHOLE, traces.UNASSIGNED, traces.EXACT, traces.CONFIDENT
NAN, INF = float("nan"), float("inf")
EDGES = (0.0, 1.0, 5.0)


def bits(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_same(got, want, fields=traces.TraceConfidence.FIELDS, tag=""):
    for k in fields:
        assert np.array_equal(bits(getattr(got, k)), bits(getattr(want, k))), (k, tag)


# ---- 1. the restatement on values written out by hand -----------------------------------------------------------------------
def test_host_decisions_by_hand():
    r = {"chosen": [0, 0, 2, -1, 1, 0], "topk_n": [1, 3, 3, 0, 2, 2],
         "topk_score": [[-1.0, NAN, NAN], [-1.5, -4.0, -9.0], [-2.0, -2.5, -2.75], [NAN, NAN, NAN], [-INF, -INF, NAN], [3.0, 3.0, NAN]]}
    d = traces.decisions_host(r)
    assert d["rank"].tolist() == [0, 0, 2, -1, 1, 0] and d["list_n"].tolist() == [1, 3, 3, 0, 2, 2]
    want = np.array([INF, 2.5, -0.75, NAN, NAN, 0.0])             # a list of one; best - second; chosen - best; none; inf - inf; a tie
    assert np.array_equal(bits(d["margin"]), bits(want))
    assert int((d["rank"] != 0).sum()) == 3                        # not_best: another tuple than the best one, or none


def hand_forest():
    # trees (by root row): 0 {0, 1, 2}; 3 {3, 4}; 5 {5, 6, 7}; 8 {8} a fragment without a decision; 9 {9, 10, 11}; 12 {12}
    rows = [(0, 90, -1), (10, 50, 0), (20, 40, 1), (100, 190, -1), (110, 150, 3), (200, 290, -1), (210, 250, 5), (220, 240, 6),
            (300, 310, -1), (400, 490, -1), (410, 450, 9), (420, 440, 9), (500, 510, -1)]
    flags = {0: W | X, 3: W, 5: W | U, 8: 0, 9: W | X, 12: W | U}
    st, link, start, end = ta.forest(rows, flags)
    st.counts = np.array([5, 1, 2, 2], dtype=np.int64)
    # requests in an order of their own: the tie of tree 9 is met at row 11 first
    in_rows = [2, 0, 3, 4, 5, 7, 11, 10, 12]
    rank = [0, 0, 0, 2, -1, 0, 0, 0, -1]
    margin = [1.0, 3.0, 2.0, -0.5, NAN, INF, 0.25, 0.25, NAN]
    return st, in_rows, rank, margin


def test_host_trees_by_hand():
    st, in_rows, rank, margin = hand_forest()
    c = traces.confidence_host(st, in_rows, rank, margin, threshold=0.0, edges=(1.0, 3.0))
    assert c.row_request.tolist() == [1, -1, 0, 2, 3, 4, -1, 5, -1, -1, 7, 6, 8]
    assert c.tree_decisions.tolist() == [2, 2, 2, 0, 2, 1]
    assert c.tree_not_best.tolist() == [0, 1, 1, 0, 0, 1]          # an unassigned request is not at its best either
    assert c.tree_unassigned.tolist() == [0, 0, 1, 0, 0, 1]
    assert np.array_equal(bits(c.tree_min_margin), bits(np.array([1.0, -0.5, INF, INF, 0.25, INF])))   # n == 1: +inf; NaN never counts
    assert c.tree_weakest_row.tolist() == [2, 4, 7, -1, 10, -1]    # the tie: the smaller row; a tree of NaN margins only: none
    assert c.tree_confident.tolist() == [1, 0, 0, 0, 1, 0]
    # buckets: 0 not best; 1 below 1.0; 2 [1.0, 3.0) -- a margin exactly on an edge has passed it; 3 from 3.0 on
    assert c.calib.tolist() == [[3, 0, 5], [1, 1, 2], [1, 1, 2], [0, 0, 0]]
    assert c.summary.tolist() == [5, 2, 9, 3, 2]
    c = traces.confidence_host(st, in_rows, rank, margin, threshold=1.0, edges=(0.25, 1.0))
    assert c.tree_confident.tolist() == [1, 0, 0, 0, 0, 0]         # 1.0 >= 1.0
    assert c.calib.tolist() == [[3, 0, 5], [0, 0, 0], [1, 1, 2], [1, 1, 2]]
    st.counts[3] = -1                                              # no ground truth: the exact column says so
    c = traces.confidence_host(st, in_rows, rank, margin)
    assert c.calib.tolist() == [[3, -1, 5], [2, -1, 4]] and c.summary.tolist() == [5, 2, 9, 3, 2]
    assert [r["trees"] for r in c.table()] == [3, 2] and c.table()[1]["from"] == -INF and np.isnan(c.table()[1]["exact_share"])


def test_host_margin_order():
    m = np.array([INF, 1.0, 0.0, -0.0, -1.0, -INF])
    k = traces.margin_key(m)
    assert np.all(k[:-1] > k[1:])                                  # -inf < -1 < -0 < +0 < 1 < +inf


# ---- 2. the decisions against the independent oracle ------------------------------------------------------------------------
ROUTES = [parity.STRESS[k] for k in (3, 6, 7)]                     # picked on the host build: see the assertions below


def run_oracle(lib, cases, routes):
    units, _ = parity.stress_units(cases)
    eng = Engine(0, lib_path=lib)
    eng.load(units)
    eng.run_pass1()
    dec, res = eng.decisions(1), eng.results(1, fields=("unit_stats",))
    with pytest.raises(EngineError) as ex:
        eng.decisions(2)
    assert ex.value.code == -4
    ora = [parity.oracle_two_pass(parity.oracle_service(u)) for u in units]   # (end_flag, pass 1, pass 2, mixtures)
    eng.set_mixtures([o[3][0] for o in ora], [o[3][1] for o in ora])
    eng.run_pass2()
    dec2, res2 = eng.decisions(2), eng.results(2, fields=("unit_stats",))
    eng.close()
    lower = above = again = 0
    for k, u in enumerate(units):
        _, p1, p2, _ = ora[k]
        assert p1["budget_windows"] == 0 and res[k]["budget_windows"] == 0 and p2["budget_windows"] == 0 and res2[k]["budget_windows"] == 0
        want, want2 = traces.decisions_host(p1), traces.decisions_host(p2)
        for f in ("rank", "list_n", "margin"):
            assert np.array_equal(bits(dec[k][f]), bits(want[f])), (cases[k], f)
            assert np.array_equal(bits(dec2[k][f]), bits(want2[f])), (cases[k], f, "pass 2")
        assert int((dec2[k]["rank"] != 0).sum()) == p2["not_best_count"] == res2[k]["not_best_count"]
        assert int((dec[k]["rank"] != 0).sum()) == p1["not_best_count"] == res[k]["not_best_count"]
        assert int((dec[k]["rank"] < 0).sum()) == p1["cnt_unassigned"]
        m = dec[k]["margin"]
        assert np.all(m[dec[k]["rank"] == 0] >= 0) and np.all(m[dec[k]["rank"] > 0] <= 0) and np.isnan(m[dec[k]["rank"] < 0]).all()
        lower += int((dec[k]["rank"] > 0).sum())
        above += int((dec[k]["rank"] < 0).sum())
        again += int(((p1["topk_n"] != p1["topk2_n"]) | (p1["topk_idx"] != p1["topk2_idx"]).any(axis=(1, 2))).sum())
    if routes:   # a request below its best, one without a tuple, one whose list was enumerated again on the remaining spans
        assert lower > 0 and above > 0 and again > 0, (lower, above, again)


def test_decisions_equal_the_oracle(emu_lib, oracle):
    run_oracle(emu_lib, ROUTES, True)
    run_oracle(emu_lib, parity.STRESS, False)


@pytest.mark.gpu
def test_decisions_equal_the_oracle_gpu(oracle):
    run_oracle(None, parity.STRESS, True)


# ---- 3. device = restatement on stitched corpora ----------------------------------------------------------------------------
def check_scores(eng, st, rows, queries=((0.0, EDGES), (2.0, (1.0, 5.0)))):
    dec = eng.decisions()
    out = []
    for threshold, edges in queries:
        got = eng.score_traces(threshold, edges)
        want = traces.confidence_host(st, rows[0], [d["rank"] for d in dec], [d["margin"] for d in dec], threshold, edges, list_n=[d["list_n"] for d in dec])
        assert_same(got, want, tag=(threshold, edges))
        assert got.threshold == threshold and got.edges.tolist() == list(edges)
        out.append(got)
    t = eng.score_timing()
    assert list(t) == ["decisions", "trees", "calibration"] and all(v >= 0 for v in t.values())
    return out


def run_case(lib, tmp_path, name, seed, n, concurrency, expect):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, name, seed, n, concurrency)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    st = eng.stitch()
    flags = st.tree_flags.copy()
    a, b = check_scores(eng, st, rows)
    assert np.array_equal(eng.stitch().tree_flags, flags) and not np.any(flags & C)   # the stitch's own flags never show the bit
    eng.score_traces()
    assert 0 < a.n_confident < a.n_scored and b.n_confident < a.n_confident   # some tree is confident and some is not
    whole = (st.tree_flags & W) != 0
    assert int(a.calib[:, 0].sum()) == int((whole & (a.tree_decisions > 0)).sum()) == int(b.calib[:, 0].sum())
    assert int(a.calib[:, 1].sum()) == int((whole & (a.tree_decisions > 0) & ((st.tree_flags & X) != 0)).sum())   # truth is set
    assert a.summary[2] == sum(u.arrays.n_in for u in units) and a.summary[3] == sum(r["not_best_count"] for r in eng.results(2, fields=("unit_stats",)))
    print("%s: %d of %d scored trees confident; calibration %s" % (name, a.n_confident, a.n_scored, a.calib.tolist()))
    eng.close()


@pytest.mark.parametrize("name,seed,n,concurrency,expect", ts.CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in ts.CASES])
def test_device_equals_host_restatement(emu_lib, tmp_path, name, seed, n, concurrency, expect):
    run_case(emu_lib, tmp_path, name, seed, n, concurrency, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,n,concurrency,expect", ts.CASES, ids=["%s-%g-%s" % (c[0], c[3], c[4]) for c in ts.CASES])
def test_device_equals_host_restatement_gpu(tmp_path, name, seed, n, concurrency, expect):
    run_case(None, tmp_path, name, seed, n, concurrency, expect)


def run_pass1_without_truth(lib, tmp_path):
    """Pass 1 stitched while it is resident (also after the mixtures are set), no ground truth: the exact column is -1."""
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "media", 7, 120, 6.0)
    rows = traces.rows_from_units(units, table)
    eng = Engine(0, lib_path=lib)
    eng.load([u.arrays for u in units])
    eng.run_pass1()
    eng.set_span_rows(*rows)
    st = eng.stitch(1)
    a, _ = check_scores(eng, st, rows)
    assert np.all(a.calib[:, 1] == -1) and a.calib[:, 0].sum() > 0
    eng.fit_mixtures(seed=0)                                      # pass 1 stays resident, and so does its forest
    b = eng.score_traces(0.0, EDGES)
    assert_same(a, b)
    eng.close()


def test_pass1_without_truth(emu_lib, tmp_path):
    run_pass1_without_truth(emu_lib, tmp_path)


@pytest.mark.gpu
def test_pass1_without_truth_gpu(tmp_path):
    run_pass1_without_truth(None, tmp_path)


# ---- 4. the bit in the attribution query ------------------------------------------------------------------------------------
def run_query(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "media", 7, 300, 6.0)
    rows = traces.rows_from_units(units, table)
    eng = ts.solve(lib, units, n_traces, rows)
    group, names = traces.groups_from_table(table)
    eng.set_row_groups(group, len(names))
    st = eng.stitch()
    link = ta.links_of([u.arrays for u in units], [r["parent"] for r in eng.results(2, fields=("parent",))], rows)
    start, end = np.asarray(rows[4]), np.asarray(rows[5])
    plain = eng.attribute()
    before = eng.attribute(need_flags=W | C)
    assert before.n_eligible == 0 and before.n_selected == 0 and before.culprit == -1   # before a scoring call the bit is never set
    last = None
    for threshold in (0.0, 2.0):                                   # the second call replaces the bits of the first
        conf = eng.score_traces(threshold)
        marked = traces.StitchedTraces(st.root, st.depth, st.tree_off, st.tree_rows, st.tree_root, st.tree_latency,
                                       (st.tree_flags | (conf.tree_confident * C)).astype(np.uint8), st.counts)
        for q in (dict(need_flags=W | C), dict(need_flags=W | C, percentile=0.5), dict(need_flags=C, skip_flags=0)):
            got = eng.attribute(**q)
            want = traces.attribute_host(marked, link, start, end, group, len(names), **q)
            for k in traces.Attribution.FIELDS:
                assert np.array_equal(getattr(got, k), getattr(want, k)), (k, q, threshold)
        sure = eng.attribute(need_flags=W | C)
        assert 0 < sure.n_eligible == int(((marked.tree_flags & (W | C | U)) == (W | C)).sum()) < plain.n_eligible
        assert last is None or sure.n_eligible < last
        last = sure.n_eligible
        assert plain.same_as(eng.attribute())                      # today's arguments give today's answers
    eng.stitch()                                                   # a new stitch starts without the bit
    assert eng.attribute(need_flags=W | C).n_eligible == 0
    eng.close()


def test_confident_bit_in_the_attribution_query(emu_lib, tmp_path):
    run_query(emu_lib, tmp_path)


@pytest.mark.gpu
def test_confident_bit_in_the_attribution_query_gpu(tmp_path):
    run_query(None, tmp_path)


# ---- 5. state and argument errors -------------------------------------------------------------------------------------------
def run_errors(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 200, 1.2)
    rows = traces.rows_from_units(units, table)
    eng = Engine(0, lib_path=lib)

    def error(code, f, *a, **kw):
        with pytest.raises(EngineError) as ex:
            f(*a, **kw)
        assert ex.value.code == code and {-4: "TW_ERR_STATE", -1: "TW_ERR_ARG"}[code] in str(ex.value)

    def load():
        eng.load([u.arrays for u in units])
        eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)

    load()
    eng._n_trees = 0
    error(-4, eng.decisions, 1)                                    # before the pass
    error(-4, eng.score_traces)                                    # before the row maps
    eng.set_span_rows(*rows)
    error(-4, eng.score_traces)                                    # before a stitch
    eng.stitch(truth=True)
    error(-4, eng.score_traces)                                    # the true forest holds no decisions
    eng.run_pass1()
    assert len(eng.decisions(1)) == len(units) and len(eng.decisions()) == len(units)
    error(-4, eng.decisions, 2)
    error(-4, eng.score_traces)                                    # a new pass dropped the forest
    par = [r["parent"] for r in eng.results(1, fields=("parent",))]
    eng.set_parents(par)
    eng.stitch(0)
    error(-4, eng.score_traces)                                    # nor does a forest of parent arrays handed over
    eng.stitch(1)
    good = eng.score_traces(0.0, EDGES)
    for bad in ((1.0, 0.0), (0.0, 0.0), (0.0, NAN), (NAN,), tuple(float(x) for x in range(16))):
        error(-1, eng.score_traces, 0.0, bad)
    assert_same(eng.score_traces(0.0, EDGES), good)                # a refused call changes nothing
    assert eng.score_traces(0.0, tuple(float(x) for x in range(15))).calib.shape == (17, 3)
    assert eng.score_traces(NAN).n_confident == 0 and eng.score_traces(-INF).n_confident == int((good.tree_not_best[good.tree_decisions > 0] == 0).sum())
    eng.set_span_rows(*rows)                                       # new row maps drop the forest
    error(-4, eng.score_traces)
    eng.stitch(1)
    eng.score_traces()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    error(-4, eng.score_traces)
    error(-4, eng.decisions, 1)                                    # pass 1 is no longer resident
    eng.stitch()
    eng.score_traces()
    eng.stitch(truth=True)
    error(-4, eng.score_traces)
    load()                                                         # a load drops everything
    error(-4, eng.score_traces)
    error(-4, eng.decisions)
    eng.close()


def test_state_and_argument_errors(emu_lib, tmp_path):
    run_errors(emu_lib, tmp_path)


@pytest.mark.gpu
def test_state_and_argument_errors_gpu(tmp_path):
    run_errors(None, tmp_path)   # (all refused on the host: nothing malformed reaches the device)


def run_after_load_scaling(lib, tmp_path):
    corpus, units, skipped, n_traces, table = ts.make_corpus(tmp_path, lib, "hotel", 5, 200, 1.5)
    eng = Engine(0, lib_path=lib)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    rows = list(traces.rows_from_units(units, table))
    eng.set_span_rows(*rows)
    eng.run_pass1()
    eng.stitch()
    eng.score_traces()
    perms = eng.scale_load([3, 2])
    with pytest.raises(EngineError) as ex:                        # the row maps are dropped, the forest with them
        eng.score_traces()
    assert ex.value.code == -4
    rows[0] = [u.in_rows[ip] for u, (ip, _, _) in zip(units, perms)]
    rows[1] = [[r[p] for r, p in zip(u.out_rows, ops)] for u, (_, ops, _) in zip(units, perms)]
    eng.set_span_rows(*rows)
    eng.run_pass1()
    check_scores(eng, eng.stitch(), rows)
    eng.close()


def test_after_load_scaling(emu_lib, tmp_path):
    run_after_load_scaling(emu_lib, tmp_path)


@pytest.mark.gpu
def test_after_load_scaling_gpu(tmp_path):
    run_after_load_scaling(None, tmp_path)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------
def test_cli_confidence_out(emu_lib, tmp_path, capsys):
    from traceweaver_amd import executor
    from traceweaver_amd.ingest import REFERENCE_FIX, open_directory

    synth.write_jaeger_corpus(str(tmp_path / "corpus"), 11, 300, app=synth.HOTEL_APP, concurrency=8.0)
    base = ["--absolute_path", str(tmp_path / "corpus"), "--cache_rate", "0", "--fix", "2", "--test_name", "gen", "--load_level", "7",
            "--engine_library", emu_lib, "--fit", "device-batch", "--seed", "3"]
    files = {k: str(tmp_path / (k + ".npz")) for k in ("traces", "attr", "conf", "attr_all")}
    executor.main(base + ["--results_directory", str(tmp_path / "plain") + "/", "--stitch_out", files["traces"] + ".plain", "--attribute_out", files["attr_all"],
                          "--query_percentile", "0.5"])
    capsys.readouterr()
    executor.main(base + ["--results_directory", str(tmp_path / "conf") + "/", "--stitch_out", files["traces"], "--attribute_out", files["attr"],
                          "--query_percentile", "0.5", "--confidence_out", files["conf"], "--min_margin", "0.5", "--query_confident", "1", "-v"])
    text = capsys.readouterr().out
    for f in sorted(os.listdir(str(tmp_path / "plain"))):          # the five pickles, byte for byte
        assert open(str(tmp_path / "plain" / f), "rb").read() == open(str(tmp_path / "conf" / f), "rb").read()
    s, plain = np.load(files["traces"]), np.load(files["traces"] + ".plain")
    assert all(np.array_equal(s[k], plain[k]) for k in s.files)    # the stitch of the resident pass is the stitch of its parent arrays
    # the same batch through the engine
    first_span, fix = REFERENCE_FIX[2]
    corpus, _ = open_directory(str(tmp_path / "corpus"), lib_path=emu_lib, first_span=first_span, fix=fix, max_traces=1001, cache=False)
    units, skipped, n_traces = corpus.units()
    table = corpus.span_table()
    eng = Engine(0, lib_path=emu_lib)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    eng.run_pass1()
    eng.fit_mixtures(seed=3)
    eng.run_pass2()
    eng.set_span_rows(*traces.rows_from_units(units, table))
    st = eng.stitch()
    want = eng.score_traces(0.5, executor.CONFIDENCE_EDGES)
    z = np.load(files["conf"])
    for k in traces.TraceConfidence.FIELDS:
        assert np.array_equal(bits(z[k]), bits(getattr(want, k))), k
    assert float(z["threshold"]) == 0.5 and z["edges"].tolist() == list(executor.CONFIDENCE_EDGES) and np.array_equal(z["tree_root"], st.tree_root)
    assert 0 < want.n_confident < want.n_scored
    line = [x for x in text.splitlines() if x.startswith("Trace confidence:")]
    assert line == ["Trace confidence: %d of %d scored traces confident (margin >= 0.5); %d of %d decisions not best, %d unassigned"
                    % (want.n_confident, want.n_scored, want.summary[3], want.summary[2], want.summary[4])]
    assert len([x for x in text.splitlines() if "whole traces," in x]) == len(executor.CONFIDENCE_EDGES) + 2   # -v: the calibration table
    # --query_confident 1: the culprit query ran on the whole and confident traces only
    group, names = traces.groups_from_table(table, corpus)
    eng.set_row_groups(group, len(names))
    sure, everything = eng.attribute(percentile=0.5, need_flags=W | C), eng.attribute(percentile=0.5)
    a, b = np.load(files["attr"]), np.load(files["attr_all"])
    assert np.array_equal(a["summary"], sure.summary) and np.array_equal(a["groups"], sure.groups) and np.array_equal(a["tree_selected"], sure.tree_selected)
    assert np.array_equal(b["summary"], everything.summary) and np.array_equal(b["groups"], everything.groups)
    assert sure.n_eligible < everything.n_eligible
    assert len([x for x in text.splitlines() if x.startswith("Delay culprit (true traces):")]) == 1
    eng.close()
    corpus.close()
    ref = ["--absolute_path", "x", "--fix", "2", "--results_directory", str(tmp_path) + "/", "--engine_library", emu_lib, "--confidence_out", "c.npz"]
    for extra in (["--cache_rate", "0.1", "--fit", "device-batch"], ["--cache_rate", "0"], ["--cache_rate", "0", "--fit", "device-batch", "--predictor_indices", "3"],
                  ["--cache_rate", "0", "--fit", "device-batch", "--query_confident", "1"], ["--cache_rate", "0", "--fit", "device-batch", "--min_margin", "nan"]):
        with pytest.raises(SystemExit):
            executor.main(ref + extra)
    with pytest.raises(SystemExit):                                # the bit needs a scoring call
        executor.main(ref[:-2] + ["--cache_rate", "0", "--attribute_out", "a.npz", "--query_confident", "1"])


# ---- 7. the ABI -------------------------------------------------------------------------------------------------------------
NAMES = ("tw_get_decisions", "tw_score_traces")


def test_symbols_in_the_hip_library():
    from traceweaver_amd import _ffi, build

    lib = ctypes.CDLL(build.build())
    for name in NAMES:
        assert hasattr(lib, name) and name in _ffi.EXPORTS


def test_symbols_in_the_emulation_build(emu_lib):
    lib = ctypes.CDLL(emu_lib)
    for name in NAMES:
        assert hasattr(lib, name)


def test_struct_layouts(tmp_path):
    from traceweaver_amd import _ffi

    pairs = (("tw_conf_query", _ffi.ConfQuery), ("tw_confidence", _ffi.Confidence))
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "traceweaver_amd.h"', 'int main(void) {', 'printf("%d", TW_TREE_CONFIDENT);']
    for c_name, t in pairs:
        src += ['printf(" %%zu", sizeof(%s));' % c_name] + ['printf(" %%zu", offsetof(%s, %s));' % (c_name, m) for m, _ in t._fields_]
    src += ['printf("\\n");', "return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(src))
    exe = str(tmp_path / "abi")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "abi.c"), "-o", exe])
    bit, *nums = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert bit == _ffi.TW_TREE_CONFIDENT == traces.CONFIDENT == 8
    for c_name, t in pairs:
        n = 1 + len(t._fields_)
        assert [ctypes.sizeof(t)] + [getattr(t, m).offset for m, _ in t._fields_] == nums[:n], c_name
        nums = nums[n:]
    assert ctypes.sizeof(_ffi.Confidence) == 8 * len(_ffi.Confidence._fields_) and ctypes.sizeof(_ffi.ConfQuery) == 24


def test_timing_slots_are_appended(emu_lib):
    """tw_get_timing keeps its first 19 slots; the scoring figures follow them."""
    eng = Engine(0, lib_path=emu_lib)
    assert list(eng.attribute_timing()) == ["tree", "select", "reduce"] and list(eng.score_timing()) == ["decisions", "trees", "calibration"]
    ms = np.full(24, -1.0)
    eng._lib.tw_get_timing(eng._h, ctypes.c_void_p(ms.ctypes.data), 22)
    assert (ms[:22] >= 0).all() and (ms[22:] == -1.0).all()
    eng.close()
