"""Synthetic skip-mode units and the engine-vs-oracle comparison on them, shared by the host-emulation tier (CPU) and the GPU
tier of tests/test_skip_synth.py.

The frozen reference runs (tests/golden/refskip_*) hold one service, one call-order DAG and cache hits at the first endpoint
only.  The units here are synth.make_unit units that lost a share of their calls at chosen endpoints -- drop_calls: any
endpoint, lists stay sorted -- or through skipmode.cache_hits (first endpoint, later spans shifted, lists no longer sorted).
The yardstick is the oracle's skip mode (tally_skip_spans, build_distributions, run_skip in oracle/tw_oracle.py), which
tests/test_skip_oracle.py pins to the reference."""
import numpy as np

import parity
import tw_oracle as T
from traceweaver_amd import _ffi, skipmode, synth, traces
from traceweaver_amd.engine import Engine, EngineError, UnitArrays

# (seed, n_in, shape, concurrency, granularity_us, endpoints, rate, how): how = "drop" (drop_calls at `endpoints`) or "cache"
# (skipmode.cache_hits: the first endpoint).  Every unit is solved by the oracle (code 0, every selection search complete).
CASES = [
    (101, 301, "chain3", 2, 1, (0,), 0.2, "drop"),        # the first endpoint, as the frozen runs, on sorted lists
    (102, 257, "chain3", 2, 1, (1,), 0.2, "drop"),        # a middle endpoint: its successor is scored from the ancestor's start
    (103, 200, "chain3", 2, 1, (2,), 0.25, "drop"),       # the last endpoint: the closing term moves to another endpoint
    (104, 200, "chain3", 1.5, 1, (0, 2), 0.15, "drop"),   # pools at two endpoints of one unit
    (105, 200, "diamond", 2, 1, (1, 2), 0.15, "drop"),    # a skipped predecessor with a predecessor of its own
    (106, 150, "chain5", 1.5, 1, (1, 3), 0.15, "drop"),
    (107, 150, "fan6", 1.5, 1, (2, 5), 0.15, "drop"),
    (108, 300, "par2", 3, 1, (1,), 0.2, "drop"),          # no call order at all
    (109, 200, "chain2", 3, 1000, (1,), 0.2, "drop"),     # millisecond-granular: score ties walk into the span lists
    (110, 200, "par2", 2, 1000, (1,), 0.2, "drop"),
    (114, 300, "chain3", 12, 1, (1,), 0.1, "drop"),       # windows at the size cap, spans consumed across windows
    (112, 300, "chain3", 2, 1, (0,), 0.2, "cache"),       # create_cache_hits: unsorted lists, the perm route
    (113, 200, "diamond", 2, 1, (0,), 0.15, "cache"),
    (203, 150, "par4", 2, 1, (0, 3), 0.2, "drop"),        # four unordered endpoints, pools at two of them
    (210, 150, "mix8", 1.3, 1, (0, 4, 7), 0.2, "drop"),   # TW_MAX_EP endpoints, pools at three
]

# (case, the oracle's code): units on which the reference raises.  -6: a tuple that skips every endpoint, a skipped
# predecessor all of whose predecessors are skipped, or a score tie compared through a skip span; -7: the scorer needs a
# (mean, std) pair BuildDistributions did not produce.
RAISING = [
    ((201, 150, "single", 2, 1, (0,), 0.2, "drop"), -6),          # every tuple skips everything
    ((202, 150, "chain3", 2, 1, (0, 1), 0.2, "drop"), -6),
    ((205, 150, "par4", 2, 1, (0, 3), 0.2, "drop"), -6),
    ((207, 150, "mix8", 1.1, 1, (0, 4, 7), 0.2, "drop"), -7),     # a missing (mean, std) pair
]

ENGINE_CODE = {-6: -9, -7: -8}   # the oracle's code -> TW_ERR_SKIP_REFERENCE_RAISES, TW_ERR_SKIP_PARAMS


def drop_calls(unit, true_parent, endpoints, rate, seed):
    """Per listed endpoint int(rate * n) requests, drawn without replacement from np.random.default_rng(seed), lose their call
    to it: the span leaves the endpoint's list, nothing else moves (the lists stay sorted).  Returns (the unit as the
    predictor receives it, true_parent with -2 = the request did not call the endpoint)."""
    rng = np.random.default_rng(seed)
    n, E = unit.n_in, unit.E
    tp = np.array(true_parent, dtype=np.int32).copy()
    starts = [unit.out_start[unit.out_off[e]:unit.out_off[e + 1]] for e in range(E)]
    ends = [unit.out_end[unit.out_off[e]:unit.out_off[e + 1]] for e in range(E)]
    for e in endpoints:
        hit = rng.choice(n, size=int(rate * n), replace=False)
        keep = np.ones(len(starts[e]), dtype=bool)
        keep[tp[e, hit]] = False
        new_index = np.cumsum(keep) - 1
        tp[e] = new_index[tp[e]]
        tp[e, hit] = -2
        starts[e], ends[e] = starts[e][keep], ends[e][keep]
    off = np.concatenate([[0], np.cumsum([len(s) for s in starts])]).astype(np.int64)
    return UnitArrays(unit.in_start, unit.in_end, off, np.concatenate(starts), np.concatenate(ends), unit.dag, unit.key_rank), tp


_made = {}


def make(case):
    """(unit, truth) of a CASES / RAISING entry; made once."""
    if case not in _made:
        seed, n, shape, conc, gran, endpoints, rate, how = case
        u, tp = synth.make_unit(seed, n, shape=shape, concurrency=conc, granularity_us=gran)
        if how == "drop":
            _made[case] = drop_calls(u, tp, endpoints, rate, seed)
        else:
            assert how == "cache" and tuple(endpoints) == (0,)
            _made[case] = skipmode.cache_hits(u, tp, rate)[:2]
    return _made[case]


class OraclePlan(object):
    """What the oracle hands its pass for one unit: time windows, skip budget, pools, (mean, std) table."""

    def __init__(self, svc, prior=(), plan=None):
        if plan is None:
            self.windows, self.budget, self.pool = T.tally_skip_spans(svc, prior)
            self.dist, self.large_delay = T.build_distributions(svc)
        else:   # a hand-made plan goes to both sides as it is
            self.windows, self.budget, self.pool, self.dist, self.large_delay = plan.windows, plan.budget, plan.pool, plan.dist, plan.large_delay


_solved = {}


def oracle_skip(unit, prior=(), plan=None):
    """(OraclePlan, window ends, the oracle's code, its result or None).  Without a hand-made plan the answer is kept per
    (unit, prior): the tests ask for the same unit alone, in batches and on reused engines."""
    key = (id(unit), tuple(prior))
    if plan is None and key in _solved:
        return _solved[key][1:]
    svc = parity.oracle_service(unit)
    op = OraclePlan(svc, prior, plan)
    end_flag = T.windows(svc)[0]
    try:
        o, code = T.run_skip(svc, end_flag, op.windows, op.pool, op.dist), 0
    except RuntimeError as ex:
        o, code = None, int(str(ex).rsplit(":", 1)[1])
    if plan is None:
        _solved[key] = (unit, op, end_flag, code, o)   # (holds the unit: its id stays its own)
    return op, end_flag, code, o


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_plan_equal(sp, op, tag=""):
    """skipmode.plan against the oracle's: windows, budget, pool, large_delay, and the table with NaNs in the same cells."""
    assert list(sp.windows) == list(op.windows), tag + " time windows"
    assert np.array_equal(sp.budget, op.budget), tag + " skip budget"
    assert np.array_equal(sp.pool, op.pool), tag + " pools"
    assert sp.large_delay == op.large_delay, tag + " large_delay"
    m = ~np.isnan(op.dist)
    assert np.array_equal(np.isnan(sp.dist), ~m), tag + " (mean, std) table: cells"
    assert np.array_equal(bits(sp.dist[m]), bits(op.dist[m])), tag + " (mean, std) table: values"


def run_skip_batch(eng, units, plans, truth=None):
    """Loads the units as one skip-mode batch and runs the pass; returns (results, decisions, evaluation or None)."""
    eng.load(units, skip=plans)
    if truth is not None:
        eng.set_truth(truth)
    eng.run_pass1()
    return eng.results(1), eng.decisions(1), (eng.evaluate() if truth is not None else None)


def assert_unit_equal(r, dec, ev, op, end_flag, o, truth=None, tag=""):
    """One unit of a skip-mode batch against the oracle's run: what tests/test_skip_engine.py::check compares with the
    oracle, the decisions and the evaluation."""
    assert np.array_equal(r["window_end"], end_flag), tag + " window ends"
    assert np.array_equal(r["topk_n"], o["topk2_n"]), tag + " candidate counts"
    assert np.array_equal(np.transpose(r["topk_idx"], (2, 0, 1)), o["topk2_idx"]), tag + " top-5 tuples"
    ok = ~np.isnan(o["topk2_score"])
    assert np.array_equal(bits(r["topk_score"].T[ok]), bits(o["topk2_score"][ok])), tag + " top-5 scores"
    assert np.isnan(r["topk_score"].T[~ok]).all(), tag + " scores beyond the list"
    assert np.array_equal(r["chosen"], o["chosen"]), tag + " selection"
    assert np.array_equal(r["parent"], o["parent"]), tag + " parent arrays"
    assert np.array_equal(r["leaves"], o["leaves"]), tag + " enumerated tuples"
    assert (r["not_best_count"], r["cnt_unassigned"], r["n_windows"]) == (o["not_best_count"], o["cnt_unassigned"], o["n_windows"]), tag + " counters"
    assert r["budget_windows"] == 0 and o["budget_windows"] == 0, tag + " a selection search ran out of its budget"
    want = traces.decisions_host(o)
    for name in ("rank", "list_n", "margin"):
        assert np.array_equal(bits(dec[name]), bits(want[name])), tag + " decisions: " + name
    if truth is not None:
        assert ev["correct"] == int(np.all(r["parent"] == truth, axis=0).sum()) == int(np.all(o["parent"] == truth, axis=0).sum()), tag + " correct"


def check_skip_units(lib_path, units, plans=None, prior=(), truth=None, engine=None):
    """Loads all units as one skip-mode batch, runs the pass and compares every unit with the oracle (every unit must be one
    the oracle solves).  plans: per unit a hand-made skipmode.SkipPlan that both sides take, or None = skipmode.plan, which is
    then held to the oracle's plan too.  prior: time windows of services solved before (hazard H8), for every unit.
    engine: an engine to run on (it stays open) instead of a fresh one.  Returns (results, decisions, oracle results)."""
    eng = Engine(0, lib_path=lib_path) if engine is None else engine
    try:
        ora, use = [], []
        for k, u in enumerate(units):
            hand = None if plans is None else plans[k]
            op, end_flag, code, o = oracle_skip(u, prior, hand)
            assert code == 0, "unit %d: the oracle returns %d" % (k, code)
            ora.append((op, end_flag, o))
            if hand is None:
                hand = skipmode.plan(eng, u, prior)
                assert_plan_equal(hand, op, "unit %d:" % k)
            use.append(hand)
        res, dec, ev = run_skip_batch(eng, units, use, truth)
    finally:
        if engine is None:
            eng.close()
    for k in range(len(units)):
        assert_unit_equal(res[k], dec[k], None if ev is None else ev[k], *ora[k], truth=None if truth is None else truth[k], tag="unit %d:" % k)
    return res, dec, [o for _, _, o in ora]


def expect_status(eng, unit, want, plan=None, prior=()):
    """A single-unit skip-mode batch that the engine must refuse with the status `want`; returns where it did: "load" or
    "pass"."""
    sp = skipmode.plan(eng, unit, prior) if plan is None else plan
    stage = "load"
    try:
        eng.load([unit], skip=[sp])
        stage = "pass"
        eng.run_pass1()
    except EngineError as ex:
        assert ex.code == want, "status %d, expected %d (%s)" % (ex.code, want, _ffi.STATUS.get(want))
        return stage
    raise AssertionError("the engine solved a unit it must refuse with %d" % want)


def primary_preds(dag):
    """[e] -> the predecessors the scorer reads (the transitive reduction of the call order)."""
    E = dag.shape[0]
    return [[p for p in range(E) if dag[p, e] and not any(m not in (p, e) and dag[p, m] and dag[m, e] for m in range(E))] for e in range(E)]


def coverage(unit, o):
    """Which of the skip-mode branches one solved unit reaches (for the assertions over the whole set)."""
    idx, n = o["topk2_idx"], o["topk2_n"]            # [n, K, E]
    dag = unit.dag
    skip = idx <= -T.SKIP_BASE
    live = np.arange(idx.shape[1])[None, :] < n[:, None]
    anc = np.zeros(idx.shape[:2], dtype=bool)
    prim = primary_preds(dag)
    for e in range(unit.E):
        for b in prim[e]:
            for a in np.flatnonzero(dag[:, b]):
                anc |= ~skip[:, :, e] & skip[:, :, b] & ~skip[:, :, a]
    return {"later_skip_chosen": bool((o["parent"][1:] == -2).any()), "skipped_pred_with_ancestor": bool((anc & live).any()),
            "not_best": bool((o["chosen"] > 0).any()), "unassigned": bool((o["chosen"] < 0).any())}
