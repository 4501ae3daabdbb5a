"""Skip mode beyond the frozen reference runs: the device walk (csrc/tw_skip.h, its host side in tw_engine.hip and
skipmode.py) against the oracle's skip mode on synthetic units (tests/skip_cases.py) -- skipped calls at later endpoints
(the skipped-predecessor branches of the scorer), skipped predecessors that order nothing, pools at several endpoints,
several units in one batch (the per-unit offsets), millisecond-granular ties, time windows carried over from another
service, the status codes and the candidate cap -- bit for bit.  A CPU tier on the host-emulation build and a GPU twin of
every test but the lane-threaded one."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parity
import skip_cases as S
from conftest import assert_pass_equal

IDS = ["%s_n%d_c%s_g%d_%s_%s" % (c[2], c[1], c[3], c[4], "".join(str(e) for e in c[5]), c[7]) for c in S.CASES]
RESULT_ARRAYS = ("parent", "topk_idx", "topk_score", "topk_n", "chosen", "leaves", "window_end")


def made(cases):
    pairs = [S.make(c) for c in cases]
    return [u for u, _ in pairs], [t for _, t in pairs]


def same_results(a, b):
    for ra, rb in zip(a, b):
        for name in RESULT_ARRAYS:
            assert np.array_equal(S.bits(ra[name]), S.bits(rb[name])), name
        assert all(ra[k] == rb[k] for k in ("not_best_count", "cnt_unassigned", "n_windows", "budget_windows"))


# ------------------------------------------------------------------------------------------------ the cases themselves
def test_cases_are_what_they_claim(oracle):
    """Every unit of CASES is solved by the oracle with every selection search complete and holds skipped calls; every
    unit of RAISING gets the code recorded for it (a unit never moves between the lists silently); over the set the
    branches the frozen runs do not reach occur."""
    sizes = [c[1] for c in S.CASES]
    assert all(150 <= n <= 600 for n in sizes) and {257, 301} <= set(sizes)
    seen = {}
    for c in S.CASES:
        u, truth = S.make(c)
        op, end_flag, code, o = S.oracle_skip(u)
        assert code == 0 and o["budget_windows"] == 0, c
        assert (o["parent"] == -2).sum() > 0 and (truth == -2).sum() > 0, c
        for k, v in S.coverage(u, o).items():
            seen[k] = seen.get(k, False) or v
    assert seen == {"later_skip_chosen": True, "skipped_pred_with_ancestor": True, "not_best": True, "unassigned": True}
    for c, want in S.RAISING:
        assert S.oracle_skip(S.make(c)[0])[2] == want, c
    kinds = {(c[2], tuple(c[5])) for c, _ in S.RAISING}
    assert {("single", (0,)), ("chain3", (0, 1)), ("par4", (0, 3)), ("mix8", (0, 4, 7))} <= kinds
    # the unit at high concurrency: a window at the size cap, and spans consumed by earlier windows
    (busy,) = [c for c in S.CASES if c[3] >= 6]
    u, _ = S.make(busy)
    end_flag, o = S.oracle_skip(u)[1], S.oracle_skip(u)[3]
    assert np.diff(np.concatenate([[-1], np.flatnonzero(end_flag)])).max() >= 30
    assert (o["topk_n"] != o["topk2_n"]).any() or (o["topk_idx"] != o["topk2_idx"]).any()


def one_alone(lib, case):
    u, truth = S.make(case)
    res, _, _ = S.check_skip_units(lib, [u], truth=[truth])
    assert (res[0]["parent"] == -2).sum() > 0


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_unit_alone_emulated(emu_lib, oracle, case):
    one_alone(emu_lib, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_unit_alone_gpu(oracle, case):
    one_alone(None, case)


def one_batch(lib):
    """All units in one load (units > 0 read their time windows, pools, tables and draw counters at their offsets), then
    in reversed order: a unit's result does not depend on its neighbours."""
    units, truth = made(S.CASES)
    fwd, _, _ = S.check_skip_units(lib, units, truth=truth)
    rev, _, _ = S.check_skip_units(lib, units[::-1], truth=truth[::-1])
    same_results(fwd, rev[::-1])
    for r in fwd:
        assert (r["parent"] == -2).sum() > 0


def test_one_batch_emulated(emu_lib, oracle):
    one_batch(emu_lib)


@pytest.mark.gpu
def test_one_batch_gpu(oracle):
    one_batch(None)


def pass_twice(lib):
    """The draw counters are cleared per pass: the pass run again on the loaded batch gives the same arrays."""
    from traceweaver_amd import skipmode
    from traceweaver_amd.engine import Engine

    units, truth = made(S.CASES[1:6])
    eng = Engine(0, lib_path=lib)
    plans = [skipmode.plan(eng, u) for u in units]
    first = S.run_skip_batch(eng, units, plans, truth)
    eng.run_pass1()
    second = (eng.results(1), eng.decisions(1), eng.evaluate())
    eng.close()
    same_results(first[0], second[0])
    for a, b in zip(first[1], second[1]):
        assert all(np.array_equal(S.bits(a[k]), S.bits(b[k])) for k in a)
    assert first[2] == second[2]
    for k, u in enumerate(units):
        S.assert_unit_equal(second[0][k], second[1][k], second[2][k], *S.oracle_skip(u)[:2], S.oracle_skip(u)[3], truth=truth[k], tag="unit %d:" % k)


def test_pass_twice_emulated(emu_lib, oracle):
    pass_twice(emu_lib)


@pytest.mark.gpu
def test_pass_twice_gpu(oracle):
    pass_twice(None)


ORDINARY = [(2, 150, "chain3", 4, 1), (4, 120, "par2", 6, 1)]


def engine_reuse(lib):
    """One engine, skip batch -> ordinary batch -> skip batch: every result equals a fresh engine's and the oracle's."""
    from traceweaver_amd.engine import Engine

    a, ta = made(S.CASES[0:3])
    b, tb = made(S.CASES[3:8])
    plain, _ = parity.stress_units(ORDINARY)
    fresh_a, _, _ = S.check_skip_units(lib, a, truth=ta)
    fresh_b, _, _ = S.check_skip_units(lib, b, truth=tb)
    fresh_p, _, ora = parity.check_units(lib, plain)
    eng = Engine(0, lib_path=lib)
    res_a, _, _ = S.check_skip_units(lib, a, truth=ta, engine=eng)
    eng.load(plain)
    eng.run_pass1()
    res_p = eng.results(1)
    res_b, _, _ = S.check_skip_units(lib, b, truth=tb, engine=eng)
    eng.close()
    same_results(res_a, fresh_a)
    same_results(res_b, fresh_b)
    same_results(res_p, fresh_p)
    for k in range(len(plain)):
        assert_pass_equal(res_p[k], ora[k][2], ora[k][1], "ordinary unit %d: pass 1" % k)


def test_engine_reuse_emulated(emu_lib, oracle):
    engine_reuse(emu_lib)


@pytest.mark.gpu
def test_engine_reuse_gpu(oracle):
    engine_reuse(None)


# ------------------------------------------------------------------------------------------------ prior_windows (hazard H8)
PRIOR_A = (121, 200, "chain2", 2, 1)                       # the service solved before: only its time windows matter
PRIOR_B = (122, 200, "chain3", 2, 1, (1,), 0.2, "drop")


def prior_windows(lib):
    """The reference never clears its list of time windows: unit B is planned and solved with unit A's windows in the list
    (overlapping time ranges), and requests of B draw from pools of windows that came from A."""
    from traceweaver_amd import skipmode, synth

    a, _ = synth.make_unit(*PRIOR_A[:2], shape=PRIOR_A[2], concurrency=PRIOR_A[3], granularity_us=PRIOR_A[4])
    prior = skipmode.time_windows(a)
    u, truth = S.make(PRIOR_B)
    own = skipmode.time_windows(u)
    assert prior[0][0] < u.in_start[-1] and u.in_start[0] < prior[-1][0]       # the time ranges overlap
    S.check_skip_units(lib, [u], prior=prior, truth=[truth])
    keys = S.oracle_skip(u, prior)[0].windows
    starts = np.array([k[0] for k in keys], dtype=np.int64)
    from_a = 0
    for t in u.in_start:                                                       # FindWindow: the largest start <= the request's
        best = starts[starts <= t].max()
        first = int(np.flatnonzero(starts == best)[0])
        from_a += keys[first] in prior and keys[first] not in own
    assert from_a > 0
    assert not np.array_equal(S.oracle_skip(u, prior)[3]["topk2_idx"], S.oracle_skip(u)[3]["topk2_idx"])   # and it matters


def test_prior_windows_emulated(emu_lib, oracle):
    prior_windows(emu_lib)


@pytest.mark.gpu
def test_prior_windows_gpu(oracle):
    prior_windows(None)


# ------------------------------------------------------------------------------------------------ statuses
def statuses(lib):
    """Every refusal on a single-unit batch, with the oracle's code next to it; after each the same engine solves a unit of
    CASES (the error word does not stick).  Then a raising unit among solvable ones: the call fails with its code."""
    from traceweaver_amd import skipmode
    from traceweaver_amd.engine import Engine, EngineError

    good, good_truth = S.make(S.CASES[1])
    eng = Engine(0, lib_path=lib)

    def recovers():
        S.check_skip_units(lib, [good], truth=[good_truth], engine=eng)

    for c, code in S.RAISING:                                                   # -6 -> -9, -7 -> -8
        u = S.make(c)[0]
        assert S.oracle_skip(u)[2] == code, c
        assert S.expect_status(eng, u, S.ENGINE_CODE[code]) == "pass", c
        recovers()
    # a request before the first time window: the oracle's -6, TW_ERR_ARG on the device
    sp = skipmode.plan(eng, good)
    late = skipmode.SkipPlan(sp.windows[1:], sp.budget, np.ascontiguousarray(sp.pool[:, 1:]), sp.dist, sp.large_delay)
    assert S.oracle_skip(good, plan=late)[2] == -6
    assert S.expect_status(eng, good, -1, plan=late) == "pass"
    recovers()
    # a pool above TW_SKIP_STRIDE: the oracle's -3, TW_ERR_ARG at load
    pool = sp.pool.copy()
    pool[1, 0] = S._ffi.TW_SKIP_STRIDE + 1
    big = skipmode.SkipPlan(sp.windows, sp.budget, pool, sp.dist, sp.large_delay)
    assert S.oracle_skip(good, plan=big)[2] == -3
    assert S.expect_status(eng, good, -1, plan=big) == "load"
    recovers()
    # one raising unit among solvable ones
    for c, code in (S.RAISING[1], S.RAISING[3]):
        units, _ = made([S.CASES[0], S.CASES[4], c, S.CASES[7]])
        with pytest.raises(EngineError) as ex:
            S.run_skip_batch(eng, units, [skipmode.plan(eng, u) for u in units])
        assert ex.value.code == S.ENGINE_CODE[code]
    recovers()
    eng.close()


def test_statuses_emulated(emu_lib, oracle):
    statuses(emu_lib)


@pytest.mark.gpu
def test_statuses_gpu(oracle):
    statuses(None)


# ------------------------------------------------------------------------------------------------ the candidate cap
def cap_unit(n_spans, n_in=70):
    """Two endpoints, 0 -> 1.  Request 0 contains `n_spans` spans of endpoint 0 and one of endpoint 1; the other requests
    follow one after the other, each with its call to endpoint 1 and none to endpoint 0.  Returns (unit, truth, plan): the
    plan holds the time windows and pools of TallySkipSpans and a hand-written (mean, std) table with every pair finite."""
    from traceweaver_amd import skipmode
    from traceweaver_amd.engine import UnitArrays

    t0 = 1_600_000_000_000_000
    in_start = t0 + np.concatenate([[0], 20_000 + 3_000 * np.arange(n_in - 1)]).astype(np.int64)
    in_end = in_start + np.concatenate([[10_000], np.full(n_in - 1, 2_000)]).astype(np.int64)
    s0 = t0 + 100 + 100 * np.arange(n_spans, dtype=np.int64)                   # inside request 0, before its endpoint-1 call
    e0 = s0 + 50
    s1 = np.concatenate([[t0 + 8_000], in_start[1:] + 500]).astype(np.int64)
    e1 = s1 + 1_000
    dag = np.array([[0, 1], [0, 0]], dtype=np.uint8)
    unit = UnitArrays(in_start, in_end, [0, n_spans, n_spans + n_in], np.concatenate([s0, s1]), np.concatenate([e0, e1]), dag)
    truth = np.stack([np.full(n_in, -2, dtype=np.int32), np.arange(n_in, dtype=np.int32)])
    truth[0, 0] = 0
    keys, budget, pool = skipmode.tally_skip_spans(unit)
    dist = np.empty((3, 3, 2))
    dist[..., 0], dist[..., 1] = 3_000.0, 50_000.0      # wide: no density underflows, no two tuples of a request tie
    return unit, truth, skipmode.SkipPlan(keys, budget, pool, dist, int(np.max(in_end - in_start)))


def candidate_cap(lib):
    """kSkipCand = 64 spans of an endpoint inside one request are solved and equal the oracle; 65 are refused with
    TW_ERR_WINDOW_WIDTH (the oracle has no cap)."""
    from traceweaver_amd.engine import Engine

    unit, truth, plan = cap_unit(64)
    res, _, ora = S.check_skip_units(lib, [unit], plans=[plan], truth=[truth])
    assert res[0]["leaves"][0] == 64 and res[0]["topk_n"][0] == 5               # every span with the one call to endpoint 1 (the water level leaves this time window no skip span)
    unit, truth, plan = cap_unit(65)
    eng = Engine(0, lib_path=lib)
    assert S.expect_status(eng, unit, -5, plan=plan) == "pass"
    eng.close()


def test_candidate_cap_emulated(emu_lib, oracle):
    candidate_cap(emu_lib)


@pytest.mark.gpu
def test_candidate_cap_gpu(oracle):
    candidate_cap(None)


# ------------------------------------------------------------------------------------------------ the wavefront as written
LANE_CASES = [(131, 150, "diamond", 2, 1, (1, 2), 0.15, "drop"), (132, 120, "chain2", 3, 1000, (1,), 0.2, "drop"),
              (133, 100, "chain3", 4, 1, (1,), 0.2, "drop")]


def test_lane_threaded_skip_walk(emu_lib, oracle):
    """TW_EMU_LANES=1: k_skip_walk by 64 host threads per unit, cross-lane operations as rendezvous -- lane 0's hand-over
    of a window's candidate lists to select_window_coop (with conflicts between tuples that hold the same skip span) as
    it is written -- on three small units in one batch, held to the oracle."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r, %r]\n"
        "import skip_cases as S\n"
        "pairs = [S.make(c) for c in %r]\n"
        "res, _, _ = S.check_skip_units(%r, [u for u, _ in pairs], truth=[t for _, t in pairs])\n"
        "assert all((r['parent'] == -2).sum() > 0 for r in res)\n"
        "print('lanes ok')\n"
    ) % (os.path.dirname(here), here, os.path.join(os.path.dirname(here), "oracle"), LANE_CASES, emu_lib)
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256", TW_TILE_SUB="2")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "lanes ok" in out.stdout, out.stderr[-2000:]
