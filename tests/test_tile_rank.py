"""Phase 5 of k_enumerate_tile's general path (traceweaver_amd/csrc/tw_tile.h): a span of more than kRankDirect tuple slots is ranked
among its survivors only -- the feasible tuples that reach a lower bound L of the span's fifth-largest score (the smallest of the
maxima of five disjoint subsets of its slots), compacted into one list per segment and one per span.  Every unit goes through
parity.check_units (both passes against the oracle bit for bit: lists, scores, leaves, windows, selection, parents, gap samples),
with the new route and with TW_TILE_RANK=0 on the loop over all slots.  CPU tier: the host-emulation builds (the tiny tables, and the
production tables at which spans are long enough to be compacted), one lane-threaded run with the production tables; the HIP
library under -m gpu."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import parity

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# (seed, n_in, shape, concurrency, granularity_us) -> what the unit must hold for its case to mean something (_facts)
CASES = {
    (7, 300, "par4", 3, 1): ("mid", "mid_above_128"),                    # mid spans without ties
    (22, 300, "par4", 2.5, 1000): ("mid", "mid_twins", "mid_tied"),      # ties across L, undecided spans
    (23, 300, "chain3", 6, 1): ("mid_sparse",),                          # fewer than five feasible tuples: empty subsets, L = -inf
    (26, 300, "chain3", 5, 1000): ("mid_tied", "mid_sparse"),            # both at once
    (24, 300, "diamond", 5, 1): ("four_endpoints", "ordered", "mid_sparse"),
    (25, 300, "par2", 10, 1000): ("two_endpoints", "exactly_32", "mid_tied"),
    (27, 200, "fan6", 2, 1): ("six_endpoints", "mid_sparse"),            # a class of k_enumerate_lean (tile limit tile_max_deep)
    (28, 129, "par4", 2.5, 1): ("a_tile_and_one",),
}
SINGLES = [(101, 300, "single", 1.6, 1), (102, 300, "single", 4, 1000), (103, 400, "single", 12, 1000), (104, 400, "single", 24, 1)]
MIXED = [c for pair in zip(CASES, itertools.cycle(SINGLES)) for c in pair]   # the cases alternating with single-endpoint units
TILE, TILE_MAX, NARROW = 128, 256, 32   # kTile, TW_TILE_MAX, kNarrow of the HIP build
MID_MIN = 65                            # above every kRankDirect that is measured (16 / 32 / 64): such a span is compacted


def _facts(u, p1):
    """From the inputs alone (FindCutoffs, containment, call order), but for `mid_tied`: the scores of the oracle's pass 1."""
    E, n = u.E, u.n_in
    off = np.asarray(u.out_off)
    os_ = [np.asarray(u.out_start[off[e]:off[e + 1]]) for e in range(E)]
    oe = [np.asarray(u.out_end[off[e]:off[e + 1]]) for e in range(E)]
    dag = np.asarray(u.dag).reshape(E, E)
    f = dict.fromkeys(("mid", "mid_above_128", "mid_twins", "mid_tied", "mid_sparse", "exactly_32", "above_256"), 0)
    for i in range(n):
        a, b = int(u.in_start[i]), int(u.in_end[i])
        lo, hi = [0] * E, [0] * E
        for e in range(E - 1, -1, -1):   # reverse topological order
            tmax = b
            for s in range(e + 1, E):
                if dag[e, s]:
                    tmax = min(tmax, int(os_[s][hi[s]]))   # (hi = -1: Python's wrap to the last span)
            lo[e] = int(np.searchsorted(os_[e], a, side="left"))
            hi[e] = int(np.searchsorted(os_[e], tmax, side="right")) - 1
        width = [hi[e] - lo[e] + 1 for e in range(E)]
        if min(width) <= 0:
            continue
        cands = []
        for e in range(E):
            w = np.arange(lo[e], hi[e] + 1)
            cands.append(w[(os_[e][w] >= a) & (oe[e][w] <= b)])
        grid = int(np.prod([len(c) for c in cands], dtype=np.int64))
        f["exactly_32"] += max(width) == NARROW
        narrow = max(width) <= NARROW
        f["above_256"] += grid > TILE_MAX
        if not (narrow and MID_MIN <= grid <= TILE_MAX):
            continue
        f["mid"] += 1
        f["mid_above_128"] += grid > 128
        f["mid_twins"] += any(len(c) > 1 and bool((np.diff(os_[e][c]) == 0).any()) for e, c in enumerate(cands))
        feasible = 0
        for tup in itertools.product(*cands):
            feasible += all(oe[p][tup[p]] <= os_[e][tup[e]] for e in range(E) for p in range(e) if dag[p, e])
            if feasible >= 5:
                break
        f["mid_sparse"] += feasible < 5
        sc = p1["topk2_score"][i]
        sc = sc[~np.isnan(sc)]
        f["mid_tied"] += len(np.unique(sc)) < len(sc)
    f["two_endpoints"], f["four_endpoints"], f["six_endpoints"] = E == 2, E == 4, E == 6
    f["ordered"] = bool(dag.any())
    f["a_tile_and_one"] = n == TILE + 1
    return f


@pytest.fixture(scope="module")
def rank_units():
    units, _ = parity.stress_units(list(CASES))
    return units


@pytest.fixture(scope="module")
def emu_prod_lib(emu_lib):
    """The emulation build with the table sizes of the HIP build (a thread per workgroup, as emu_lib sets it up): tile limit 256, so
    that the mid spans are the tile kernel's own and are compacted.  (The tiny tables hold spans of at most 24 tuples.)"""
    from tests.hostemu.build_emu import build

    return build(production=True)


def test_units_hold_what_their_cases_are_for(rank_units):
    for case, u in zip(CASES, rank_units):
        svc = parity.oracle_service(u)
        end_flag, _, _ = parity.T.windows(svc)
        f = _facts(u, parity.T.run_pass(svc, end_flag, gauss=parity.T.gauss_params(svc)))
        print(case, {k: int(v) for k, v in f.items()})
        for need in CASES[case]:
            assert f[need], "%s: no %s" % (case, need)
        assert f["above_256"], "%s: no span beyond the tile limit" % (case,)


@pytest.mark.parametrize("rank", ["1", "0"])
def test_rank_units_emulated(emu_lib, monkeypatch, rank_units, rank):
    monkeypatch.setenv("TW_TILE_RANK", rank)
    parity.check_units(emu_lib, rank_units)


@pytest.mark.parametrize("rank", ["1", "0"])
def test_rank_units_emulated_with_production_tables(emu_prod_lib, monkeypatch, rank_units, rank):
    monkeypatch.setenv("TW_TILE_RANK", rank)
    parity.check_units(emu_prod_lib, rank_units)


@pytest.mark.parametrize("rank", ["1", "0"])
def test_mixed_batch_emulated(emu_prod_lib, monkeypatch, rank):
    monkeypatch.setenv("TW_TILE_RANK", rank)
    units, _ = parity.stress_units(MIXED)
    parity.check_units(emu_prod_lib, units)


_LANES = (
    "import sys, os\n"
    "sys.path[:0] = [%r, %r, %r]\n"
    "import parity\n"
    "units, _ = parity.stress_units([(22, 300, 'par4', 2.5, 1000), (26, 300, 'chain3', 5, 1000), (28, 129, 'par4', 2.5, 1)])\n"
    "parity.check_units(%r, units)\n"
    "print('lanes ok')\n"
)


def test_lane_threaded_ranks_with_production_tables():
    """A host thread per lane, 256 to a tile of 128 spans, with the table sizes of the HIP build: the maxima through atomics, the
    appends of whole wavefronts to the segment's list and to the spans' lists, the lists in the term tables between phase 4 and
    phase 5b, sub-tile workgroups (TW_TILE_SUB=2) -- and the loop over all slots on the same units."""
    from tests.hostemu.build_emu import build

    code = _LANES % (REPO, HERE, os.path.join(REPO, "oracle"), build(production=True))
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256", TW_TILE_SUB="2")
    # (the two routes side by side, a process each: the test is as long as the slower one)
    runs = [subprocess.Popen([sys.executable, "-c", code], env=dict(env, TW_TILE_RANK=v), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for v in ("1", "0")]
    for v, p in zip(("1", "0"), runs):
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0 and "lanes ok" in out, "TW_TILE_RANK=%s: %s" % (v, err[-2000:])


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rank", ["1", "0"])
def test_rank_units_on_the_gpu(monkeypatch, rank_units, rank):
    monkeypatch.setenv("TW_TILE_RANK", rank)
    parity.check_units(None, rank_units)


@pytest.mark.gpu
def test_mixed_batch_on_the_gpu_twice():
    units, _ = parity.stress_units(MIXED)
    a1, a2, _ = parity.check_units(None, units)
    b1, b2, _ = parity.check_units(None, units)
    for x, y in zip(a1 + a2, b1 + b2):
        _assert_same(x, y)


def _assert_same(x, y):
    assert sorted(x) == sorted(y)
    for k in x:
        if isinstance(x[k], np.ndarray):
            assert np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == "f"), k
        else:
            assert x[k] == y[k], k


_AB = (
    "import sys, pickle\n"
    "sys.path[:0] = [%r]\n"
    "from traceweaver_amd import synth\n"
    "from traceweaver_amd.engine import Engine\n"
    "units = [synth.make_unit(301 + k, 20000, shape=s, concurrency=c, granularity_us=g)[0]\n"
    "         for k, (s, c, g) in enumerate([('par4', 1.6, 1), ('par4', 3, 1), ('chain3', 5, 1000), ('diamond', 5, 1)])]\n"
    "eng = Engine(0)\n"
    "eng.load(units)\n"
    "eng.run_pass1()\n"
    "r1 = eng.results(1)\n"
    "eng.fit_mixtures()\n"
    "eng.run_pass2()\n"
    "r2 = eng.results(2)\n"
    "eng.close()\n"
    "with open(sys.argv[1], 'wb') as f:\n"
    "    pickle.dump((r1, r2), f)\n"
)


@pytest.mark.gpu
def test_both_routes_agree_at_scale_on_the_gpu(tmp_path):
    """Four units of 20 000 requests (par4 at concurrency 1.6 and 3, chain3 at 5 millisecond-granular, diamond at 5), solved in fresh
    child processes with the compacted ranks and with the loop over all slots: all of results(1) and results(2) are equal."""
    import pickle

    got = []
    for v in ("1", "0"):
        out = str(tmp_path / ("rank%s.pkl" % v))
        p = subprocess.run([sys.executable, "-c", _AB % REPO, out], env=dict(os.environ, TW_TILE_RANK=v), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        with open(out, "rb") as f:
            got.append(pickle.load(f))
    for a, b in zip(got[0][0] + got[0][1], got[1][0] + got[1][1]):
        _assert_same(a, b)
