"""The two-endpoint path of k_enumerate_tile (traceweaver_amd/csrc/tw_tile.h, PAIR): items and tuple slots named by their span's
thread, a tuple decoded by one division, unpadded slots, tables sized for the class, the survivor ranks shared with the general path.
Every unit goes through parity.check_units (both passes against the oracle bit for bit: lists, scores, leaves, windows, selection,
parents, gap samples, parameters), on the pair path and with TW_TILE_PAIR=0 on the general one.  CPU tier: the host-emulation builds
(the tiny tables, and the production tables at which spans of more than 32 tuples are the tile kernel's own), one lane-threaded run
with the production tables; the HIP library under -m gpu."""
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
    (301, 300, "par2", 1.6, 1): ("bench_regime", "no_twins", "none_above_256"),
    (302, 300, "par2", 4, 1000): ("twins", "mid"),                                   # phase 5b; survivor ranks
    (303, 400, "par2", 8, 1000): ("twins_and_above_256_in_a_tile", "several_segments"),
    (304, 400, "par2", 12, 1): ("wider_32", "above_256", "no_twins"),
    (305, 400, "par2", 24, 1): ("wider_32", "above_256"),
    (306, 257, "par2", 6, 1000): ("two_tiles_and_one",),
    (307, 2, "par2", 1, 1): ("smallest",),
    (311, 300, "chain2", 1.6, 1): ("ordered", "infeasible"),                         # per-tuple pair term, s_bits / s_leaves
    (312, 300, "chain2", 4, 1000): ("ordered", "infeasible", "twins"),
    (313, 400, "chain2", 12, 1): ("ordered", "above_256", "mid"),
    (314, 400, "chain2", 24, 1): ("ordered", "wider_32"),
}
OTHERS = [(101, 300, "single", 1.6, 1), (7, 300, "par4", 3, 1), (1, 400, "chain3", 1.5, 1)]
MIXED = [c for k, case in enumerate(CASES) for c in (case, OTHERS[k % len(OTHERS)])]   # the classes alternating in the batch
TILE, TILE_MAX, TILE_GRID, NARROW, WINDOW_LIMIT = 128, 256, 1024, 32, 128   # kTile, TW_TILE_MAX, TW_TILE_GRID, kNarrow, 64 * kCandWords of the HIP build


def _facts(u):
    """Recomputed from the inputs alone: FindCutoffs in reverse topological order, the containment test, the call order."""
    assert u.E == 2
    n = u.n_in
    off = np.asarray(u.out_off)
    os_ = [np.asarray(u.out_start[off[e]:off[e + 1]]) for e in range(2)]
    oe = [np.asarray(u.out_end[off[e]:off[e + 1]]) for e in range(2)]
    dag = np.asarray(u.dag).reshape(2, 2)
    assert not dag[1, 0] and not dag[0, 0] and not dag[1, 1]
    ordered = bool(dag[0, 1])
    tuples = np.zeros(n, np.int64)      # grid points: the product of the contained candidates
    widest = np.zeros(n, np.int64)
    twins = np.zeros(n, bool)
    infeasible = 0
    for i in range(n):
        a, b = int(u.in_start[i]), int(u.in_end[i])
        lo1 = int(np.searchsorted(os_[1], a, side="left"))
        hi1 = int(np.searchsorted(os_[1], b, side="right")) - 1
        tmax = min(b, int(os_[1][hi1])) if ordered else b   # (hi = -1: Python's wrap to the last span)
        lo0 = int(np.searchsorted(os_[0], a, side="left"))
        hi0 = int(np.searchsorted(os_[0], tmax, side="right")) - 1
        lo, hi = (lo0, lo1), (hi0, hi1)
        widest[i] = max(hi[e] - lo[e] + 1 for e in range(2))
        if min(hi[e] - lo[e] + 1 for e in range(2)) <= 0:
            continue
        cands = []
        for e in range(2):
            w = np.arange(lo[e], hi[e] + 1)
            cands.append(w[(os_[e][w] >= a) & (oe[e][w] <= b)])
        tuples[i] = len(cands[0]) * len(cands[1])
        twins[i] = tuples[i] > 0 and any(len(c) > 1 and bool((np.diff(os_[e][c]) == 0).any()) for e, c in enumerate(cands))
        if ordered and tuples[i] > 0:
            infeasible += int((oe[0][cands[0]][:, None] > os_[1][cands[1]][None, :]).sum())
    narrow = widest <= NARROW
    own = narrow & (tuples <= TILE_MAX)     # what the tile kernel enumerates itself
    tiles = np.arange(0, n, TILE)
    per_tile = np.add.reduceat(np.where(own, tuples, 0), tiles)
    both = np.logical_and(np.add.reduceat((twins & own).astype(np.int64), tiles) > 0, np.add.reduceat((tuples > TILE_MAX).astype(np.int64), tiles) > 0)
    mean = float(tuples[tuples > 0].mean()) if (tuples > 0).any() else 0.0
    return {
        "bench_regime": 3.0 <= mean <= 6.0,
        "no_twins": not twins.any(),
        "twins": int(twins.sum()) >= 1,
        "none_above_256": int((tuples > TILE_MAX).sum()) == 0,
        "above_256": int((tuples > TILE_MAX).sum()) >= 1,
        "mid": int((own & (tuples > NARROW)).sum()) >= 1,          # more than kRankDirect = 32 tuples: ranked among the survivors
        "twins_and_above_256_in_a_tile": bool(both.any()),
        "several_segments": int(per_tile.max()) > TILE_GRID,
        "wider_32": int((widest > NARROW).sum()) >= 1,
        "two_tiles_and_one": n == 2 * TILE + 1,
        "smallest": n == 2,
        "ordered": ordered,
        "infeasible": infeasible >= 1,
        "widest": int(widest.max()),
        "counts": dict(mean_tuples=round(mean, 2), twins=int(twins.sum()), above_256=int((tuples > TILE_MAX).sum()),
                       mid=int((own & (tuples > NARROW)).sum()), wider_32=int((widest > NARROW).sum()), infeasible=infeasible,
                       most_tuples_a_tile=int(per_tile.max())),
    }


@pytest.fixture(scope="module")
def pair_units():
    units, _ = parity.stress_units(list(CASES))
    return units


@pytest.fixture(scope="module")
def emu_prod_lib(emu_lib):
    """The emulation build with the table sizes of the HIP build (a thread per workgroup, as emu_lib sets it up): tile limit 256, so
    that spans of 33 to 256 tuples are the tile kernel's own.  (The tiny tables hold spans of at most 24 tuples.)"""
    from tests.hostemu.build_emu import build

    return build(production=True)


def test_units_hold_what_their_cases_are_for(pair_units):
    for case, u in zip(CASES, pair_units):
        f = _facts(u)
        print(case, f["widest"], f["counts"])
        for need in CASES[case]:
            assert f[need], "%s: no %s (%s)" % (case, need, f["counts"])
        assert f["widest"] <= WINDOW_LIMIT, "%s: a window of %d candidates" % (case, f["widest"])


@pytest.mark.parametrize("pair", ["1", "0"])
def test_pair_units_emulated(emu_lib, monkeypatch, pair_units, pair):
    monkeypatch.setenv("TW_TILE_PAIR", pair)
    parity.check_units(emu_lib, pair_units)


@pytest.mark.parametrize("pair", ["1", "0"])
def test_pair_units_emulated_with_production_tables(emu_prod_lib, monkeypatch, pair_units, pair):
    """The spans of 33 to 256 tuples by the tile kernel itself, a thread per workgroup."""
    monkeypatch.setenv("TW_TILE_PAIR", pair)
    parity.check_units(emu_prod_lib, pair_units)


@pytest.mark.parametrize("pair", ["1", "0"])
def test_mixed_batch_emulated(emu_lib, monkeypatch, pair):
    monkeypatch.setenv("TW_TILE_PAIR", pair)
    units, _ = parity.stress_units(MIXED)
    parity.check_units(emu_lib, units)


_LANES = (
    "import sys, os\n"
    "sys.path[:0] = [%r, %r, %r]\n"
    "import parity\n"
    "units, _ = parity.stress_units([(302, 300, 'par2', 4, 1000), (303, 400, 'par2', 8, 1000), (313, 400, 'chain2', 12, 1)])\n"
    "parity.check_units(%r, units)\n"
    "print('lanes ok')\n"
)


def test_lane_threaded_pair_path_with_production_tables():
    """The pair path by a host thread per lane, 256 to a tile of 128 requests, with the table sizes of the HIP build: the block-wide
    prefix sums, the items and slots named by their spans' threads, the maxima through atomics, the wavefronts' appends to the
    survivor lists, replays across the lanes, several segments per tile (case 303), sub-tile workgroups (TW_TILE_SUB=2) -- and the
    general path on the same units."""
    from tests.hostemu.build_emu import build

    code = _LANES % (REPO, HERE, os.path.join(REPO, "oracle"), build(production=True))
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256", TW_TILE_SUB="2")
    # (the two routes side by side, a process each: the test is as long as the slower one)
    runs = [subprocess.Popen([sys.executable, "-c", code], env=dict(env, TW_TILE_PAIR=v), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for v in ("1", "0")]
    for v, p in zip(("1", "0"), runs):
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0 and "lanes ok" in out, "TW_TILE_PAIR=%s: %s" % (v, err[-2000:])


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["1", "0"])
def test_pair_units_on_the_gpu(monkeypatch, pair_units, pair):
    monkeypatch.setenv("TW_TILE_PAIR", pair)
    parity.check_units(None, pair_units)


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
    "units = [synth.make_unit(401 + k, 20000, shape=s, concurrency=c, granularity_us=g)[0]\n"
    "         for k, (s, c, g) in enumerate([('par2', 1.6, 1), ('par2', 8, 1000), ('chain2', 4, 1), ('chain2', 12, 1)])]\n"
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
    """Four two-endpoint units of 20 000 requests (par2 at concurrency 1.6 and at 8 millisecond-granular, chain2 at 4 and at 12),
    solved in fresh child processes on the pair path and on the general one: all of results(1) and results(2) are equal."""
    import pickle

    got = []
    for v in ("1", "0"):
        out = str(tmp_path / ("route%s.pkl" % v))
        p = subprocess.run([sys.executable, "-c", _AB % REPO, out], env=dict(os.environ, TW_TILE_PAIR=v), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        with open(out, "rb") as f:
            got.append(pickle.load(f))
    for a, b in zip(got[0][0] + got[0][1], got[1][0] + got[1][1]):
        _assert_same(a, b)
