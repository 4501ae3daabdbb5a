"""The single-endpoint path of k_enumerate_tile (traceweaver_amd/csrc/tw_tile.h, SINGLE): a tuple is an item -- one prefix sum, one
score table, the rank counted among the span's own items, undecided spans replayed by their own thread.  Every unit goes through
parity.check_units (both passes against the oracle bit for bit: lists, scores, leaves, windows, selection, parents, gap samples,
Gaussian parameters), on the lean path and with TW_TILE_SINGLE=0 on the general one.  CPU tier: the host-emulation build, one
lane-threaded run with the production tables; the HIP library under -m gpu."""
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
    (101, 300, "single", 1.6, 1): (),                                        # the bench's own regime: 1.5 candidates a span
    (102, 300, "single", 4, 1000): ("twins",),                               # equal starts: phase 5b
    (103, 400, "single", 12, 1000): ("twins", "more_than_five", "wider_32"),
    (104, 400, "single", 24, 1): ("exactly_32", "wider_32", "several_segments"),
    (106, 257, "single", 8, 1000): ("two_tiles_and_one",),
    (109, 2, "single", 1, 1): (),                                            # the smallest legal unit
}
MIXED = [(101, 300, "single", 1.6, 1), (7, 300, "par4", 3, 1), (102, 300, "single", 4, 1000), (4, 300, "par2", 6, 1),
         (103, 400, "single", 12, 1000), (7, 300, "par4", 3, 1), (104, 400, "single", 24, 1), (4, 300, "par2", 6, 1),
         (106, 257, "single", 8, 1000), (7, 300, "par4", 3, 1), (109, 2, "single", 1, 1), (4, 300, "par2", 6, 1)]
TILE, TILE_ITEMS, WINDOW_LIMIT = 128, 768, 128   # kTile, TW_TILE_ITEMS, 64 * kCandWords of the HIP build


def _facts(u):
    """Recomputed from the inputs alone (FindCutoffs and the containment test of a single endpoint)."""
    assert u.E == 1
    os_, oe = np.asarray(u.out_start), np.asarray(u.out_end)
    lo = np.searchsorted(os_, u.in_start, side="left")
    hi = np.searchsorted(os_, u.in_end, side="right")   # one past the window
    width = hi - lo
    contained = np.zeros(u.n_in, np.int64)
    twins = np.zeros(u.n_in, bool)
    for i in range(u.n_in):
        w = np.arange(lo[i], hi[i])
        c = w[(os_[w] >= u.in_start[i]) & (oe[w] <= u.in_end[i])]
        contained[i] = len(c)
        twins[i] = len(c) > 1 and bool((np.diff(os_[c]) == 0).any())
    per_tile = np.add.reduceat(contained, np.arange(0, u.n_in, TILE))
    return {
        "twins": int(twins.sum()) >= 1,
        "more_than_five": int((contained > 5).sum()) >= 1,
        "exactly_32": int((width == 32).sum()) >= 1,
        "wider_32": int((width > 32).sum()) >= 1,
        "several_segments": int(per_tile.max()) > TILE_ITEMS,
        "two_tiles_and_one": u.n_in == 2 * TILE + 1,
        "widest": int(width.max()),
    }


@pytest.fixture(scope="module")
def single_units():
    units, _ = parity.stress_units(list(CASES))
    return units


def test_units_hold_what_their_cases_are_for(single_units):
    for case, u in zip(CASES, single_units):
        f = _facts(u)
        for need in CASES[case]:
            assert f[need], "%s: no %s" % (case, need)
        assert f["widest"] <= WINDOW_LIMIT, "%s: a window of %d candidates" % (case, f["widest"])


@pytest.mark.parametrize("single", ["1", "0"])
def test_single_units_emulated(emu_lib, monkeypatch, single_units, single):
    monkeypatch.setenv("TW_TILE_SINGLE", single)
    parity.check_units(emu_lib, single_units)


@pytest.mark.parametrize("single", ["1", "0"])
def test_mixed_batch_emulated(emu_lib, monkeypatch, single):
    monkeypatch.setenv("TW_TILE_SINGLE", single)
    units, _ = parity.stress_units(MIXED)
    parity.check_units(emu_lib, units)


_LANES = (
    "import sys, os\n"
    "sys.path[:0] = [%r, %r, %r]\n"
    "import parity\n"
    "units, _ = parity.stress_units([(102, 300, 'single', 4, 1000), (104, 400, 'single', 24, 1), (106, 257, 'single', 8, 1000)])\n"
    "parity.check_units(%r, units)\n"
    "print('lanes ok')\n"
)


def test_lane_threaded_single_path_with_production_tables():
    """The single-endpoint path by a host thread per request of a tile of 128 with the table sizes of the HIP build: the block-wide
    prefix sum, the items named by their spans' threads, ranks and replays across the lanes, several segments per tile (case 104),
    sub-tile workgroups (TW_TILE_SUB=2) -- and the general path (256 threads per tile) on the same units."""
    from tests.hostemu.build_emu import build

    code = _LANES % (REPO, HERE, os.path.join(REPO, "oracle"), build(production=True))
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256", TW_TILE_SUB="2")
    # (the two routes side by side, a process each: the test is as long as the slower one)
    runs = [subprocess.Popen([sys.executable, "-c", code], env=dict(env, TW_TILE_SINGLE=v), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for v in ("1", "0")]
    for v, p in zip(("1", "0"), runs):
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0 and "lanes ok" in out, "TW_TILE_SINGLE=%s: %s" % (v, err[-2000:])


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_single_units_on_the_gpu(single_units):
    parity.check_units(None, single_units)


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
    "units = [synth.make_unit(201 + k, 20000, shape='single', concurrency=c, granularity_us=g)[0]\n"
    "         for k, (c, g) in enumerate([(1.6, 1), (4, 1), (8, 1000), (12, 1)])]\n"
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
    """Four single-endpoint units of 20 000 requests (concurrency 1.6 / 4 / 8 millisecond-granular / 12), solved in fresh child
    processes on the lean path and on the general one: all of results(1) and results(2) are equal."""
    import pickle

    got = []
    for v in ("1", "0"):
        out = str(tmp_path / ("route%s.pkl" % v))
        p = subprocess.run([sys.executable, "-c", _AB % REPO, out], env=dict(os.environ, TW_TILE_SINGLE=v), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        with open(out, "rb") as f:
            got.append(pickle.load(f))
    for a, b in zip(got[0][0] + got[0][1], got[1][0] + got[1][1]):
        _assert_same(a, b)
