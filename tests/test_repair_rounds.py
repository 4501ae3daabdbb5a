"""The repair rounds of the span consumption (k_claim, k_detect_gone, the mode-1 enumeration on the remaining spans, the
listed windows solved again) on units that are nearly all repair: most windows hold a request whose list on the remaining spans is not
its list on all spans.  Every unit goes through parity.check_units, which holds both passes to the oracle bit for bit -- since this
file exists also the lists the selection read (Engine.decisions against the oracle's lists on the remaining spans).  What a case is
for is proven from the oracle alone (_facts).

CPU tier: the host-emulation builds a thread per workgroup (the tiny tables; the production tables, where the wide spans of the first
solve are on the wavefront kernel's wide list -- the configuration in which a class' first repair round enumerated them again on
invalid words of P.gone until reset_class_lists reset all of the lists with fewer than eight threads: profiles/HISTORY.md), one
lane-threaded run with the production tables, and a sweep of 80 further units.  The HIP library under -m gpu."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import parity

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# (seed, n_in, shape, concurrency, granularity_us): 257 to 400 requests, three tiles of 128 with windows across the tile borders, 12 to
# 24 requests in flight.  Picked by their facts among seeds 501.. of single / par2 / chain2 / chain3 (and 314 of tests/test_tile_pair.py)
# with an oracle run of under a second each.  (par4 at these loads: the oracle's own search takes 3 to 80 s a unit -- left out; chain3 at
# 400 requests, (545, 400, "chain3", 24, 1), is identical to the oracle on every tier too but takes the lane-threaded emulation nine
# minutes: the smaller chain3 unit stands for the shape.)
CASES = [
    (314, 400, "chain2", 24, 1), (506, 400, "single", 12, 1000), (510, 257, "single", 24, 1000), (512, 400, "single", 24, 1000),
    (516, 257, "par2", 12, 1000), (520, 300, "par2", 24, 1), (533, 400, "chain2", 24, 1), (543, 257, "chain3", 24, 1),
    (532, 300, "chain2", 24, 1),
]

# The sweep: seeds 0..39 of chain2 at 300 requests and of par2 at 100, 24 requests in flight, 1 us.  (par2 at 300 requests: the oracle's
# selection search alone takes minutes over the 40 units; at 100 the whole sweep takes half a minute.)  Seeds on which the oracle's own
# search runs out of its node budget are replaced by the next that do not: par2 2, 15, 32 by 40, 41, 42 (three of the four allowed).
SWEEP_REPLACED = {"par2": {2: 40, 15: 41, 32: 42}, "chain2": {}}
SWEEP_REQUESTS = {"chain2": 300, "par2": 100}
SWEEP = [(SWEEP_REPLACED[shape].get(seed, seed), SWEEP_REQUESTS[shape], shape, 24, 1) for shape in ("chain2", "par2") for seed in range(40)]


def _differs(p):
    """Per request: its list on the remaining spans (topk_*) is not its list on all spans (topk2_*)."""
    return (p["topk_n"] != p["topk2_n"]) | (p["topk_idx"] != p["topk2_idx"]).any(axis=(1, 2))


def _facts(end_flag, p1, p2):
    """From the oracle's two passes alone."""
    ends = np.nonzero(np.asarray(end_flag))[0]
    first = np.concatenate(([0], ends[:-1] + 1))
    d1, d2 = _differs(p1), _differs(p2)
    repaired = sum(bool(d2[a:b + 1].any()) for a, b in zip(first.tolist(), ends.tolist()))
    return {
        "windows": len(ends), "repaired_windows": repaired, "longest_window": int((ends - first + 1).max()),
        "shorter": int(sum(((p["topk_n"] < p["topk2_n"]) & (p["topk_n"] > 0)).sum() for p in (p1, p2))),
        "empty": int(sum(((p["topk_n"] == 0) & (p["topk2_n"] > 0)).sum() for p in (p1, p2))),
        "pass2_only": int((d2 & ~d1).sum()),
        "budget_windows": int(p1["budget_windows"] + p2["budget_windows"]),
    }


@pytest.fixture(scope="module")
def repair_units():
    units, _ = parity.stress_units(CASES)
    return units


@pytest.fixture(scope="module")
def repair_facts(repair_units, oracle):
    return [_facts(*parity.oracle_two_pass(parity.oracle_service(u))[:3]) for u in repair_units]


@pytest.fixture(scope="module")
def emu_prod_lib(emu_lib):
    """The emulation build with the table sizes of the HIP build, a thread per workgroup as emu_lib sets it up."""
    from tests.hostemu.build_emu import build

    return build(production=True)


def test_units_hold_what_their_cases_are_for(repair_facts):
    for case, f in zip(CASES, repair_facts):
        print(case, f)
        assert f["budget_windows"] == 0, case
        assert 2 * f["repaired_windows"] >= f["windows"], "%s: %d of %d windows hold a request with a list of its own on the remaining spans" % (case, f["repaired_windows"], f["windows"])
        assert f["longest_window"] > 16, case
    assert any(f["shorter"] > 0 for f in repair_facts)       # a list on the remaining spans with fewer entries than the list on all spans
    assert any(f["empty"] > 0 for f in repair_facts)         # ... empty, while the list on all spans is not
    assert any(f["pass2_only"] > 0 for f in repair_facts)    # a request whose list differs in pass 2 but not in pass 1


def test_repair_units_emulated(emu_lib, repair_units):
    r1, r2, _ = parity.check_units(emu_lib, repair_units)
    assert all(r["repaired_windows"] > 0 for r in r1 + r2)


def test_repair_units_emulated_with_production_tables(emu_prod_lib, repair_units):
    r1, r2, _ = parity.check_units(emu_prod_lib, repair_units)
    assert all(r["repaired_windows"] > 0 for r in r1 + r2)


_LANES = (
    "import sys, os\n"
    "sys.path[:0] = [%r, %r, %r]\n"
    "import parity\n"
    "units, _ = parity.stress_units(%r)\n"
    "parity.check_units(%r, units)\n"
    "print('lanes ok')\n"
)


def test_lane_threaded_repair_with_production_tables(repair_facts):
    """The three units with the most repaired windows by a host thread per lane, 128 requests to a tile, with the table sizes of the HIP
    build: the workgroups of the GPU's own configuration, windows across the tile borders."""
    from tests.hostemu.build_emu import build

    most = sorted(range(len(CASES)), key=lambda k: -repair_facts[k]["repaired_windows"])[:3]
    lib = build(production=True)
    env = dict(os.environ, TW_EMU_LANES="1", TW_TILE="128", TW_COOP_THREADS="256", TW_TILE_SUB="2")
    # (a process per unit, side by side: the test is as long as the slowest)
    runs = [subprocess.Popen([sys.executable, "-c", _LANES % (REPO, HERE, os.path.join(REPO, "oracle"), [CASES[k]], lib)], env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k in most]
    for k, p in zip(most, runs):
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0 and "lanes ok" in out, "%s: %s" % (CASES[k], err[-2000:])


def test_sweep_emulated_with_production_tables(emu_prod_lib, oracle):
    """80 units, each held to the oracle on its own (no allow_budget); their repaired windows are counted."""
    t0 = time.time()
    assert len(SWEEP) == len(set(SWEEP)) == 80 and sum(len(v) for v in SWEEP_REPLACED.values()) <= 4
    repaired = 0
    for case in SWEEP:
        units, _ = parity.stress_units([case])
        try:
            r1, r2, ora = parity.check_units(emu_prod_lib, units)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (case, e)) from e
        assert ora[0][2]["budget_windows"] == 0 and ora[0][3]["budget_windows"] == 0, case
        repaired += r1[0]["repaired_windows"] + r2[0]["repaired_windows"]
    print("sweep: %d units, %d repaired windows, %.1f s" % (len(SWEEP), repaired, time.time() - t0))
    assert repaired > 0


def test_emulation_refuses_workgroups_of_several_threads_without_lanes(emu_lib, monkeypatch):
    """Without the environment of the emu_lib fixture (or with a tile of several threads) and no TW_EMU_LANES=1 the emulation library
    is refused with an error -- it used to run and end the process in pass 1."""
    from traceweaver_amd.engine import Engine, EngineError

    for unset, setting in ((("TW_TILE", "TW_COOP_THREADS"), {}), ((), {"TW_TILE": "128"}), ((), {"TW_COOP_THREADS": "64"})):
        with monkeypatch.context() as m:
            m.delenv("TW_EMU_LANES", raising=False)
            for k in unset:
                m.delenv(k, raising=False)
            for k, v in setting.items():
                m.setenv(k, v)
            with pytest.raises(EngineError) as ex:
                Engine(0, lib_path=emu_lib)
            assert ex.value.code == -3
    Engine(0, lib_path=emu_lib).close()


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_repair_units_on_the_gpu_twice(repair_units):
    a1, a2, _ = parity.check_units(None, repair_units)
    b1, b2, _ = parity.check_units(None, repair_units)
    assert all(r["repaired_windows"] > 0 for r in a1 + a2)
    for x, y in zip(a1 + a2, b1 + b2):
        assert sorted(x) == sorted(y)
        for k in x:
            if isinstance(x[k], np.ndarray):
                assert np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == "f"), k
            else:
                assert x[k] == y[k], k
