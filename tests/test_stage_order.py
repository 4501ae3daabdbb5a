"""The order in which the per-class streams of a staged pass meet: the stage gate (TW_STAGE_GATE).  The classes other
than the critical one -- the deepest class, where the general path of the tile kernel serves it -- hold the persistent part of their
stage until the critical class' tile kernel has ended.  Only the launch order changes, so a staged batch of alternating classes is
held to the oracle bit for bit with the gate as built and with TW_STAGE_GATE=0: one batch that needs no repair, one in which repair
rounds occur (those run joined and ungated behind the gated stages).

The knobs are read once in tw_create: every engine here is created with the environment it is to see.  The CPU tier runs the
host-emulation build (a thread per workgroup; the streams run in submission order there: what it checks is that both settings queue a
complete pass), the GPU tier the HIP library, where the event orders real streams -- the small batches, and units of 20 000 to
100 000 requests, where the tile kernel of the deepest class fills the CUs while the other classes' persistent selection launches are
held behind it.  Engine.gated_stages says how many class stages of a pass were queued behind the gate: the tests assert that the
gated path was taken where it should be, and only there."""
import os

import pytest

import parity
from traceweaver_amd.engine import Engine

# (seed, n_in, shape, concurrency, granularity_us), the classes interleaved: one, four, two, two, one and four endpoints -- the deepest
# class has four, so the gate applies.  QUIET: 1.6 requests in flight, microseconds -- no unit needs a repair round in either pass.
# BUSY: 4 in flight on millisecond timestamps -- 710, 701, 702 and 705 each go through a repair round in both passes.  (Seeds 700..
# looked at on the CPU tier; the oracle takes well under a second for each.)
QUIET = [(700, 320, "single", 1.6, 1), (701, 300, "par4", 1.6, 1), (702, 330, "par2", 1.6, 1), (703, 310, "chain2", 1.6, 1),
         (704, 400, "single", 1.6, 1), (705, 340, "par4", 1.6, 1)]
BUSY = [(710, 320, "single", 4, 1000), (701, 320, "par4", 4, 1000), (702, 320, "par2", 4, 1000), (703, 320, "chain2", 4, 1000),
        (704, 320, "single", 4, 1000), (705, 320, "par4", 4, 1000)]
GATES = ("1", "0")   # the gate as built (behind k_select_fast) and the A/B switch
# the GPU tier's sizes (those of test_runs_from_the_hash_table_equal_runs_from_the_sort_on_gpu): 470 + 157 + 782 tiles; the deepest class,
# three endpoints, is on the general path of the tile kernel, so the stages of the other two are gated
LARGE = [(47, 60000, "par2", 2, 1), (48, 20000, "chain3", 2, 1000), (49, 100000, "single", 1.6, 1)]


class _Env(object):
    """The environment an engine is created in (and nothing left behind); every batch here is staged."""

    def __init__(self, **kv):
        self.kv = dict(kv, TW_STAGE_MIN_TILES="1")

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check_with_rounds(lib_path, units, monkeypatch):
    """parity.check_units; the repair rounds of the two passes it ran and the class stages each queued behind the gate."""
    rounds, gated = [], []

    class Recording(Engine):
        def run_pass1(self):
            Engine.run_pass1(self)
            rounds.append(int(self.timing()["rounds"]))
            gated.append(self.gated_stages())

        def run_pass2(self):
            Engine.run_pass2(self)
            rounds.append(int(self.timing()["rounds"]))
            gated.append(self.gated_stages())

    with monkeypatch.context() as m:
        m.setattr(parity, "Engine", Recording)
        parity.check_units(lib_path, units)
    return rounds, gated


def _gate_cases(lib_path, monkeypatch):
    quiet, _ = parity.stress_units(QUIET)
    busy, _ = parity.stress_units(BUSY)
    for gate in GATES:
        with _Env(TW_STAGE_GATE=gate):
            rq, gq = _check_with_rounds(lib_path, quiet, monkeypatch)
            rb, gb = _check_with_rounds(lib_path, busy, monkeypatch)
        print("TW_STAGE_GATE=%s: repair rounds (pass 1, pass 2) quiet %s, busy %s; gated stages %s, %s" % (gate, rq, rb, gq, gb))
        # the classes of one and of two endpoints wait for the tile kernel of the four-endpoint class, in both passes -- or nothing does
        assert gq == gb == ([2, 2] if gate == "1" else [0, 0]), (gate, gq, gb)
        assert rq == [0, 0], (gate, rq)              # conditions on the inputs: the stages' results are the passes' results ...
        assert rb[0] > 0 and rb[1] > 0, (gate, rb)   # ... and here they are not


def test_staged_alternating_classes_equal_the_oracle_gated_and_ungated(emu_lib, oracle, monkeypatch):
    _gate_cases(emu_lib, monkeypatch)


def test_batches_the_rule_leaves_ungated(emu_lib, oracle, monkeypatch):
    """The deepest class on the pair path of the tile kernel (the nodejs shape's classes), and a batch that is not staged."""
    units, _ = parity.stress_units(QUIET[2:5])
    with _Env(TW_STAGE_GATE="1"):
        assert _check_with_rounds(emu_lib, units, monkeypatch)[1] == [0, 0]
    quiet, _ = parity.stress_units(QUIET[:3])
    with _Env(TW_STAGE_GATE="1", TW_CLASS_PIPELINE="0"):
        assert _check_with_rounds(emu_lib, quiet, monkeypatch)[1] == [0, 0]


@pytest.mark.gpu
def test_staged_alternating_classes_equal_the_oracle_gated_and_ungated_on_gpu(oracle, monkeypatch):
    _gate_cases(None, monkeypatch)


@pytest.mark.gpu
def test_large_units_equal_the_oracle_gated_and_ungated_on_gpu(oracle, monkeypatch):
    units, _ = parity.stress_units(LARGE)
    for gate in GATES:
        with _Env(TW_STAGE_GATE=gate):
            rounds, gated = _check_with_rounds(None, units, monkeypatch)
        print("TW_STAGE_GATE=%s: repair rounds %s, gated stages %s" % (gate, rounds, gated))
        assert gated == ([2, 2] if gate == "1" else [0, 0]), (gate, gated)
