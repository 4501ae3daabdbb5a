"""Baseline predictors (traceweaver_amd/baselines.py) against the reference's own classes: same inputs -> identical
assignments.  What the reference's FCFS, ArrivalOrder, vPath and WAP5 returned for every input below is stored in
tests/golden/baseline_refs.npz (tests/golden/make_baseline_refs.py runs the reference's classes on the same inputs)."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO
from traceweaver_amd import baselines, synth
from traceweaver_amd.ingest import Corpus, REFERENCE_FIX

REF_OUT = os.path.join(REPO, "tests", "golden", "baseline_refs.npz")


class Span(object):
    """The attributes the baseline classes read (reference spans.py:1-75)."""

    def __init__(self, trace_id, sid, start, dur, kind):
        # after the executor's load scaling start_mus is a float (helpers/transforms.py:21,30); durations stay ints
        self.trace_id, self.sid, self.duration_mus, self.span_kind = trace_id, sid, int(dur), kind
        self.start_mus = float(start) if isinstance(start, float) else int(start)

    def GetId(self):
        return (self.trace_id, self.sid)


def reference_classes(ref_py):
    """FCFS, ArrivalOrder, vPath, WAP5 of the reference tree's python port (tests/golden/make_baseline_refs.py only)."""
    saved = list(sys.path)
    sys.path.insert(0, ref_py)
    try:
        from algorithms.arrival_order import ArrivalOrder
        from algorithms.fcfs import FCFS
        from algorithms.vpath import vPath
        from algorithms.wap5 import WAP5
    finally:
        sys.path[:] = saved
    return FCFS, ArrivalOrder, vPath, WAP5


def protocol_inputs(u, trace_of_in, trace_of_out):
    """Partitions in partition-key order, as the executor hands them to a predictor."""
    a = u.arrays
    if a.time_scale is None:
        i_s, i_d, o_s, o_d = a.in_start, a.in_end - a.in_start, a.out_start, a.out_end - a.out_start
    else:   # a load-scaled unit: the float starts it is the exact image of, the integer durations
        i_s, o_s = a.in_start * a.time_scale, a.out_start * a.time_scale
        i_d, o_d = np.rint((a.in_end - a.in_start) * a.time_scale), np.rint((a.out_end - a.out_start) * a.time_scale)
        assert np.array_equal(i_s + i_d, a.in_end * a.time_scale) and np.array_equal(o_s + o_d, a.out_end * a.time_scale)
    in_spans = [Span(trace_of_in[i], "in%d" % i, i_s[i], i_d[i], "server") for i in range(a.n_in)]
    parts, keys = {}, [int(k) for k in np.argsort(a.key_rank, kind="stable")]
    for e in keys:
        o0, o1 = int(a.out_off[e]), int(a.out_off[e + 1])
        parts[u.out_eps[e]] = [Span(trace_of_out[e][j], "o%d_%d" % (e, j), o_s[o0 + j], o_d[o0 + j], "client")
                               for j in range(o1 - o0)]
    truth = {u.out_eps[e]: {in_spans[i].GetId(): parts[u.out_eps[e]][u.true_parent[e, i]].GetId() for i in range(a.n_in)} for e in keys}
    return {u.in_ep: in_spans}, parts, truth


def to_parent(u, asg, in_parts, parts):
    in_spans = list(in_parts.values())[0]
    out = np.full((u.arrays.E, u.arrays.n_in), -1, dtype=np.int32)
    for e, ep in enumerate(u.out_eps):
        pos = {s.GetId(): j for j, s in enumerate(parts[ep])}
        for i, s in enumerate(in_spans):
            v = asg[ep][s.GetId()]
            out[e, i] = pos[v] if v != ("NA", "NA") else -1
    return out


def _unit_traces(u, wap5):
    a = u.arrays
    trace_in = ["t%d" % k for k in u.in_trace]
    if wap5:
        trace_out = [["x%d_%d" % (e, j) for j in range(int(a.out_off[e + 1] - a.out_off[e]))] for e in range(a.E)]
    else:
        trace_out = [["t%d" % u.in_trace[np.flatnonzero(u.true_parent[e] == j)[0]] if (u.true_parent[e] == j).any() else "x%d_%d" % (e, j)
                      for j in range(int(a.out_off[e + 1] - a.out_off[e]))] for e in range(a.E)]
    return trace_in, trace_out


def run_reference(units, classes, parents=True, wap5=True):
    """The reference's classes on the units, in the protocol the executor uses: {key: array} as stored in baseline_refs.npz --
    "<k>/<name>" the parent array [E, n_in] of FCFS / ArrivalOrder / vPath for unit k, "<k>/WAP5/<e>/calls" and "<k>/WAP5/<e>/off"
    the calls WAP5 gave every request of endpoint e (one WAP5 instance fed the units in order: state leaks between services)."""
    import copy

    FCFS, ArrivalOrder, vPath, WAP5 = classes
    out, w = {}, WAP5({}, {})
    for k, u in enumerate(units):
        in_parts, parts, truth = protocol_inputs(u, *_unit_traces(u, False))
        for name, cls in (("FCFS", FCFS), ("ArrivalOrder", ArrivalOrder), ("vPath", vPath)) if parents else ():
            ref = cls({}, {}).FindAssignments(name, u.service, copy.deepcopy(in_parts), copy.deepcopy(parts), False, [], truth)
            out["%d/%s" % (k, name)] = to_parent(u, ref, in_parts, parts)
        if not wap5:
            continue
        in_parts, parts, truth = protocol_inputs(u, *_unit_traces(u, True))
        got = w.FindAssignments("WAP5", u.service, copy.deepcopy(in_parts), copy.deepcopy(parts), False, [], truth)
        in_spans = list(in_parts.values())[0]
        for e, ep in enumerate(u.out_eps):
            pos = {s.GetId(): j for j, s in enumerate(parts[ep])}
            calls = [[pos[x] for x in got[ep][s.GetId()] if tuple(x) != ("NA", "NA")] for s in in_spans]
            out["%d/WAP5/%d/calls" % (k, e)] = np.array([j for c in calls for j in c], dtype=np.int32)
            out["%d/WAP5/%d/off" % (k, e)] = np.cumsum([0] + [len(c) for c in calls]).astype(np.int32)
    return out


def stored(case):
    with np.load(REF_OUT) as d:
        return {k[len(case) + 1:]: d[k] for k in d.files if k.startswith(case + "/")}


def check_units(units, case):
    ref = stored(case)
    assert ref, case
    for k, u in enumerate(units):
        a = u.arrays
        for name, mine in (("FCFS", baselines.fcfs(a)), ("ArrivalOrder", baselines.arrival_order(a)), ("vPath", baselines.vpath(a, u.true_parent))):
            assert np.array_equal(ref["%d/%s" % (k, name)], mine), (u.service, name)


def check_wap5(units, case):
    """One reference instance and one of ours, fed the services in the same order (state leaks between services)."""
    ref, mine = stored(case), baselines.WAP5()
    assert ref, case
    for k, u in enumerate(units):
        options = mine.assign(u.arrays, u.out_eps)
        for e, ep in enumerate(u.out_eps):
            calls, off = ref["%d/WAP5/%d/calls" % (k, e)], ref["%d/WAP5/%d/off" % (k, e)]
            assert len(off) == u.arrays.n_in + 1, (u.service, ep)
            for i in range(u.arrays.n_in):
                assert options[e][i] == calls[off[i]:off[i + 1]].tolist(), (u.service, ep, i)


# the inputs: (case, how its units are made) -- shared with tests/golden/make_baseline_refs.py
def generated_units(lib, directory, app, seed, traces, concurrency):
    synth.write_jaeger_corpus(str(directory), seed, traces, app=app, concurrency=concurrency)
    c = Corpus(lib_path=lib)
    c.add_directory(str(directory), first_span=app["root_op"], max_traces=0)
    units = c.units()[0]
    c.close()
    return units


def corpus_units(lib, root, rel, fix):
    first, surgery = REFERENCE_FIX[fix]
    c = Corpus(lib_path=lib)
    c.add_directory(os.path.join(root, "data", rel), first_span=first, max_traces=1001, fix=surgery)
    units = c.units()[0]
    c.close()
    return units


GENERATED = [("gen_wap5", synth.HOTEL_APP, 23, 300, 2.0), ("gen_hotel", synth.HOTEL_APP, 21, 250, 2.5), ("gen_fanout", synth.FANOUT_APP, 21, 250, 1.6)]
WAP5_CORPORA = [("hotel_reservation/hotel_load100", 2), ("nodejs_microservices/node_load150", 0)]
BASELINE_CORPORA = [("hotel_reservation/hotel_load150", 2), ("nodejs_microservices_with_arbitrary_file_io/node_1", 0),
                    ("media_microservices/media_load100", 1)]
SCALED = [3, 7]


def _gen(case):
    return next(g for g in GENERATED if g[0] == case)[1:]


def test_wap5_on_generated_corpora(emu_lib, tmp_path):
    check_wap5(generated_units(emu_lib, tmp_path, *_gen("gen_wap5")), "gen_wap5")


@pytest.mark.parametrize("rel,fix", WAP5_CORPORA)
def test_wap5_on_reference_corpora(emu_lib, reference_root, rel, fix):
    check_wap5(corpus_units(emu_lib, reference_root, rel, fix), rel)


def test_baselines_on_generated_corpora(emu_lib, tmp_path):
    for case in ("gen_hotel", "gen_fanout"):
        check_units(generated_units(emu_lib, tmp_path / case, *_gen(case)), case)


@pytest.mark.parametrize("rel,fix", BASELINE_CORPORA)
def test_baselines_on_reference_corpora(emu_lib, reference_root, rel, fix):
    check_units(corpus_units(emu_lib, reference_root, rel, fix), rel)


def _scaled(units, factor):
    """The units after the executor's load scaling (traceweaver_amd/transforms.py)."""
    from traceweaver_amd import transforms
    from traceweaver_amd.ingest import IngestedUnit

    out = []
    for u in units:
        s = transforms.compress_unit(u.arrays, u.true_parent, factor, trace_key=["t%d" % k for k in u.in_trace])
        out.append(IngestedUnit(s.arrays, s.true_parent, u.in_trace[s.in_perm], u.service, u.in_ep, u.out_eps, u.in_rows[s.in_perm],
                                [r[p] for r, p in zip(u.out_rows, s.out_perm)], u.process_id))
    return out


def scaled_units(lib, directory, factor):
    return _scaled(generated_units(lib, directory, synth.HOTEL_APP, 29, 300, 1.2), factor)


@pytest.mark.parametrize("factor", SCALED)
def test_baselines_on_load_scaled_units(emu_lib, tmp_path, factor):
    """--compress_factor > 1 hands the reference's classes float timestamps; ours read the exact integer image of them."""
    units = scaled_units(emu_lib, tmp_path, factor)
    assert all(u.arrays.time_scale < 1.0 for u in units)
    check_units(units, "scaled_%d" % factor)
    check_wap5(units, "scaled_%d" % factor)
