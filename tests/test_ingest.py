"""Native Jaeger-JSON ingest (csrc/tw_ingest.cpp) against (a) a plain-Python restatement of what
the reference's executor does between reading a directory and calling the predictor (executor.py:287-339,
755-849,1080-1135; helpers/utils.py:22-32) on generated corpora, and (b) the inputs frozen from the reference
itself for every shipped corpus (tests/golden/ref_*; the JSON files from tests/golden/corpus_*.tar.xz)."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from traceweaver_amd import synth
from traceweaver_amd.engine import Engine
from traceweaver_amd.ingest import Corpus

def python_pipeline(paths, first_span, max_traces=1001):
    """The reference's loader restated with dicts and lists (no span rewriting)."""
    starts, docs = [], []
    for p in paths:
        d = json.load(open(p))["data"][0]
        docs.append(d)
        root = next((s for s in d["spans"] if len(s["references"]) == 0), None)
        starts.append(float(root["startTime"]) if root else float("inf"))
    order = sorted(range(len(paths)), key=lambda i: (starts[i], i))
    ins, outs, spans_all, service_of, cnt = {}, {}, {}, {}, 0
    for i in order:
        d = docs[i]
        tid = d["traceID"]
        procs = {k: v["serviceName"] for k, v in d["processes"].items()}
        spans = {}
        for s in d["spans"]:
            kind = [t["value"] for t in s["tags"] if t["key"] == "span.kind"][0]
            spans[s["spanID"]] = dict(sid=s["spanID"], tid=tid, start=s["startTime"], dur=s["duration"], op=s["operationName"],
                                      refs=[r["spanID"] for r in s["references"]], svc=procs[s["processID"]], kind=kind, children=[])
        root = None
        for s in spans.values():
            if not s["refs"]:
                root = s
            for r in s["refs"]:
                spans[r]["children"].append(s["sid"])
        for s in spans.values():
            s["children"].sort(key=lambda c: spans[c]["start"])
        if first_span and root["op"] != first_span:
            continue

        def walk(s):
            (outs if s["kind"] == "client" else ins).setdefault(s["svc"], []).append(s)
            for c in s["children"]:
                walk(spans[c])
        walk(root)
        spans_all.update({(tid, k): v for k, v in spans.items()})
        cnt += 1
        if cnt >= max_traces:
            break
    units = {}
    for svc in outs:
        def parts(lst, key):
            out = {}
            for s in lst:
                out.setdefault(key(s), []).append(s)
            for v in out.values():
                v.sort(key=lambda x: (x["start"], x["start"] + x["dur"]))
            return out
        ip = parts(ins[svc], lambda s: ("client_" + s["op"]) if not s["refs"] else spans_all[(s["tid"], s["refs"][0])]["svc"])
        op = parts(outs[svc], lambda s: spans_all[(s["tid"], s["children"][0])]["svc"])
        if len(ip) != 1:
            continue
        in_ep, in_spans = list(ip.items())[0]
        keys = list(op.keys())
        truth = {k: [next((j for j, o in enumerate(op[k]) if o["tid"] == s["tid"]), -1) for s in in_spans] for k in keys}
        E = len(keys)
        rel = np.ones((E, E), np.uint8) - np.eye(E, dtype=np.uint8)
        for i in range(len(in_spans)):
            for a in range(E):
                for b in range(E):
                    if a != b:
                        x, y = op[keys[a]][truth[keys[a]][i]], op[keys[b]][truth[keys[b]][i]]
                        if x["start"] + x["dur"] > y["start"]:
                            rel[a, b] = 0
        topo = synth.topo_order(rel)
        units[svc] = dict(in_ep=in_ep, out_eps=[keys[a] for a in topo], key_rank=topo,
                          in_start=np.array([s["start"] for s in in_spans]), in_end=np.array([s["start"] + s["dur"] for s in in_spans]),
                          out_start=np.concatenate([[o["start"] for o in op[keys[a]]] for a in topo]),
                          out_end=np.concatenate([[o["start"] + o["dur"] for o in op[keys[a]]] for a in topo]),
                          dag=rel[np.ix_(topo, topo)], truth=np.array([truth[keys[a]] for a in topo]),
                          in_ids=[(s["tid"], s["sid"]) for s in in_spans])
    return units


@pytest.mark.parametrize("app,conc", [(synth.HOTEL_APP, 2.0), (synth.FANOUT_APP, 1.3)])
def test_native_ingest_matches_python_restatement(emu_lib, tmp_path, app, conc):
    paths = synth.write_jaeger_corpus(str(tmp_path), 5, 300, app=app, concurrency=conc)
    paths = sorted(paths, reverse=True)  # any file order: the loader orders traces by root start
    ref = python_pipeline(paths, app["root_op"])
    c = Corpus(lib_path=emu_lib)
    counts = c.add_files(paths, first_span=app["root_op"], threads=3)
    assert counts["traces"] == 300 and counts["files_rejected"] == 0
    units, skipped, n_traces = c.units()
    assert n_traces == 300 and sum(skipped.values()) == 0
    assert [u.service for u in units] == list(ref.keys())
    table = c.span_table()
    for u in units:
        r, a = ref[u.service], u.arrays
        assert u.in_ep == r["in_ep"] and u.out_eps == r["out_eps"] and a.key_rank.tolist() == r["key_rank"]
        assert np.array_equal(a.in_start, r["in_start"]) and np.array_equal(a.in_end, r["in_end"])
        assert np.array_equal(a.out_start, r["out_start"]) and np.array_equal(a.out_end, r["out_end"])
        assert np.array_equal(a.dag, r["dag"]) and np.array_equal(u.true_parent, r["truth"])
        got = [c.string(table["span_id"][row]) for row in u.in_rows]
        assert got == [sid for _, sid in r["in_ids"]]          # rows translate back to span ids
    c.close()


def test_first_span_filter_and_limits(emu_lib, tmp_path):
    paths = synth.write_jaeger_corpus(str(tmp_path / "a"), 1, 40, app=synth.HOTEL_APP)
    other = synth.write_jaeger_corpus(str(tmp_path / "b"), 2, 10, app=synth.FANOUT_APP)
    bad = tmp_path / "broken.json"
    bad.write_text('{"data": [{"traceID": "x", "spans": [')
    c = Corpus(lib_path=emu_lib)
    counts = c.add_files(paths + other + [str(bad)], first_span="HTTP GET /hotels", max_traces=25)
    assert counts["traces"] == 25 and counts["files_rejected"] == 1 and "broken.json" in c.first_error()
    units, _, _ = c.units()
    assert {u.service for u in units} == {"frontend", "search"} and all(u.arrays.n_in == 25 for u in units)
    c.close()


# (golden name, directory under the reference's data/, --fix): every corpus the goldens were frozen from
REFERENCE_CORPORA = [
    ("hotel_load100", "hotel_reservation/hotel_load100", 2), ("hotel_load150", "hotel_reservation/hotel_load150", 2),
    ("media_load100", "media_microservices/media_load100", 1), ("media_load150", "media_microservices/media_load150", 1),
    ("nodeio_1", "nodejs_microservices_with_arbitrary_file_io/node_1", 0),
    ("nodeio_0.6", "nodejs_microservices_with_arbitrary_file_io/node_0.6", 0),
    ("node_load150", "nodejs_microservices/node_load150", 0),
    ("hotel_load50", "hotel_reservation/hotel_load50", 2), ("media_load50", "media_microservices/media_load50", 1),
    ("node_load100", "nodejs_microservices/node_load100", 0),
    ("nodeio_0.2", "nodejs_microservices_with_arbitrary_file_io/node_0.2", 0),
    ("hotel_load25", "hotel_reservation/hotel_load25", 2), ("hotel_load75", "hotel_reservation/hotel_load75", 2),
    ("hotel_load125", "hotel_reservation/hotel_load125", 2),
    ("media_load25", "media_microservices/media_load25", 1), ("media_load125", "media_microservices/media_load125", 1),
    ("node_load25", "nodejs_microservices/node_load25", 0), ("node_load50", "nodejs_microservices/node_load50", 0),
    ("node_load75", "nodejs_microservices/node_load75", 0), ("node_load125", "nodejs_microservices/node_load125", 0),
    ("nodeio_0", "nodejs_microservices_with_arbitrary_file_io/node_0", 0),
    ("nodeio_0.4", "nodejs_microservices_with_arbitrary_file_io/node_0.4", 0),
    ("nodeio_0.8", "nodejs_microservices_with_arbitrary_file_io/node_0.8", 0),
    # 1500 files; frozen on its first 1000 by name (with all of them the reference keeps 1001 traces and its
    # eleventh parameter block holds one sample: NaN, reference hazard H3) -- reference_files() makes the same cut
    ("media_load75", "media_microservices/media_load75", 1),
]


def reference_files(directory, max_files=1000):
    """The files of a shipped corpus the frozen runs were made from: the first `max_files` by name (oracle/refrun/gen_golden.py
    make_scratch_root) -- all of them for every corpus but media_load75."""
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.endswith(".json"))[:max_files]


@pytest.mark.parametrize("name,rel,fix", REFERENCE_CORPORA, ids=[c[0] for c in REFERENCE_CORPORA])
def test_native_ingest_reproduces_the_reference_inputs(emu_lib, reference_root, name, rel, fix):
    """The arrays the native loader hands the engine == the arrays the reference's executor handed TraceWeaverV3 in
    the frozen runs (tests/golden/ref_*): plain Jaeger (hotel), FixSpans2 (media), FixSpans (nodejs)."""
    from traceweaver_amd.ingest import REFERENCE_FIX

    first_span, surgery = REFERENCE_FIX[fix]
    c = Corpus(lib_path=emu_lib)
    counts = c.add_files(reference_files(os.path.join(reference_root, "data", rel)), first_span=first_span, max_traces=1001, fix=surgery)
    assert counts["traces"] == 1000 and counts["files_rejected"] == 0 and counts["traces_filtered"] == 0
    units, skipped, _ = c.units()
    golden = {os.path.basename(p)[len("ref_%s__" % name):-4]: p for p in GOLDEN if os.path.basename(p).startswith("ref_%s__" % name)}
    assert {u.service for u in units} == set(golden)          # the same services reach the predictor
    assert skipped["several_callers"] == (1 if fix == 1 else 0)   # media: compose-review-service (executor.py:1126-1128)
    for u in units:
        g = np.load(golden[u.service])
        a = u.arrays
        assert np.array_equal(a.in_start, g["in_start"]) and np.array_equal(a.in_end - a.in_start, g["in_dur"])
        assert np.array_equal(a.out_off, g["out_off"]) and np.array_equal(a.out_start, g["out_start"])
        assert np.array_equal(a.out_end - a.out_start, g["out_dur"]) and np.array_equal(a.dag, g["dag"])
        assert u.out_eps == [str(x) for x in g["out_eps"]] and u.in_ep == str(g["in_ep"])
        assert np.array_equal(u.true_parent, g["true_parent"])
        order = [str(x) for x in g["partition_key_order"]]
        assert a.key_rank.tolist() == [order.index(e) for e in u.out_eps]
    c.close()


def reconstruct(lib_path, tmp_path):
    paths = synth.write_jaeger_corpus(str(tmp_path), 9, 2000, app=synth.FANOUT_APP, concurrency=1.4)
    c = Corpus(lib_path=lib_path)
    c.add_files(paths, first_span="compose", max_traces=0)
    units, _, n_traces = c.units()
    eng = Engine(0, lib_path=lib_path)
    eng.load([u.arrays for u in units])
    eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
    eng.run_pass1()
    eng.fit_mixtures()
    eng.run_pass2()
    per, (right, right_topk) = eng.evaluate()
    eng.close()
    c.close()
    assert [u.service for u in units] == ["gateway", "text"] and [u.arrays.E for u in units] == [4, 2]
    assert all(p["accuracy"] > 0.9 for p in per) and right_topk >= right > 0.85 * n_traces
    return per


def test_json_to_assignment_end_to_end_emulated(emu_lib, tmp_path):
    reconstruct(emu_lib, tmp_path)


@pytest.mark.gpu
def test_json_to_assignment_end_to_end_gpu(tmp_path):
    reconstruct(None, tmp_path)


# ------------------------------------------------------------------------------------------------
# --fix 5: the output shape of alibaba-analysis/real-parser.py (rpc-id span ids, a server + a client record per call,
# self-calls split off as "...-loop" services, traces breaking containment dropped) -- executor.py:377-448.
# tests/golden/refali_*.npz: the unmodified reference parsed a generated corpus of that shape and ran predictor 10
# (oracle/refrun/gen_golden_alibaba.py); the corpus is regenerated here from the recorded seed.
ALI = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refali_*.npz")))


def _ali_cases():
    names = sorted({os.path.basename(p)[len("refali_"):].rsplit("__", 1)[0] for p in ALI})
    return [(n, [p for p in ALI if os.path.basename(p).startswith("refali_%s__" % n)]) for n in names]


def _same_service(mine, ref):
    return mine == ref or (mine.endswith("-loop") and ref.endswith("-loop"))   # the reference draws that name at random


@pytest.mark.parametrize("name,files", _ali_cases(), ids=[c[0] for c in _ali_cases()])
def test_alibaba_parser_shape_matches_the_reference_inputs(emu_lib, tmp_path, name, files):
    from traceweaver_amd import transforms

    gs = sorted((np.load(p) for p in files), key=lambda g: int(g["service_order"]))
    seed, n_traces = (int(x) for x in gs[0]["corpus"])
    conc, viol = (float(x) for x in gs[0]["corpus_params"])
    factor = int(gs[0]["compress_factor"])
    replicas = dict(zip((str(s) for s in gs[0]["replica_names"]), (int(r) for r in gs[0]["replica_counts"])))
    synth.write_alibaba_corpus(str(tmp_path), seed, n_traces, concurrency=conc, violations=viol)
    c = Corpus(lib_path=emu_lib)
    counts = c.add_directory(str(tmp_path), first_span=None, max_traces=1001, fix="rpc_twins")
    assert counts["files_rejected"] == 0 and counts["traces_filtered"] > 0 and counts["traces"] == len(gs[0]["in_start"])
    units, skipped, _ = c.units()
    assert sum(skipped.values()) == 0
    loops = [u for u in units if u.service.endswith("-loop")]
    assert len(loops) == 1 and c.loop_origin(loops[0].service) == "cart" and c.loop_origin("cart") is None
    if factor == 1:
        assert len(units) == len(gs)                          # the same services reach the predictor, in the same order
    names = c.trace_names()
    table = c.span_table()
    for g in gs:
        u = units[int(g["service_order"])]
        assert _same_service(u.service, str(g["process"])) and u.process_id == int(g["service_order"])
        assert len(u.out_eps) == len(g["out_eps"]) and all(_same_service(a, str(b)) for a, b in zip(u.out_eps, g["out_eps"]))
        assert _same_service(u.in_ep, str(g["in_ep"]))
        tids = [c.string(names[t]) for t in u.in_trace]
        a, truth = u.arrays, u.true_parent
        if factor > 1:                                        # executor.py:1086-1097 + helpers/transforms.py:10-40
            f = transforms.load_factor(factor, replicas[c.loop_origin(u.service) or u.service])
            s = transforms.compress_unit(a, truth, f, trace_key=tids)
            assert np.array_equal(s.in_start, g["in_start"]) and np.array_equal(s.out_start, g["out_start"])   # the reference's floats
            a, truth, tids = s.arrays, s.true_parent, [tids[i] for i in s.in_perm]
            in_sid = [c.string(table["span_id"][r]) for r in u.in_rows[s.in_perm]]
            assert np.array_equal(a.in_end - a.in_start, (g["in_dur"] / a.time_scale).astype(np.int64))
        else:
            in_sid = [c.string(table["span_id"][r]) for r in u.in_rows]
            assert np.array_equal(a.in_start, g["in_start"]) and np.array_equal(a.in_end - a.in_start, g["in_dur"])
            assert np.array_equal(a.out_start, g["out_start"]) and np.array_equal(a.out_end - a.out_start, g["out_dur"])
        assert np.array_equal(a.out_off, g["out_off"]) and np.array_equal(a.dag, g["dag"])
        assert tids == [str(t) for t in g["in_trace_id"]] and in_sid == [str(x) for x in g["in_span_id"]]
        assert np.array_equal(truth, g["true_parent"])
        order = [str(x) for x in g["partition_key_order"]]
        assert a.key_rank.tolist() == [order.index(str(e)) for e in g["out_eps"]]
    c.close()


def _snapshot(c):
    """Everything a corpus hands out, with names resolved to text (string ids are handles)."""
    table = c.span_table()
    units, skipped, n_traces = c.units()
    names = [c.string(i) for i in c.trace_names()]
    cols = {k: (table[k].tolist() if k not in ("span_id", "service", "op_name") else [c.string(i) for i in table[k]]) for k in table}
    us = [(u.service, u.in_ep, u.out_eps, u.arrays.in_start.tolist(), u.arrays.in_end.tolist(), u.arrays.out_off.tolist(),
           u.arrays.out_start.tolist(), u.arrays.out_end.tolist(), u.arrays.dag.tolist(), u.arrays.key_rank.tolist(),
           u.true_parent.tolist(), u.in_trace.tolist(), u.in_rows.tolist(), [r.tolist() for r in u.out_rows], u.process_id) for u in units]
    raw_ids = (table["service"].tolist(), table["op_name"].tolist(), table["span_id"].tolist())
    return names, cols, us, skipped, n_traces, c.counts(), raw_ids


@pytest.mark.parametrize("shape", ["hotel", "alibaba"])
def test_parser_thread_count_changes_nothing(emu_lib, tmp_path, shape):
    """Rows, units and even the string ids are the same for 1, 3 and 8 parser threads (names are interned by one thread in
    trace order, whichever thread parsed the trace), and for the file list in any order."""
    if shape == "hotel":
        paths, fix = synth.write_jaeger_corpus(str(tmp_path), 11, 400, app=synth.HOTEL_APP, concurrency=2.5), None
    else:
        paths, fix = synth.write_alibaba_corpus(str(tmp_path), 11, 400, concurrency=1.5, violations=0.02), "rpc_twins"
    snaps = []
    for threads, order in ((1, paths), (3, paths), (8, paths)):
        c = Corpus(lib_path=emu_lib)
        c.add_files(order, first_span=None, max_traces=0, threads=threads, fix=fix)
        snaps.append(_snapshot(c))
        c.close()
    assert snaps[0] == snaps[1] == snaps[2]
    assert snaps[0][4] > 300 and len(snaps[0][2]) >= 2
    # two calls on one corpus append (rows and trace numbers continue)
    c = Corpus(lib_path=emu_lib)
    c.add_files(paths[:150], first_span=None, max_traces=0, threads=2, fix=fix)
    first = c.counts()
    c.add_files(paths[150:], first_span=None, max_traces=0, threads=4, fix=fix)
    both = c.counts()
    assert both["files"] == len(paths) and both["spans"] > first["spans"] and both["traces"] > first["traces"]
    table = c.span_table()
    assert all(c.string(i) is not None for i in table["span_id"][[0, first["spans"] - 1, first["spans"], both["spans"] - 1]])
    assert c.string(int(c.trace_names()[-1])) is not None and c.string(both["strings"] + (1 << 30)) is None
    c.close()


def test_scanner_escapes_numbers_and_duplicates(emu_lib, tmp_path):
    """The paths of the scanner a generated corpus never takes: escaped keys and values (decoded like json.load does),
    numbers of 19 digits and in exponent notation, values the loader does not read (nested, escaped, unicode), a span id
    that occurs twice (the later record wins, as in the reference's dict), unknown keys before and after the known ones."""
    def span(sid, op, start, dur, kind, pid, refs, tid="t\\u0031", extra=""):
        return ('{"x\\"y": {"deep": [1, 2.5e3, "a\\\\b\\"c", null, true, {"k": "\\ud83d\\ude00"}]}, "traceID": "%s", "sp\\u0061nID": "%s", %s'
                '"operationName": "%s", "references": [%s], "startTime": %s, "duration": %s, '
                '"tags": [{"key": "http.url", "type": "string", "value": "a\\\\\\"b"}, {"key": "span.kind", "value": "%s"}], "logs": [{"fields": [{"key": "e", "value": "\\\\"}]}], '
                '"processID": "%s", "warnings": null}') % (tid, sid, extra, op, ", ".join('{"refType": "CHILD_OF", "traceID": "%s", "spanID": "%s"}' % (tid, r) for r in refs), start, dur, kind, pid)
    docs = []
    for n in range(40):
        t0 = 1655760000000000 + 5000 * n
        tid = "t%d" % n
        spans = [span("a", "GET /x\\ty", t0, "3.0e3" if n % 2 else 3000, "server", "p1", [], tid=tid),
                 span("b", "call", t0 + 10, 100, "client", "p1", ["a"], tid=tid),
                 span("c", "old", t0 + 1, 1, "server", "p2", ["b"], tid=tid),            # shadowed by the next record with the same id
                 span("c", "h\\u00e9llo", t0 + 20, 50, "server", "p2", ["b"], tid=tid)]
        docs.append('{"total": 0, "data": [{"spans": [%s], "processes": {"p1": {"tags": [], "serviceName": "front"}, "p2": {"serviceName": "b\\u0061ck"}}, "traceID": "%s"}], "errors": null}'
                    % (", ".join(spans), tid))
    big = '{"data": [{"traceID": "big", "spans": [%s], "processes": {"p1": {"serviceName": "front"}}}]}' % span("r", "GET /x\\ty", 9223372036854775807, 1, "server", "p1", [], tid="big")
    paths = []
    for n, text in enumerate(docs + [big]):
        json.loads(text)                                  # the fixtures are valid JSON
        p = tmp_path / ("%03d.json" % n)
        p.write_text(text)
        paths.append(str(p))
    c = Corpus(lib_path=emu_lib)
    counts = c.add_files(paths, first_span="GET /x\ty", max_traces=0, threads=2)
    assert counts["files_rejected"] == 0 and counts["traces"] == 41 and counts["spans"] == 40 * 3 + 1, (counts, c.first_error())
    table = c.span_table()
    ops = {c.string(i) for i in table["op_name"]}
    assert ops == {"GET /x\ty", "call", "héllo"} and {c.string(i) for i in table["service"]} == {"front", "back"}
    assert int(table["start"].max()) == 9223372036854775807 and set(table["duration"].tolist()) == {3000, 100, 50, 1}
    assert {c.string(i) for i in c.trace_names()} == {"t%d" % n for n in range(40)} | {"big"}
    units, skipped, _ = c.units()
    assert units == [] and skipped["skip_mode"] == 1      # the lone root of "big" makes no call: 41 requests, 40 calls
    c.close()
    c = Corpus(lib_path=emu_lib)
    c.add_files(paths[:-1], first_span="GET /x\ty", max_traces=0, threads=3)
    units, skipped, _ = c.units()
    assert [u.service for u in units] == ["front"] and units[0].out_eps == ["back"] and units[0].arrays.n_in == 40
    assert np.array_equal(units[0].arrays.out_start - units[0].arrays.in_start, np.full(40, 10))
    assert np.array_equal(units[0].true_parent, np.arange(40)[None, :])
    c.close()
    bad = tmp_path / "bad.json"
    bad.write_text(docs[0].replace('"a\\\\\\"b"', '"a\\qb"'))          # a malformed escape in a value nobody reads still rejects the file
    c = Corpus(lib_path=emu_lib)
    counts = c.add_files([str(bad)], first_span=None, max_traces=0)
    assert counts["files_rejected"] == 1 and "bad escape" in c.first_error()
    c.close()


def _same_corpus(a, b):
    ua, sa, na = a.units()
    ub, sb, nb = b.units()
    assert sa == sb and na == nb and len(ua) == len(ub)
    assert {k: v for k, v in a.counts().items() if k != "strings"} == {k: v for k, v in b.counts().items() if k != "strings"}   # (a live corpus interns names as they are asked for)
    for x, y in zip(ua, ub):
        assert (x.service, x.in_ep, x.out_eps, x.process_id) == (y.service, y.in_ep, y.out_eps, y.process_id)
        for k in ("in_start", "in_end", "out_off", "out_start", "out_end", "dag", "key_rank"):
            assert np.array_equal(getattr(x.arrays, k), getattr(y.arrays, k)), k
        assert np.array_equal(x.true_parent, y.true_parent) and np.array_equal(x.in_trace, y.in_trace) and np.array_equal(x.in_rows, y.in_rows)
        assert all(np.array_equal(p, q) for p, q in zip(x.out_rows, y.out_rows))
    ta, tb = a.span_table(), b.span_table()
    assert all(np.array_equal(ta[k], tb[k]) for k in ta)
    assert np.array_equal(a.trace_names(), b.trace_names())
    for col in ("span_id", "service", "op_name"):
        for h in np.unique(ta[col])[:200]:
            assert a.string(h) == b.string(h)
    for h in a.trace_names():
        assert a.string(h) == b.string(h)
    assert a.string(-5) is None and b.string(-5) is None


@pytest.mark.parametrize("kind", ["hotel", "alibaba"])
def test_span_table_cache_of_a_directory(emu_lib, tmp_path, kind):
    """ingest.open_directory: the second load of a directory starts from the cache file the first one left
    in it and offers exactly the same corpus; --clear_cache, other arguments, a changed directory or a broken file mean a
    fresh load."""
    from traceweaver_amd import ingest

    d = str(tmp_path)
    if kind == "alibaba":
        synth.write_alibaba_corpus(d, 5, 300, concurrency=1.5)
        kw = dict(first_span=None, max_traces=0, fix="rpc_twins")
    else:
        synth.write_jaeger_corpus(d, 5, 300, app=synth.HOTEL_APP)
        kw = dict(first_span=synth.HOTEL_APP["root_op"], max_traces=0, fix=None)
    fresh, counts = ingest.open_directory(d, lib_path=emu_lib, **kw)
    assert not fresh.from_cache and os.path.exists(os.path.join(d, ingest.CACHE_FILE)) and counts["traces"] > 0
    again, counts2 = ingest.open_directory(d, lib_path=emu_lib, **kw)
    assert again.from_cache and counts2 == counts
    _same_corpus(fresh, again)
    if kind == "alibaba":
        loops = [u.service for u in fresh.units()[0] if u.service.endswith("-loop")]
        for sv in loops + ["no-such-service"]:
            assert fresh.loop_origin(sv) == again.loop_origin(sv)
    # a miss: other arguments / cache not wanted / cleared / a trace removed / a damaged file
    assert not ingest.open_directory(d, lib_path=emu_lib, **dict(kw, max_traces=7))[0].from_cache
    assert not ingest.open_directory(d, lib_path=emu_lib, cache=False, **dict(kw, max_traces=7))[0].from_cache
    assert ingest.open_directory(d, lib_path=emu_lib, **dict(kw, max_traces=7))[0].from_cache
    assert not ingest.open_directory(d, lib_path=emu_lib, clear_cache=True, **kw)[0].from_cache
    assert ingest.open_directory(d, lib_path=emu_lib, **kw)[0].from_cache
    victim = sorted(f for f in os.listdir(d) if f.endswith("json"))[0]
    os.remove(os.path.join(d, victim))
    smaller, counts3 = ingest.open_directory(d, lib_path=emu_lib, **kw)
    assert not smaller.from_cache and counts3["files"] == counts["files"] - 1
    with open(os.path.join(d, ingest.CACHE_FILE), "r+b") as f:
        f.truncate(100)
    assert not ingest.open_directory(d, lib_path=emu_lib, **kw)[0].from_cache
    assert ingest.open_directory(d, lib_path=emu_lib, **kw)[0].from_cache


def test_command_line_from_the_span_table_cache(emu_lib, tmp_path):
    """`--span_cache 1`: the second run of the command line starts from the directory's cache and writes the same result files."""
    import pickle

    from traceweaver_amd import executor, ingest

    data = tmp_path / "data"
    data.mkdir()
    synth.write_jaeger_corpus(str(data), 5, 400, app=synth.HOTEL_APP, concurrency=2.0)
    runs = []
    for k in range(2):
        out = str(tmp_path / ("out%d" % k)) + "/"
        executor.main(["--absolute_path", str(data), "--compressed", "0", "--cache_rate", "0", "--fix", "2", "--test_name", "t",
                       "--load_level", "100", "--results_directory", out, "--predictor_indices", "3,4,7,10", "--span_cache", "1",
                       "--engine_library", emu_lib])
        runs.append({f: pickle.load(open(out + f, "rb")) for f in sorted(os.listdir(out)) if f.endswith(".pickle")})
    assert os.path.exists(str(data / ingest.CACHE_FILE))
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) >= 5
    assert pickle.dumps(runs[0]) == pickle.dumps(runs[1])
