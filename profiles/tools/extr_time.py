"""Times Engine.extract_traces (tw_extract_traces / tw_get_extracted, csrc/tw_extr.h) on one resident batch: tw_get_timing slots 49..51
(HIP events) and the wall clock of the whole Python call, beside what the same answer costs without the stage -- Engine.stitch()'s copy
of the whole forest to the host plus Engine.attribute()'s link table, timed in the same process and round (wall clock of the call
less the device time of its kernels) -- and the rate of tw_measure_hbm_copy.  The batch is the media-shape table of
profiles/filt_time.json (conf_time.py builds it), stitched from the true assignment, with an attribution resident, so the self and
path times are gathered.  Queries: (a) the 100 slowest traces, (b) the exemplars at five quantiles, (c) a list of 10^4 trees, (d) the
whole forest in tree order (tw_extract_traces alone: the result stays on the device).  Writes one JSON document.

    python profiles/tools/extr_time.py --out profiles/extr_time.json            # 0.2 M and 52 M rows
    python profiles/tools/extr_time.py --sizes 1x2000 --lib <host build>        # a rehearsal without a GPU: no times worth reading
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conf_time import span_table  # noqa: E402
from traceweaver_amd import _ffi, synth, traces  # noqa: E402
from traceweaver_amd.engine import Engine  # noqa: E402

ROW_BYTES_READ = 4 + 4 + 4 + 1 + 4 + 8 + 8 + 8 + 8      # tree_rows, link, depth, row_kind, row_group, start, end, self_time, path_time
ROW_BYTES_WRITTEN = 4 * 4 + 1 + 4 + 4 * 8               # row, parent, depth, subtree, kind, group, start, end, self_time, path_time
TREE_BYTES = 4 + 8 + 8 + 8                              # sel_tree, the two ends in tree_off, out_off (k_extr_trees; the sel_* columns are k_extr_sizes')


def wall(call):
    t = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t) * 1e3


def whole_forest(eng):
    """(d): tw_extract_traces alone, TOP by tree with limit 0."""
    q = _ffi.ExtractQuery(traces.WHOLE, 0, 0, 0, 0, 0, 0, None, None)
    summary = np.zeros(6, dtype=np.int64)
    _, ms = wall(lambda: eng._check(eng._lib.tw_extract_traces(eng._h, ctypes.byref(q), summary.ctypes.data_as(ctypes.c_void_p))))
    return summary, ms


def measure(eng, replicas, n_in, rounds, check, single_rows):
    units, truth = synth.make_workload(7, n_in, services=synth.MEDIA_SERVICES, replicas=replicas, concurrency=1.6)
    rows, group = span_table(units)
    eng.load(units)
    eng.set_truth(truth)
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, 8)
    st = eng.stitch(truth=True)
    listed = np.random.default_rng(3).integers(0, st.n_trees, size=min(10000, st.n_trees)).astype(np.int32)
    queries = {"top_100_slowest": dict(mode="top", order="slowest", limit=100), "quantiles_5": dict(mode="quantiles", probs=(0.5, 0.9, 0.95, 0.99, 1.0)),
               "list_10000": dict(mode="list", trees=listed)}
    gbps = eng.hbm_copy_gbps()
    out = {"rows": len(rows[2]), "trees": st.n_trees, "hbm_copy_gbps": gbps}
    runs = []
    for k in range(rounds + 1):
        _, stitch_ms = wall(lambda: eng.stitch(truth=True))
        stitch_dev = eng.stitch_timing()["stitch"]
        a, attr_ms = wall(lambda: eng.attribute(percentile=0.0))
        attr_dev = sum(eng.attribute_timing().values())
        run = {"stitch_call_ms": stitch_ms, "stitch_device_ms": stitch_dev, "attribute_call_ms": attr_ms, "attribute_device_ms": attr_dev,
               "host_copy_ms": (stitch_ms - stitch_dev) + (attr_ms - attr_dev)}
        for name, q in queries.items():
            x, ms = wall(lambda: eng.extract_traces(**q))
            run[name] = dict(eng.extract_timing(), call_ms=ms, selected=x.n_trees, eligible=x.n_eligible, rows=int(x.summary[2]), times=int(x.summary[5]))
        summary, ms = whole_forest(eng)
        t = eng.extract_timing()
        nbytes = int(summary[2]) * (ROW_BYTES_READ + ROW_BYTES_WRITTEN) + int(summary[1]) * TREE_BYTES
        run["whole_forest"] = {"select": t["select"], "trees": t["trees"], "call_ms": ms, "selected": int(summary[1]), "rows": int(summary[2]),
                               "single_tree_route": int(summary[4]), "bytes": nbytes, "gbps": nbytes / (t["trees"] * 1e6) if t["trees"] > 0 else 0.0}
        run["whole_forest"]["fraction_of_hbm_copy"] = run["whole_forest"]["gbps"] / gbps if gbps > 0 else 0.0
        runs.append(run)
        print("round %d of %d" % (k, rounds), file=sys.stderr, flush=True)
    for name in list(queries) + ["whole_forest"]:
        best = min(runs[1:], key=lambda r: r[name]["select"] + r[name]["trees"])
        out[name] = dict(best[name], host_copy_ms=best["host_copy_ms"])
    if check:
        for name, q in queries.items():
            host = traces.extract_host(st, a.link, rows[3], rows[4], rows[5], group, attribution=traces.attribute_host(st, a.link, rows[4], rows[5], group, 8),
                                       single_rows=single_rows, **q)
            out[name]["equals_host"] = bool(eng.extract_traces(**q).same_as(host))
    out["all"] = runs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1x8000,16x125000", help="replicas x requests per service, comma separated; the first one is checked against the host restatement")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of stitch, attribute and the four extractions after a warm-up: the best is reported, all are listed")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--single_rows", type=int, default=traces.EXTRACT_SINGLE_ROWS, help="kExtrCap of the library (the host build of the tests: 12), for the check's summary")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    eng = Engine(0, lib_path=args.lib)
    doc = {"what": "tw_extract_traces / tw_get_extracted on one MI355X: HIP events of tw_get_timing slots 49..51 (select: selection, sizes and offsets; trees: "
                   "k_extr_trees; copies: tw_get_extracted to the host) and call_ms, the wall clock of Engine.extract_traces; host_copy_ms: what the same "
                   "answer costs without the stage, the wall clock of Engine.stitch() and Engine.attribute() less the device time of their kernels (the "
                   "copies of the forest and of link, self_time and path_time to the host), same process and round; --rounds + 1 rounds, per query the "
                   "best after the first, all listed.  whole_forest: TOP by tree with limit 0, tw_extract_traces alone; bytes = rows x (%d read + %d "
                   "written) + trees x %d; gbps over the tree kernel's time, as a fraction of tw_measure_hbm_copy's rate.  Rows: media-shape synthetic "
                   "batch, every request, every call and a callee span below every call, stitched from the true assignment, attribution resident." % (
                       ROW_BYTES_READ, ROW_BYTES_WRITTEN, TREE_BYTES)}
    for k, size in enumerate(args.sizes.split(",")):
        r, n = (int(x) for x in size.split("x"))
        key = "media_shape_%dx%d" % (r, n)
        doc[key] = measure(eng, r, n, args.rounds, k == 0, args.single_rows)
        print(size, json.dumps({q: v for q, v in doc[key].items() if q != "all"}), flush=True)
    eng.close()
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
