"""Times Engine.score_traces (tw_score_traces, csrc/tw_conf.h) next to the stitch and the attribution it follows, in one process
on one resident batch: tw_get_timing slots 19..21 beside slots 10..15 and 16..18 (HIP events).  The batch is the media-shape
table of profiles/attr_time.json: --replicas copies of the six media services with --n-in requests each; every request, every
call and a callee span below every call are rows of the span table (depth-2 trees).  Writes one JSON document.

    python profiles/tools/conf_time.py --out profiles/conf_time.json            # 0.2 M and 52 M rows
    python profiles/tools/conf_time.py --sizes 1x2000 --lib <host build>        # a rehearsal without a GPU: no times worth reading
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from traceweaver_amd import synth, traces  # noqa: E402
from traceweaver_amd.engine import Engine  # noqa: E402

EDGES = (0.0, 1.0, 2.0, 5.0)


def span_table(units):
    """Rows per unit: its requests (roots), its calls per endpoint, one callee span below every call."""
    in_rows, out_rows, link, kind, start, end, group = [], [], [], [], [], [], []
    base = 0
    for k, u in enumerate(units):
        n_out = int(u.out_off[-1])
        in_rows.append(np.arange(base, base + u.n_in, dtype=np.int32))
        calls = base + u.n_in + np.arange(n_out, dtype=np.int32)
        out_rows.append([calls[int(u.out_off[e]):int(u.out_off[e + 1])] for e in range(u.E)])
        link += [np.full(u.n_in + n_out, -1, dtype=np.int32), calls.astype(np.int32)]
        kind += [np.full(u.n_in, 1, dtype=np.uint8), np.full(n_out, 2, dtype=np.uint8), np.full(n_out, 1, dtype=np.uint8)]
        start += [u.in_start, u.out_start, u.out_start + 1]
        end += [u.in_end, u.out_end, np.maximum(u.out_end - 1, u.out_start + 1)]
        callee = np.concatenate([np.full(int(u.out_off[e + 1] - u.out_off[e]), 4 + e, dtype=np.int32) for e in range(u.E)])
        group += [np.full(u.n_in + n_out, k % 4, dtype=np.int32), callee]
        base += u.n_in + 2 * n_out
    cat = np.concatenate
    return (in_rows, out_rows, cat(link), cat(kind), cat(start).astype(np.int64), cat(end).astype(np.int64)), cat(group)


def measure(eng, replicas, n_in, rounds, check):
    units, _ = synth.make_workload(7, n_in, services=synth.MEDIA_SERVICES, replicas=replicas, concurrency=1.6)
    rows, group = span_table(units)
    eng.load(units)
    eng.run_pass1()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, 8)
    runs = []
    for _ in range(rounds):
        st = eng.stitch()
        conf = eng.score_traces(0.0, EDGES)
        t = {"stitch": eng.stitch_timing(), "score": eng.score_timing()}
        eng.attribute(percentile=0.95, need_flags=traces.WHOLE | traces.CONFIDENT)
        t["attribute"] = eng.attribute_timing()
        runs.append(t)
    n_req, n_rows, n_trees = int(sum(u.n_in for u in units)), len(rows[2]), st.n_trees
    best = min(runs[1:] or runs, key=lambda t: sum(t["score"].values()))
    whole = sum(best["score"].values())
    gbps = eng.hbm_copy_gbps()
    # bytes the algorithm needs.  Decision kernel, per request: chosen 4 + rep 1 + list length 4 + two scores 16 read, rank 4 +
    # list_n 4 + margin 8 written.  Tree reduction: the row map (4 written per row, in_row 4 read + 4 written per request), two
    # sweeps over the rows (tree_rows 4 + row_request 4 each) and the decisions (rank 4 + margin 8, then margin 8), per tree its
    # offset 8, the figures 4 * 4 + 8 + 1 and the flags 1 + 1.
    b_dec = 41 * n_req
    b_tree = 4 * n_rows + 8 * n_req + 2 * 8 * n_rows + 20 * n_req + 35 * n_trees
    out = {"rows": n_rows, "requests": n_req, "trees": n_trees, "counts": st.counts.tolist(), "summary5": conf.summary.tolist(),
           "calib": conf.calib.tolist(), "edges": list(EDGES), "score_ms": best["score"], "stitch_ms": best["stitch"], "attribute_ms": best["attribute"],
           "all": runs, "score_whole_ms": whole, "score_over_stitch": whole / best["stitch"]["stitch"],
           "hbm_copy_gbps": gbps,
           "decision_kernel": {"bytes_per_request": 41, "gbps": b_dec / best["score"]["decisions"] / 1e6, "of_copy_rate": b_dec / best["score"]["decisions"] / 1e6 / gbps},
           "tree_reduction": {"bytes": b_tree, "gbps": b_tree / best["score"]["trees"] / 1e6, "of_copy_rate": b_tree / best["score"]["trees"] / 1e6 / gbps}}
    if check:
        dec = eng.decisions()
        want = traces.confidence_host(st, rows[0], [d["rank"] for d in dec], [d["margin"] for d in dec], 0.0, EDGES, list_n=[d["list_n"] for d in dec])
        out["equals_host"] = bool(conf.same_as(want))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1x8000,16x125000", help="replicas x requests per service, comma separated; the first one is checked against the host restatement")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    eng = Engine(0, lib_path=args.lib)
    doc = {"what": "tw_score_traces next to tw_stitch_traces and tw_attribute_traces on one MI355X, same batch and process: HIP events of tw_get_timing "
                   "slots 19..21 (decision kernel, row map + per-tree reduction, calibration), 10..15 and 16..18; --rounds stitch + score + "
                   "attribute(percentile=0.95, whole and confident) calls, the best scoring call after the first, all listed; no ground truth set.  "
                   "Rows: media-shape synthetic batch, every request, every call and a callee span below every call."}
    for k, size in enumerate(args.sizes.split(",")):
        r, n = (int(x) for x in size.split("x"))
        doc["media_shape_%dx%d" % (r, n)] = measure(eng, r, n, args.rounds, check=k == 0)
        print(size, json.dumps({a: doc["media_shape_%dx%d" % (r, n)][a] for a in ("rows", "trees", "score_ms", "score_over_stitch", "decision_kernel", "tree_reduction")}), flush=True)
    eng.close()
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
