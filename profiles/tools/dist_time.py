"""Times Engine.distributions (tw_latency_distributions, csrc/tw_dist.h) next to the stitch and the attribution it follows, in one
process on one resident batch: tw_get_timing slots 22..24 beside slots 10..15, 16..18 and 19..21 (HIP events) and the rate of
tw_measure_hbm_copy.  The batch is the media-shape table of profiles/attr_time.json and profiles/conf_time.json (conf_time.py
builds it).  Two queries: the default 5 % selection, and percentile 0 (every eligible tree: the worst case for items and sort).
Writes one JSON document.

    python profiles/tools/dist_time.py --out profiles/dist_time.json            # 0.2 M and 52 M rows
    python profiles/tools/dist_time.py --sizes 1x2000 --lib <host build>        # a rehearsal without a GPU: no times worth reading
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conf_time import span_table  # noqa: E402
from traceweaver_amd import synth, traces  # noqa: E402
from traceweaver_amd.engine import Engine  # noqa: E402

PROBS = (0.5, 0.95, 0.99)
EDGES = tuple(10 ** k for k in range(1, 8))
# bytes k_dist_items needs per row: the row's tree 4 and the tree's selection byte 1 in either sweep; a row of a selected tree also
# its cohort 4, group 4, flag 1, start 8, end 8, self time 8, path time 8 in either sweep, and 8 written per item in the second
UNSELECTED_ROW, SELECTED_ROW, ITEM = 2 * 5, 2 * 41, 8


def measure(eng, replicas, n_in, rounds, check):
    units, _ = synth.make_workload(7, n_in, services=synth.MEDIA_SERVICES, replicas=replicas, concurrency=1.6)
    rows, group = span_table(units)
    eng.load(units)
    eng.run_pass1()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, 8)
    n_rows = len(rows[2])
    st = eng.stitch()
    out = {"rows": n_rows, "trees": st.n_trees, "counts": st.counts.tolist(), "stitch_ms": eng.stitch_timing(), "score_ms": None}
    eng.score_traces(0.0, (0.0, 1.0, 2.0, 5.0))
    out["score_ms"] = eng.score_timing()
    gbps = eng.hbm_copy_gbps()
    out["hbm_copy_gbps"] = gbps
    for tag, pct in (("percentile_0.95", 0.95), ("percentile_0", 0.0)):
        runs = []
        for _ in range(rounds):
            a = eng.attribute(percentile=pct)
            d = eng.distributions(PROBS, EDGES, values=False)
            runs.append({"attribute": eng.attribute_timing(), "distributions": eng.distributions_timing()})
        best = min(runs[1:] or runs, key=lambda t: sum(t["distributions"].values()))
        sel_rows = int(d.seg_count[:8].sum()) + 0
        b_items = UNSELECTED_ROW * (n_rows - sel_rows) + SELECTED_ROW * sel_rows + ITEM * d.n_items
        out[tag] = {"selected_trees": a.n_selected, "selected_rows": sel_rows, "items": d.n_items, "segments": int(d.summary[1]),
                    "distributions_ms": best["distributions"], "attribute_ms": best["attribute"], "all": runs,
                    "items_over_attr_reduce": best["distributions"]["items"] / best["attribute"]["reduce"],
                    "items_kernel": {"bytes": b_items, "bytes_per_row": b_items / float(n_rows), "gbps": b_items / best["distributions"]["items"] / 1e6,
                                     "of_copy_rate": b_items / best["distributions"]["items"] / 1e6 / gbps},
                    "sort": {"bytes_per_item_and_pass": 16, "items_per_ms": d.n_items / best["distributions"]["sort"] if best["distributions"]["sort"] > 0 else None}}
        if check:
            full = eng.distributions(PROBS, EDGES)
            want = traces.distributions_host(st, a, rows[4], rows[5], group, 8, None, 1, PROBS, EDGES)
            out[tag]["equals_host"] = bool(full.same_as(want))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1x8000,16x125000", help="replicas x requests per service, comma separated; the first one is checked against the host restatement")
    ap.add_argument("--rounds", type=int, default=4, help="attribute + distributions calls per query: a warm-up and the best of the rest")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    eng = Engine(0, lib_path=args.lib)
    doc = {"what": "tw_latency_distributions next to tw_stitch_traces, tw_score_traces and tw_attribute_traces on one MI355X, same batch and process: HIP "
                   "events of tw_get_timing slots 22..24 (cohorts + the two sweeps of k_dist_items; sort, offsets and values; quantiles and histogram), "
                   "10..15, 16..18 and 19..21; per query --rounds attribute + distributions calls, the best distributions call after the first, all "
                   "listed; one cohort, 8 groups (25 segments: the LDS route), no ground truth set.  Rows: media-shape synthetic batch, every request, "
                   "every call and a callee span below every call.  The yardsticks are attribute_ms.reduce (k_attr_reduce over the same rows) and "
                   "hbm_copy_gbps, taken in the same run."}
    for k, size in enumerate(args.sizes.split(",")):
        r, n = (int(x) for x in size.split("x"))
        key = "media_shape_%dx%d" % (r, n)
        doc[key] = measure(eng, r, n, args.rounds, check=k == 0)
        print(size, json.dumps({q: {a: doc[key][q][a] for a in ("items", "distributions_ms", "attribute_ms", "items_over_attr_reduce")} for q in ("percentile_0.95", "percentile_0")}), flush=True)
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
