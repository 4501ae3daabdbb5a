"""Times Engine.filter_traces (tw_filter_traces, csrc/tw_filt.h) next to the two older sweeps over the same rows, in one process on one
resident batch and in the same round: tw_get_timing slots 46..48 beside slot 22 (k_dist_cohort and the two sweeps of k_dist_items,
with cohort labels set) and slot 28 (k_prof_clear + k_prof_rows), HIP events, and the rate of tw_measure_hbm_copy.  The batch is the
media-shape table of profiles/prof_time.json (conf_time.py builds it), stitched from the true assignment: the filter reads a forest,
whichever assignment made it, and the truth needs no pass.  Queries of 1, 4 and 16 clauses; the second holds an EDGE clause and a
clause on self time.  Writes one JSON document.

    python profiles/tools/filt_time.py --out profiles/filt_time.json            # 0.2 M and 52 M rows
    python profiles/tools/filt_time.py --sizes 1x2000 --lib <host build>        # a rehearsal without a GPU: no times worth reading
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
from traceweaver_amd.traces import clause  # noqa: E402


def queries(latency, span):
    """The three queries, bounds at the medians of the batch: 1 clause (the longest span of a trace), 4 clauses in 2 terms (latency and
    a group sum; an edge count and the least self time), 16 clauses in 8 terms (the four of the second, then group sums, minima and
    maxima of every metric)."""
    one = [clause("group", span, None, group=-1, metric="span", reduce="max")]
    four = [clause("latency", latency, None, term=0), clause("group", span, None, term=0, group=4, metric="span"),
            clause("edge", 1, None, term=1, group=4, caller=0), clause("group", None, span, term=1, group=-1, metric="self", reduce="min")]
    more = [clause("group", lo, hi, term=2 + k // 2, group=g, metric=m, reduce=r, negate=k % 5 == 4)
            for k, (g, m, r, lo, hi) in enumerate([(0, "span", "max", span, None), (1, "self", "sum", None, span), (2, "path", "max", 1, None), (3, "onpath", "sum", 1, None),
                                                   (5, "count", "sum", 1, 1), (6, "span", "min", None, span), (7, "self", "max", span, None), (-1, "path", "sum", latency, None),
                                                   (-1, "count", "sum", 3, None), (4, "span", "sum", None, 2 * span), (5, "self", "min", 1, None), (-1, "onpath", "sum", 2, None)])]
    return {"1_clause": one, "4_clauses": four, "16_clauses": four + more}


def measure(eng, replicas, n_in, rounds, check):
    units, truth = synth.make_workload(7, n_in, services=synth.MEDIA_SERVICES, replicas=replicas, concurrency=1.6)
    rows, group = span_table(units)
    eng.load(units)
    eng.set_truth(truth)
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, 8)
    eng.set_row_cohorts(np.where(group >= 0, group % 2, -1).astype(np.int32), 2)   # (so that k_dist_cohort runs: a sweep of the same shape)
    st = eng.stitch(truth=True)
    dur = np.maximum(rows[5] - rows[4], 0)
    q = queries(int(np.median(st.tree_latency)), int(np.median(dur)))
    out = {"rows": len(rows[2]), "trees": st.n_trees, "hbm_copy_gbps": eng.hbm_copy_gbps()}
    runs = []
    for k in range(rounds + 1):
        a = eng.attribute(percentile=0.0)                         # (drops the items and the profile: every stage below runs its kernels)
        eng.distributions((0.5,), None, values=False)
        eng.signatures("edges")
        eng.class_profiles()
        run = {"dist_items_ms": eng.distributions_timing()["items"], "prof_sweep_ms": eng.profiles_timing()["sweep"]}
        for name, clauses in q.items():
            f = eng.filter_traces(clauses)
            run[name] = dict(eng.filter_timing(), matched=f.n_matched, eligible=f.n_eligible)
        runs.append(run)
    for name, clauses in q.items():
        best = min(runs[1:], key=lambda r: r[name]["trees"])
        out[name] = dict(best[name], prof_sweep_ms=best["prof_sweep_ms"], dist_items_ms=best["dist_items_ms"],
                         trees_over_prof_sweep=best[name]["trees"] / best["prof_sweep_ms"], trees_over_dist_items=best[name]["trees"] / best["dist_items_ms"],
                         expression=traces.format_filter(clauses))
        if check:
            sig = traces.signatures_host(st, a.link, rows[3], group, 8, "edges")
            host = traces.attribute_host(st, a.link, rows[4], rows[5], group, 8)
            out[name]["equals_host"] = bool(eng.filter_traces(clauses).same_as(
                traces.filter_host(st, a.link, rows[3], rows[4], rows[5], group, 8, clauses, attribution=host, signatures=sig)))
    out["all"] = runs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1x8000,16x125000", help="replicas x requests per service, comma separated; the first one is checked against the host restatement")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of attribute, distributions, signatures, class_profiles and the three filters after a warm-up: the best is reported, all are listed")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    eng = Engine(0, lib_path=args.lib)
    doc = {"what": "tw_filter_traces next to tw_latency_distributions and tw_class_profiles on one MI355X, same batch, process and round: HIP events of "
                   "tw_get_timing slots 46..48 (trees: k_filt_trees; list: the three scan kernels; copies: to the host, clause_value [trees][clauses] among "
                   "them), slot 22 (dist_items_ms: k_dist_cohort + k_dist_items twice, with two cohorts) and slot 28 (prof_sweep_ms: k_prof_clear + "
                   "k_prof_rows); --rounds + 1 rounds, per query the best after the first, all listed; 8 groups.  Rows: media-shape synthetic batch, every "
                   "request, every call and a callee span below every call, stitched from the true assignment.  The yardsticks read the same rows once."}
    for k, size in enumerate(args.sizes.split(",")):
        r, n = (int(x) for x in size.split("x"))
        key = "media_shape_%dx%d" % (r, n)
        doc[key] = measure(eng, r, n, args.rounds, check=k == 0)
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
