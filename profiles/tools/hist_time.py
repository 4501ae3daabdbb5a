"""Times Engine.history_push (tw_history_push, csrc/tw_hist.h) on one resident batch: the store is brought to 1x, 4x and 16x the
batch by repeated pushes of its distribution items (percentile 0: every eligible tree), and every push is recorded --
tw_get_timing slots 38, 39 (plan, merge kernel; HIP events), the bytes it moves (16 B per item held afterwards) and the share of
tw_measure_hbm_copy's rate, taken in the same run.  Beside it the only route of the code before the history to the same result:
the sort slot (23) of a tw_latency_distributions call, measured in the same run on the batches of --sizes; a store of k x the
items of size AxN is compared with the sort of size (kA)xN where that size was run too (the same number of items), otherwise
only with k times the batch's own sort, marked as scaled, not measured.  The batch is the media-shape table of
profiles/dist_time.json (conf_time.py builds it).  Writes one JSON document.

    python profiles/tools/hist_time.py --out profiles/hist_time.json
    python profiles/tools/hist_time.py --sizes 1x500,4x500 --levels 1,4 --lib <host build>    # a rehearsal without a GPU: no times worth reading
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conf_time import span_table  # noqa: E402
from traceweaver_amd import synth, traces  # noqa: E402
from traceweaver_amd.engine import Engine  # noqa: E402

PROBS = (0.5, 0.95, 0.99)
BYTES_PER_ITEM = 16                  # 8 read (from the store or from the batch), 8 written


def measure(eng, replicas, n_in, levels, rounds, check):
    units, _ = synth.make_workload(7, n_in, services=synth.MEDIA_SERVICES, replicas=replicas, concurrency=1.6)
    rows, group = span_table(units)
    eng.load(units)
    eng.run_pass1()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, 8)
    eng.stitch()
    gbps = eng.hbm_copy_gbps()
    sorts = []
    for _ in range(rounds):                                       # the route without a history: items and sort of the whole population
        eng.attribute(percentile=0.0)
        d = eng.distributions(PROBS, values=False)
        sorts.append(eng.distributions_timing())
    best_sort = min(sorts[1:] or sorts, key=lambda t: t["sort"])
    out = {"rows": len(rows[2]), "items": d.n_items, "hbm_copy_gbps": gbps, "distributions_ms": best_sort, "all_distributions_ms": sorts, "pushes": []}
    eng.history_reset()
    for k in range(1, max(levels) + 1):
        s = eng.history_push()
        t = eng.history_timing()
        moved = BYTES_PER_ITEM * int(s[1])
        out["pushes"].append({"store_x": k, "items_added": int(s[0]), "items_held": int(s[1]), "plan_ms": t["plan"], "merge_ms": t["merge"], "bytes": moved,
                              "gbps": moved / t["merge"] / 1e6 if t["merge"] > 0 else None,
                              "of_copy_rate": moved / t["merge"] / 1e6 / gbps if t["merge"] > 0 and gbps > 0 else None,
                              "capacity": eng.history_info()["capacity"]})
    out["levels"] = {str(k): out["pushes"][k - 1] for k in levels}
    if check:                                                     # the store against the restatement: k copies of the batch's items
        full = eng.distributions(PROBS)
        h = eng.history_distributions(PROBS)
        out["equals_host"] = bool(h.same_as(traces.history_host([(full, None)] * max(levels), PROBS)))
    eng.history_reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1x8000,16x8000,1x125000,16x125000",
                    help="replicas x requests per service, comma separated; the first one is checked against the host restatement")
    ap.add_argument("--levels", default="1,4,16", help="store sizes, in batches, at which a push is reported")
    ap.add_argument("--rounds", type=int, default=3, help="attribute + distributions calls for the sort slot: a warm-up and the best of the rest")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    levels = sorted(int(x) for x in args.levels.split(","))
    eng = Engine(0, lib_path=args.lib)
    doc = {"what": "tw_history_push on one MI355X: per push the HIP events of tw_get_timing slots 38, 39 (k_hist_plan; k_hist_merge), the bytes moved "
                   "(16 B per item held afterwards) and their share of hbm_copy_gbps, taken in the same run; the store holds one cohort, 8 groups (25 "
                   "segments) and is brought to 1x, 4x and 16x the batch by pushes of the same batch (percentile 0).  distributions_ms.sort is slot 23 "
                   "of a tw_latency_distributions call on that batch in the same run: the route to a sorted union without a history.  "
                   "against_sort compares a push into the k x store with the sort of as many items: measured where the size (k A)xN was run, else "
                   "k times the batch's own sort (scaled: not a measurement).  Rows: media-shape synthetic batch as in profiles/dist_time.json."}
    sizes = [tuple(int(x) for x in size.split("x")) for size in args.sizes.split(",")]

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")

    for i, (r, n) in enumerate(sizes):
        key = "media_shape_%dx%d" % (r, n)
        doc[key] = measure(eng, r, n, levels, args.rounds, check=i == 0)
        print(key, json.dumps({"items": doc[key]["items"], "sort_ms": doc[key]["distributions_ms"]["sort"], "levels": doc[key]["levels"]}), flush=True)
        write()                                                   # (what has been measured so far survives a run that is cut short)
    eng.close()
    for r, n in sizes:
        me = doc["media_shape_%dx%d" % (r, n)]
        me["against_sort"] = {}
        for k in levels:
            push, other = me["levels"][str(k)], doc.get("media_shape_%dx%d" % (k * r, n))
            row = {"merge_ms": push["merge_ms"], "plan_and_merge_ms": push["plan_ms"] + push["merge_ms"], "items_held": push["items_held"],
                   "sort_ms_scaled": k * me["distributions_ms"]["sort"]}
            if other is not None:
                row.update(sort_ms_measured=other["distributions_ms"]["sort"], sort_items=other["items"],
                           push_over_sort=row["plan_and_merge_ms"] / other["distributions_ms"]["sort"] if other["distributions_ms"]["sort"] > 0 else None)
            me["against_sort"][str(k)] = row
    write()
    if not args.out:
        print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
