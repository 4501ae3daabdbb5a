"""Times Engine.signatures (tw_trace_signatures, csrc/tw_sig.h) next to the stitch it follows and the distributions' sort over the
same rows, in one process on one resident batch: tw_get_timing slots 25..27 beside slots 10..15 and 22..24 (HIP events) and the
rate of tw_measure_hbm_copy.  The batch is the media-shape table of profiles/conf_time.json and profiles/dist_time.json
(conf_time.py builds it).  Both modes, whole traces (need_flags 1).  Writes one JSON document.

    python profiles/tools/sig_time.py --out profiles/sig_time.json             # 0.2 M and 52 M rows
    python profiles/tools/sig_time.py --sizes 1x2000 --lib <host build>        # a rehearsal without a GPU: no times worth reading
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

# bytes k_sig_items needs per row: the row's number 4, kind 1, depth 4, group 4, the level written 4 and the key written 8; in mode
# "edges" a server row also reads two links 8, the kind of the rows it passes 2 and its caller's group 4
ROW_LEVELS, SERVER_ROW_EDGES = 25, 14


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
    servers = int((np.asarray(rows[3]) == 1).sum())
    st = eng.stitch()
    out = {"rows": n_rows, "trees": st.n_trees, "counts": st.counts.tolist(), "stitch_ms": eng.stitch_timing()}
    gbps = eng.hbm_copy_gbps()
    out["hbm_copy_gbps"] = gbps
    a = eng.attribute(percentile=0.0)
    eng.distributions((0.5,), None, values=False)
    out["distributions_ms"] = eng.distributions_timing()
    for mode in traces.SIGNATURE_MODES:
        runs = []
        for k in range(rounds):
            s = eng.signatures(mode, skip_flags=4 * ((rounds - k) % 2))   # (another query than the call before, the same trees -- no truth, no EXACT bit: no call just copies)
            runs.append(eng.signatures_timing())
        s = eng.signatures(mode)
        runs.append(eng.signatures_timing())
        best = min(runs[1:], key=lambda t: sum(t.values()))
        b_items = ROW_LEVELS * n_rows + (SERVER_ROW_EDGES * servers if mode == "edges" else 0)
        out[mode] = {"eligible_trees": s.n_eligible, "classes": s.n_classes, "items": int(s.summary[2]), "entries": int(s.summary[3]),
                     "signatures_ms": best, "all": runs,
                     "over_stitch_group": sum(best.values()) / out["stitch_ms"]["group"],
                     "over_distributions_items_and_sort": sum(best.values()) / (out["distributions_ms"]["items"] + out["distributions_ms"]["sort"]),
                     "items_kernel": {"bytes": b_items, "bytes_per_row": b_items / float(n_rows), "gbps": b_items / best["items"] / 1e6 if best["items"] > 0 else None,
                                      "of_copy_rate": b_items / best["items"] / 1e6 / gbps if best["items"] > 0 else None},
                     "items_per_ms": int(s.summary[2]) / sum(best.values()) if sum(best.values()) > 0 else None}
        if check:
            want = traces.signatures_host(st, a.link, rows[3], group, 8, mode)
            out[mode]["equals_host"] = bool(s.same_as(want))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1x8000,16x125000", help="replicas x requests per service, comma separated; the first one is checked against the host restatement")
    ap.add_argument("--rounds", type=int, default=4, help="signatures calls per mode before the one that is reported with them: a warm-up and the best of the rest")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    eng = Engine(0, lib_path=args.lib)
    doc = {"what": "tw_trace_signatures next to tw_stitch_traces and tw_latency_distributions on one MI355X, same batch and process: HIP events of "
                   "tw_get_timing slots 25..27 (items and levels; segmented sort of the large trees, LDS sort, run lengths and hash; hash sort, classes "
                   "and per-class reduction), 10..15 and 22..24; per mode --rounds + 1 calls with alternating queries, the best after the first, all "
                   "listed; 8 groups (by service), no ground truth set, no comparison.  Rows: media-shape synthetic batch, every request, every call "
                   "and a callee span below every call.  The yardsticks are stitch_ms.group (k_stitch_group: the same rows, a rank sort per tree), "
                   "distributions_ms items + sort at percentile 0 (sweeps and a radix sort over the same rows) and hbm_copy_gbps, taken in the same run."}
    for k, size in enumerate(args.sizes.split(",")):
        r, n = (int(x) for x in size.split("x"))
        key = "media_shape_%dx%d" % (r, n)
        doc[key] = measure(eng, r, n, args.rounds, check=k == 0)
        print(size, json.dumps({m: {a: doc[key][m][a] for a in ("classes", "items", "signatures_ms", "over_stitch_group", "over_distributions_items_and_sort")}
                                for m in traces.SIGNATURE_MODES}), flush=True)
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
