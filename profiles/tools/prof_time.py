"""Times Engine.class_profiles (tw_class_profiles, csrc/tw_prof.h) next to the two kernels that read the same rows before it, in one
process on one resident batch: tw_get_timing slots 28..30 beside slot 25 (k_sig_items and k_sig_trees: the signature stage's sweep
over the rows) and slot 18 (k_attr_reduce: the attribution's group reduction), HIP events, and the rate of tw_measure_hbm_copy.  The
batch is the media-shape table of profiles/sig_time.json (conf_time.py builds it).  Both modes, whole traces, the slowest 5 % and
every trace.  Writes one JSON document.

    python profiles/tools/prof_time.py --out profiles/prof_time.json            # 0.2 M and 52 M rows
    python profiles/tools/prof_time.py --sizes 1x2000 --lib <host build>        # a rehearsal without a GPU: no times worth reading
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


def measure(eng, replicas, n_in, rounds, check):
    units, _ = synth.make_workload(7, n_in, services=synth.MEDIA_SERVICES, replicas=replicas, concurrency=1.6)
    rows, group = span_table(units)
    eng.load(units)
    eng.run_pass1()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, 8)
    st = eng.stitch()
    out = {"rows": len(rows[2]), "trees": st.n_trees, "hbm_copy_gbps": eng.hbm_copy_gbps()}
    for pct in (0.95, 0.0):
        for mode in traces.SIGNATURE_MODES:
            runs = []
            for k in range(rounds + 1):
                a = eng.attribute(percentile=pct)                 # (drops the profile: no class_profiles call just copies)
                s = eng.signatures(mode)
                p = eng.class_profiles()
                runs.append({"profiles_ms": eng.profiles_timing(), "sig_items_ms": eng.signatures_timing()["items"],
                             "attr_reduce_ms": eng.attribute_timing()["reduce"]})
            best = min(runs[1:], key=lambda t: sum(t["profiles_ms"].values()))
            key = "%s_percentile_%g" % (mode, pct)
            out[key] = dict(best, counted_trees=p.n_counted, classes=s.n_classes, entries=p.n_entries, counted_rows=int(p.summary[2]),
                            sweep_over_sig_items_plus_attr_reduce=best["profiles_ms"]["sweep"] / (best["sig_items_ms"] + best["attr_reduce_ms"]), all=runs)
            if check:
                sig = traces.signatures_host(st, a.link, rows[3], group, 8, mode)
                host = traces.attribute_host(st, a.link, rows[4], rows[5], group, 8, pct)
                out[key]["equals_host"] = bool(p.same_as(traces.class_profiles_host(st, sig, host, a.link, rows[3], rows[4], rows[5], group)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1x8000,16x125000", help="replicas x requests per service, comma separated; the first one is checked against the host restatement")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of attribute, signatures, class_profiles per query after a warm-up: the best is reported, all are listed")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    eng = Engine(0, lib_path=args.lib)
    doc = {"what": "tw_class_profiles next to tw_trace_signatures and tw_attribute_traces on one MI355X, same batch and process: HIP events of "
                   "tw_get_timing slots 28..30 (k_prof_clear + k_prof_rows: the sweep; k_prof_trees + k_prof_classes; the copies to the host), slot 25 "
                   "(sig_items_ms: k_sig_items + k_sig_trees) and slot 18 (attr_reduce_ms: k_attr_reduce); per query --rounds + 1 rounds of attribute, "
                   "signatures and class_profiles, the best after the first, all listed; 8 groups (by service).  Rows: media-shape synthetic batch, "
                   "every request, every call and a callee span below every call.  The yardstick is the sum of the two older kernels of the same "
                   "round: the sweep reads the same rows once and reduces into more cells."}
    for k, size in enumerate(args.sizes.split(",")):
        r, n = (int(x) for x in size.split("x"))
        key = "media_shape_%dx%d" % (r, n)
        doc[key] = measure(eng, r, n, args.rounds, check=k == 0)
        print(size, json.dumps({q: {a: v[a] for a in ("counted_trees", "entries", "profiles_ms", "sig_items_ms", "attr_reduce_ms")}
                                for q, v in doc[key].items() if isinstance(v, dict)}), flush=True)
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
