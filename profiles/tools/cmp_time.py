"""Times Engine.compare_cohorts (tw_compare_cohorts, csrc/tw_cmp.h) next to the distributions it follows, in one process on one
resident batch: tw_get_timing slots 33, 34 beside slots 22..24 (HIP events).  The batch is the media-shape table of
profiles/dist_time.json (conf_time.py builds it), its traces split into two cohorts by the parity of their first service's row.
Per query (the default 5 % selection, and percentile 0: every eligible tree) the comparison of cohort 0 with cohort 1 without
and with 1000 permutations.  Writes one JSON document.

    python profiles/tools/cmp_time.py --out profiles/cmp_time.json             # 0.2 M and 13 M rows
    python profiles/tools/cmp_time.py --sizes 1x2000 --lib <host build>        # a rehearsal without a GPU: no times worth reading
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
PERMUTATIONS = (0, 1000)


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
    label = np.where(np.asarray(group) == 0, np.arange(n_rows) % 2, -1).astype(np.int32)
    eng.set_row_cohorts(label, 2)
    st = eng.stitch()
    out = {"rows": n_rows, "trees": st.n_trees}
    for tag, pct in (("percentile_0.95", 0.95), ("percentile_0", 0.0)):
        a = eng.attribute(percentile=pct)
        d = eng.distributions(PROBS, values=False)
        q = {"selected_trees": a.n_selected, "items": d.n_items, "trees_without_cohort": int(d.summary[3]), "distributions_ms": eng.distributions_timing()}
        for n_perm in PERMUTATIONS:
            runs = []
            for _ in range(rounds):
                c = eng.compare_cohorts(((0, 1),), PROBS, n_perm, seed=1)
                runs.append(eng.compare_timing())
            best = min(runs[1:] or runs, key=lambda t: t["observed"] + t["permutations"])
            both = (c.n_a > 0) & (c.n_b > 0)
            pooled = int(c.summary[2]) if n_perm else int((c.n_a + c.n_b)[both].sum())
            q["permutations_%d" % n_perm] = {
                "rows_compared": int(c.summary[0]), "pooled_items": pooled, "largest_row": int((c.n_a + c.n_b)[both].max()) if both.any() else 0,
                "compare_ms": best, "all": runs,
                "observed_over_distributions": best["observed"] / sum(q["distributions_ms"].values()),
                "walk_steps_per_ms": pooled * n_perm / best["permutations"] if n_perm and best["permutations"] > 0 else None}
            if check and pct > 0:
                want = traces.compare_cohorts_host(eng.distributions(PROBS), ((0, 1),), PROBS, min(n_perm, 8), 1)
                got = eng.compare_cohorts(((0, 1),), PROBS, min(n_perm, 8), seed=1)
                q["permutations_%d" % n_perm]["equals_host_at_8_permutations"] = bool(got.same_as(want))
        out[tag] = q
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1x8000,4x125000", help="replicas x requests per service, comma separated; the first one's 5 %% query is checked against the host restatement")
    ap.add_argument("--rounds", type=int, default=3, help="compare calls per setting: a warm-up and the best of the rest")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    eng = Engine(0, lib_path=args.lib)
    doc = {"what": "tw_compare_cohorts next to tw_latency_distributions on one MI355X, same batch and process: HIP events of tw_get_timing slots 33 (k_cmp_rank, "
                   "k_cmp_at, k_cmp_final: ranks, pool, observed statistics) and 34 (k_cmp_perm: the permutation walk) beside 22..24 of the call that built "
                   "the items; per setting --rounds calls, the best after the first, all listed.  Two cohorts (the parity of the row of a trace's first "
                   "service), 8 groups, one pair: 25 rows.  walk_steps_per_ms = pooled items x permutations / the walk's time; the walk of one "
                   "permutation is sequential, so largest_row bounds the call.  Rows: the media-shape synthetic batch of dist_time.json."}
    for k, size in enumerate(args.sizes.split(",")):
        r, n = (int(x) for x in size.split("x"))
        key = "media_shape_%dx%d" % (r, n)
        doc[key] = measure(eng, r, n, args.rounds, check=k == 0)
        print(size, json.dumps({q: {p: doc[key][q][p]["compare_ms"] for p in ("permutations_0", "permutations_1000")} for q in ("percentile_0.95", "percentile_0")}), flush=True)
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
