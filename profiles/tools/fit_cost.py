"""What one fit of the refit costs when it has a CU to itself: a batch of at most 64 identical gap rows (fewer than there are CUs, so no
two workgroups of a launch share one) of 100 000 samples -- short rows of ~1 200 distinct values, then long rows of ~10 000, the two
kinds of the headline batch (profiles/HISTORY.md, round 13) -- is refitted once under `rocprofv3 --kernel-trace --stats`, and the
durations of the fit kernels are read from the trace: with every fit on a CU of its own, a launch lasts as long as its longest fit.

    python profiles/tools/fit_cost.py [--out DIR]            both row types, one profiled child process each
    python profiles/tools/fit_cost.py --rows short|long      the refit alone (what the profiled process runs)

The rows are set with Engine.set_gaps on a few copies of a small synthetic unit: no pass runs."""
import argparse
import csv
import glob
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DISTINCT = {"short": 1200, "long": 10000}
N, MAX_ROWS = 100000, 64


def refit(kind):
    from traceweaver_amd import synth
    from traceweaver_amd.engine import Engine
    from traceweaver_amd.predictor import reference_fit_order

    u, _ = synth.make_unit(7, N, shape="chain3", concurrency=1.6, granularity_us=1)
    scored = reference_fit_order(u, u.key_rank)
    units = [u] * max(1, MAX_ROWS // len(scored))
    rng = np.random.RandomState(3)
    # a lognormal body like a service's latencies, cut to the wanted number of distinct integer microseconds
    x = np.round(rng.lognormal(6.0 if kind == "short" else 8.6, 0.45, u.n_in))
    vals = np.unique(x)
    if len(vals) > DISTINCT[kind]:   # (the samples beyond the first values are dropped and the row is filled up with the others again)
        x = np.resize(x[x <= vals[DISTINCT[kind] - 1]], u.n_in)
    g = np.full((u.nslot, u.n_in), np.nan)
    g[scored] = x
    eng = Engine(0)
    eng.load(units)
    eng.set_gaps([g] * len(units))
    eng.fit_mixtures(seed=5)
    hits, misses = eng.fit_spec()
    n = eng.mixtures()[0][0]
    print("%s rows: %d rows of %d samples, %d distinct values; selected count %d; %d hits, %d misses; refit %.3f ms" %
          (kind, len(units) * len(scored), u.n_in, len(np.unique(x)), int(n[scored[0]]), hits, misses, eng.timing()["fit"]), flush=True)
    eng.close()


def launches(directory):
    f = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(f)) if "k_fit_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"].replace("tw::", "").replace("void ", "").split("(")[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
            for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=sorted(DISTINCT), default=None)
    ap.add_argument("--out", default="out/fit_cost")
    args = ap.parse_args()
    if args.rows:
        refit(args.rows)
        return 0
    for kind in ("short", "long"):
        d = os.path.join(args.out, kind)
        rc = subprocess.call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--",
                              sys.executable, os.path.abspath(__file__), "--rows", kind], timeout=240)
        if rc != 0:
            print("%s rows: the profiled run ended with status %d" % (kind, rc))
            return rc
        for name, ms in launches(d):
            print("  %-18s %8.3f ms" % (name, ms))
    return 0


if __name__ == "__main__":
    sys.exit(main())
