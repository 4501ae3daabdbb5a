"""Times the call-order search (traceweaver_amd/order.py) on one MI355X: the k_order_bound kernel (tw_get_timing slot 31, HIP events)
and the wall clock, rounds and solves of order.infer_order over a synthetic media + hotel batch (synth.make_workload: the six media
services and the two hotel services, endpoints handed over in the order make_unit gives them).  The baseline is the route a user had
before the search existed: the reference's loop (executor.py:152-212) written around TraceWeaverGPU.solve_arrays, one call per candidate
graph, one service at a time, no bound -- order.infer_order_host with that solver.  Writes one JSON document.

    python profiles/tools/order_time.py --out profiles/order_time.json
    python profiles/tools/order_time.py --requests 200 --lib <host build>       # a rehearsal without a GPU: no times worth reading
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from traceweaver_amd import order, synth  # noqa: E402
from traceweaver_amd.engine import Engine  # noqa: E402
from traceweaver_amd.predictor import TraceWeaverGPU  # noqa: E402


def workload(n_in, concurrency):
    media, _ = synth.make_workload(7, n_in, services=synth.MEDIA_SERVICES, concurrency=concurrency)
    hotel, _ = synth.make_workload(8, n_in, services=synth.HOTEL_SERVICES, concurrency=concurrency)
    return media + hotel, list(synth.MEDIA_SERVICES) + list(synth.HOTEL_SERVICES)


def measure(args, n_in):
    units, shapes = workload(n_in, args.concurrency)
    eng = Engine(0, lib_path=args.lib)
    bound = []
    for _ in range(args.rounds + 1):
        t = time.perf_counter()
        viol = eng.order_bound(units)
        bound.append({"kernel_ms": eng.order_bound_ms(), "call_ms": (time.perf_counter() - t) * 1e3})
    runs = []
    for _ in range(args.rounds + 1):
        t = time.perf_counter()
        found = order.infer_order(eng, units)
        runs.append((time.perf_counter() - t) * 1e3)
    eng.close()
    pred = TraceWeaverGPU({}, {}, fit="device", replay_true_fit=False, lib_path=args.lib)
    base_runs = []
    for _ in range(args.rounds + 1):
        np.random.seed(10)
        t = time.perf_counter()
        base = order.infer_order_host(units, lambda u: pred.solve_arrays(u)[1]["cnt_unassigned"], use_bound=False)
        base_runs.append((time.perf_counter() - t) * 1e3)
    pred._engine.close()
    best, base_best = min(runs[1:]), min(base_runs[1:])
    return {
        "requests_per_service": n_in, "services": shapes, "concurrency": args.concurrency, "spans": int(sum(u.n_spans for u in units)),
        "order_bound": dict(min(bound[1:], key=lambda b: b["kernel_ms"]), all=bound, pairs_rejected=int(sum(int((v > 0).sum()) for v in viol))),
        "infer_order": {"total_ms": best, "rounds": found.rounds, "solves": found.solves, "all_ms": runs,
                        "equals_find_order": [bool(np.array_equal(d, u.dag)) for d, u in zip(found.dags, units)]},
        "one_solve_arrays_call_per_candidate": {"total_ms": base_best, "solves": base.solves, "all_ms": base_runs,
                                                "same_graphs_as_infer_order": bool(all(np.array_equal(a, b) for a, b in zip(base.dags, found.dags)))},
        "baseline_over_infer_order": base_best / best,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", default="1000,20000", help="requests per service, comma separated")
    ap.add_argument("--concurrency", type=float, default=1.5)
    ap.add_argument("--rounds", type=int, default=2, help="repetitions after a warm-up: the best is reported, all are listed")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    doc = {"what": "order.infer_order on one MI355X over a synthetic media + hotel batch (8 services, E in {1,1,1,1,2,4,3,2}): k_order_bound by HIP "
                   "events (tw_get_timing slot 31) and by the wall clock of the whole tw_order_bound call (uploads included); infer_order by wall "
                   "clock, stage + bound + every round (gather, load, pass 1, seeded refit, pass 2, counters), default refit; the baseline is the "
                   "same greedy loop without the bound around TraceWeaverGPU.solve_arrays (fit='device'), one call per candidate graph and "
                   "service.  --rounds + 1 repetitions each, the best after the first, all listed."}
    for n in (int(x) for x in args.requests.split(",")):
        doc["media_hotel_%d" % n] = measure(args, n)
        r = doc["media_hotel_%d" % n]
        print(n, json.dumps({"bound_kernel_ms": r["order_bound"]["kernel_ms"], "infer_ms": r["infer_order"]["total_ms"], "rounds": r["infer_order"]["rounds"],
                             "solves": r["infer_order"]["solves"], "baseline_ms": r["one_solve_arrays_call_per_candidate"]["total_ms"],
                             "baseline_solves": r["one_solve_arrays_call_per_candidate"]["solves"], "ratio": r["baseline_over_infer_order"]}), flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
