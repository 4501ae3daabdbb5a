#!/usr/bin/env python3
"""Command-line surface of the reference's executor (executor.py:38-74) for predictor 10, end to end on the GPU:

    python -m traceweaver_amd.executor --relative_path data/hotel_reservation/hotel_load100/ --compressed 0 \\
        --cache_rate 0 --fix 2 --test_name hotel_test --load_level 100 --compress_factor 1 --repeat_factor 1 \\
        --execute_parallel 0 --results_directory results/ --clear_cache 1 --predictor_indices "10"

Same flags, same result files (executor.py:1235-1244): `accuracy_*` ({method: end-to-end %, method+"TopK": ...}),
`process_acc_*` ({(method, process_id): accuracy}), `confidence_scores_*` ({service: [accuracy, not_best_count,
requests]}), `bin_acc_*` ({method: [(percentile, accuracy, response time ms)]}, helpers/utils.py:187-214) and
`e2e_*` (true / predicted end-to-end traces; as lists of (trace id, span id) keys ordered by start time -- the
reference pickles its own Span objects there).  Everything between reading the directory and writing the files runs
in libtwgpu.so: native ingest (tw_corpus_*), both passes of every service in one batch, device refit, device
accuracy reductions.

Indices 3 (WAP5), 4 (FCFS) and 7 (vPath) run on the resident table as well (csrc/tw_baselines.h; identical to the
reference's classes, also on load-scaled units; skip-mode services and index 5, ArrivalOrder, as host code:
traceweaver_amd/baselines.py) and add their columns to the same files --
`exps/exp1`'s and `exps/exp5`'s "3,4,7,10" run as they are.
`--compress_factor N` (N > 1) applies the reference's load scaling (helpers/transforms.py:10-40, executor.py:1086-1097,
1146-1148) to every service before it is solved: per-service load factor max(1, ceil(N / #replicas)) with the replica
table read from data/misc/service_to_replica_new.pickle under the project root (executor.py:912), timestamps handed to
the engine as exact images of the reference's floats (traceweaver_amd/transforms.py).  `--repeat_factor` is accepted and,
as in the reference (repeat_change_spans never reads it), only shows up in the result file names.
`--cache_rate r` (r > 0, exps/exp2) injects cache hits into the service named "frontend" like the reference
(executor.py:1150-1152, helpers/transforms.py:153-238 = traceweaver_amd/skipmode.py) and solves it in skip mode on the device.
What it does not do (and says so instead of approximating): the other predictor indices (the older TraceWeaver
variants 0-2, 6, 8, 9), --cache_rate together with --compress_factor > 1, --parallel / --instrumented, tar archives
(--compressed 1).  For those keep the reference's executor and register the predictor.
The mixture refit between the passes is the reference's own procedure (traceweaver_v3.py:764-786) on the GPU (csrc/tw_fit.h).
`--fit device` (default) feeds its k-means++ seedings the doubles numpy's global RNG would hand scikit-learn at that point of
a reference run started with np.random.seed(--seed), service by service in the reference's order -- incl. the reseeding
np.random.seed(10) the reference performs when it reaches the service named "frontend" (create_cache_hits runs for it at
every cache rate, executor.py:1150-1152, helpers/transforms.py:155) -- so a seeded run reproduces a seeded reference run;
`--fit sklearn` runs scikit-learn itself on the host at the same place (cross-check); `--fit device-batch` solves all
services in one batch with draws from the engine's own MT19937(--seed): the same procedure on another random stream, as an
unseeded reference run is (SURVEY.md hazard H9).
"""
import argparse
import os
import pickle
import sys
import time

import numpy as np

METHOD = "MaxScoreBatchSubsetWithSkips"   # predictors[10] (executor.py:888-900)
NA = ("NA", "NA")


def parse_args(argv=None):
    q = lambda s: str(s).strip("'")   # the reference declares these with type=ascii and strips the quotes again
    ap = argparse.ArgumentParser(description="Map incoming and outgoing spans at each service (MI355X engine).")
    ap.add_argument("--relative_path", type=q, default=None)
    ap.add_argument("--absolute_path", type=q, default=None)
    ap.add_argument("--compressed", type=int, default=0, choices=[0, 1])
    ap.add_argument("--load_level", type=int, default=0)
    ap.add_argument("--test_name", type=q, default="test")
    ap.add_argument("--parallel", type=int, default=0, choices=[0, 1])
    ap.add_argument("--instrumented", type=int, default=0, choices=[0, 1])
    ap.add_argument("--cache_rate", type=float, required=True)
    ap.add_argument("--fix", type=int, required=True)
    ap.add_argument("--repeat_factor", type=int, default=1)
    ap.add_argument("--compress_factor", type=float, default=1)
    ap.add_argument("--execute_parallel", type=int, default=1)
    ap.add_argument("--results_directory", type=q, required=True)
    ap.add_argument("--clear_cache", type=int, default=0)
    ap.add_argument("--predictor_indices", type=str, default="")
    # additions (defaults keep the reference's behaviour)
    ap.add_argument("--project_root", type=q, default=os.getcwd(), help="what --relative_path is relative to")
    ap.add_argument("--max_traces", type=int, default=1001, help="the reference's literal limit (executor.py:873); 0 = all")
    ap.add_argument("--replicas_file", type=q, default=None,
                    help="pickle {service: [replica ids]} for --compress_factor > 1 (default: data/misc/service_to_replica_new.pickle under --project_root, executor.py:912)")
    ap.add_argument("--span_cache", type=int, default=0, choices=[0, 1],
                    help="1: keep the parsed span table of the trace directory in it (tw_span_table.bin) and start from it next time; "
                         "--clear_cache 1 rebuilds it, as it does the reference's file-order cache.  Off by default: it writes into "
                         "the data directory")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--fit", default="device", choices=["device", "device-batch", "sklearn"],
                    help="mixture refit between the passes: the reference's procedure (traceweaver_v3.py:764-786) in every case.  'device' "
                         "(default) = on the GPU, service by service in the reference's order, k-means++ draws replayed from numpy's global "
                         "RNG seeded by --seed: reproduces a reference run started with np.random.seed(seed) (SURVEY.md hazard H9).  "
                         "'sklearn' = scikit-learn on the host at the same place (cross-check; the passes still run on the GPU).  "
                         "'device-batch' = all services in one batch, draws from the engine's own MT19937(seed): fastest")
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--allow_partial", type=int, default=0, choices=[0, 1],
                    help="go on when services of the corpus cannot be solved here (skip mode, < 2 requests, cyclic call order); they are "
                         "recorded under 'left_out' in the confidence_scores pickle.  Default: stop, because the accuracy files would "
                         "otherwise count those services as right")
    ap.add_argument("--stitch_out", type=q, default=None,
                    help="write the traces predictor 10's assignments make together to this .npz (traceweaver_amd/traces.py: the per-service "
                         "parent arrays joined with the observed hops on the GPU, tw_stitch_traces) and print their counts.  Default: off, "
                         "nothing changes")
    ap.add_argument("--attribute_out", type=q, default=None,
                    help="answer the reference's delay-culprit query (src/query_engine/delay_culprit.py) on the stitched traces on the GPU "
                         "(tw_attribute_traces: critical paths, per-service totals over the slowest traces), write the result to this .npz "
                         "and print the culprit.  Stitches whether or not --stitch_out is given.  Default: off, nothing changes")
    ap.add_argument("--query_percentile", type=float, default=0.95, help="--attribute_out: the latency bracket, traces from this quantile on")
    ap.add_argument("--query_after", type=int, default=None, help="--attribute_out: only traces whose root starts at or after this time (us)")
    ap.add_argument("-v", "--verbose", action="store_true",
                    help="--attribute_out: print the same figures taken from the true traces; --confidence_out: print the calibration table; "
                         "--latency_out: print the culprit's quantiles next to its mean")
    ap.add_argument("--latency_out", type=q, default=None,
                    help="write the latency distributions behind the delay-culprit query to this .npz (tw_latency_distributions: per service "
                         "the sorted span latencies, self times and critical-path times of the selected traces, and the traces' latencies, "
                         "with counts, sums and quantiles -- the lists delay_culprit.py writes).  Needs --attribute_out's conditions and runs "
                         "its query.  Default: off, nothing changes")
    ap.add_argument("--quantiles", type=q, default="0.5,0.95,0.99", help="--latency_out: the quantiles, comma-separated, each in [0, 1]")
    ap.add_argument("--cohort_service", type=q, default=None,
                    help="--latency_out: split the traces into cohorts by the operation of this service's span in them (the smallest "
                         "operation index where a trace holds several); traces without a span of the service are left out")
    ap.add_argument("--compare_out", type=q, default=None,
                    help="compare the cohorts of --cohort_service pair by pair on the device (tw_compare_cohorts: per service and metric the "
                         "two-sample KS gap, the Mann-Whitney U, the shifts of --quantiles (at most 8) and, with --permutations, a permutation "
                         "test of each), write the result to this .npz and print the culprit's span latency per pair.  Needs --latency_out "
                         "and --cohort_service.  Default: off, nothing changes")
    ap.add_argument("--compare_pairs", type=q, default="0,1", help="--compare_out: the pairs of cohorts a,b, separated by semicolons (0,1;0,2)")
    ap.add_argument("--permutations", type=int, default=0, help="--compare_out: permutations per compared segment, at most 65536 (0: no test)")
    ap.add_argument("--compare_seed", type=int, default=0, help="--compare_out: the seed of the permutations")
    ap.add_argument("--history", type=q, default=None,
                    help="--latency_out: keep this run's distributions in a store across runs (tw_history_push): the file is read into "
                         "the device history if it exists (tw_history_merge), the run's sorted values are merged in on the device and the "
                         "store is written back.  The store's services must be this run's.  Default: off, nothing changes")
    ap.add_argument("--history_cohort", type=int, default=0, help="--history: the run's cohort c goes to cohort K + c of the store (default 0)")
    ap.add_argument("--history_compare_out", type=q, default=None,
                    help="--history: compare cohorts of the store pair by pair on the device (tw_history_compare: one run against another), "
                         "with --compare_pairs, --permutations, --compare_seed and --quantiles read as for --compare_out, and write the "
                         "result to this .npz")
    ap.add_argument("--signatures_out", type=q, default=None,
                    help="group the traces by call-graph signature on the device (per level the services seen there, the reference's "
                         "AssignCGSignature / FindUniqueCGs): the signatures of the true traces are kept as the reference set, those of "
                         "the predicted traces compared with them; write both and the shape accuracy (the share of whole traces with "
                         "the true call graph) to this .npz and print the most frequent call graphs.  Needs --stitch_out's conditions")
    ap.add_argument("--signature_mode", type=q, default="levels", choices=("levels", "edges"),
                    help="--signatures_out: levels = the services per level; edges = the caller -> callee edges per level")
    ap.add_argument("--profiles_out", type=q, default=None,
                    help="the aggregate trace of every call graph (tw_class_profiles): per entry of the call-graph signatures "
                         "(--signature_mode) the rows, durations, self and critical-path times and start offsets over the traces of that "
                         "shape which the delay-culprit query selects (--query_percentile, --query_after), for the predicted and for the "
                         "true traces; write both to this .npz and print the largest classes with the call that holds most of their "
                         "critical path.  Needs --stitch_out's conditions")
    ap.add_argument("--class_history", type=q, default=None,
                    help="--profiles_out or --signatures_out: keep this run's call graphs in a catalogue across runs "
                         "(tw_class_history_push): the file is read into the device catalogue if it exists (tw_class_history_merge), the "
                         "predicted traces' classes are matched against it (which shapes are new), added on the device -- with "
                         "--profiles_out their profiles too -- and the store is written back.  The store's services and signature mode "
                         "must be this run's.  Default: off, nothing changes")
    ap.add_argument("--class_history_epoch", type=int, default=0, help="--class_history: the label of this run (first / last epoch per call graph)")
    ap.add_argument("--trace_filter", type=q, default=None,
                    help="select the stitched traces by a predicate on the device (tw_filter_traces) before --attribute_out, --latency_out, "
                         "--compare_out, --history, --signatures_out, --profiles_out and --class_history, which then work on the whole traces "
                         "that match: terms separated by |, a term's clauses by &, a leading ! negates; a clause is SUBJECT followed by >=V, "
                         "<=V, ==V or `in LO..HI` (integers, us) with SUBJECT one of latency, rows, start, class, METRIC[.REDUCE][SERVICE] or "
                         "METRIC[.REDUCE][CALLER>SERVICE] -- METRIC one of count, span, self, path, onpath, REDUCE one of sum, min, max, "
                         "SERVICE * = any counted service, CALLER - = no caller; e.g. 'latency>=20000 & !count[cache]>=1 | span.max[search]>=5000'.  "
                         "At most 16 clauses in 8 terms.  Needs --stitch_out's conditions.  Default: off, nothing changes")
    ap.add_argument("--traces_out", type=q, default=None,
                    help="extract reconstructed traces on the device (tw_extract_traces) after the other requested stages and write them into this "
                         "directory: every trace in pre-order with its parents, with self / path times where --attribute_out or --profiles_out "
                         "left an attribution.  Selected by one of --traces_top (default: 20), --traces_quantiles, --traces_matched among the "
                         "whole traces of the predicted forest.  Needs --stitch_out's conditions.  Default: off, nothing changes")
    ap.add_argument("--traces_top", type=int, default=None, help="--traces_out: the N slowest whole traces (0: all of them)")
    ap.add_argument("--traces_quantiles", type=q, default=None, help="--traces_out: the exemplars, the traces at these quantiles of the latency, e.g. 0.5,0.99 (at most 32)")
    ap.add_argument("--traces_matched", type=int, default=0, help="--traces_out: 1 = every trace --trace_filter matched, in tree order (needs --trace_filter)")
    ap.add_argument("--traces_format", type=q, default="jaeger", choices=("jaeger", "npz"),
                    help="--traces_out: jaeger = one Jaeger JSON file per trace, in the shape the corpus came in, which a trace viewer opens; npz = one traces.npz")
    ap.add_argument("--filter_out", type=q, default=None, help="--trace_filter: write the matched traces, the clauses' values and counts to this .npz")
    ap.add_argument("--confidence_out", type=q, default=None,
                    help="score the stitched traces by confidence on the GPU (tw_score_traces: per request the margin between the selected "
                         "tuple and the best other one, per trace the weakest decision, a calibration table against ground truth), write "
                         "the result to this .npz and print the counts.  Needs --stitch_out's conditions and --fit device-batch: the "
                         "decisions are those of one batch resident on the device.  Default: off, nothing changes")
    ap.add_argument("--min_margin", type=float, default=0.0,
                    help="--confidence_out: a trace is confident when every decision in it is the best of its list by at least this margin")
    ap.add_argument("--query_confident", type=int, default=0, choices=[0, 1],
                    help="1: --attribute_out asks for whole AND confident traces only (needs --confidence_out)")
    ap.add_argument("--infer_order", type=int, default=0, choices=[0, 1],
                    help="1: solve every service under a call-order graph inferred from its spans alone (the reference's "
                         "FindConstraintsUsingFit, executor.py:152-212, as traceweaver_amd/order.py runs it: all services of the run in one "
                         "batch per candidate round) instead of FindOrder's, which reads the true assignments; prints per service whether "
                         "the two graphs are equal (the reference's cg_booleans).  Not with --cache_rate > 0 or --compress_factor > 1.  "
                         "Default: off, nothing changes")
    ap.add_argument("--engine_library", type=q, default=None, help=argparse.SUPPRESS)   # tests: host-emulation build
    args = ap.parse_args(argv)
    if args.relative_path is None and args.absolute_path is None:
        ap.error("At least one of --relative_path and --absolute_path is required")
    return args


BASELINES = {3: "WAP5", 4: "FCFS", 5: "ArrivalOrder", 7: "vPath"}   # predictors[3], [4], [5], [7] (executor.py:888-900), host code like the reference's


def requested(args):
    idx = [int(x) for x in args.predictor_indices.split(",") if x.strip() != ""]
    return idx if idx else [10]


def quantiles_of(args):
    """--quantiles as a list of floats, None if it is malformed."""
    try:
        probs = [float(x) for x in args.quantiles.split(",") if x.strip() != ""]
    except ValueError:
        return None
    return probs if 0 < len(probs) <= 32 and all(0.0 <= p <= 1.0 for p in probs) else None


def pairs_of(args):
    """--compare_pairs as a list of (a, b), None if it is malformed (the cohorts' range is checked once their number is known)."""
    try:
        pairs = [tuple(int(x) for x in part.split(",")) for part in args.compare_pairs.split(";") if part.strip() != ""]
    except ValueError:
        return None
    return pairs if 0 < len(pairs) <= 64 and all(len(p) == 2 and p[0] != p[1] and min(p) >= 0 for p in pairs) else None


def unsupported(args):
    problems = []
    bad = [i for i in requested(args) if i != 10 and i not in BASELINES]
    if bad:
        problems.append("--predictor_indices %s (index 10 runs on the GPU, %s as host baselines; not %s)"
                        % (args.predictor_indices, sorted(BASELINES), bad))
    if args.compressed:
        problems.append("--compressed 1")
    if args.parallel or args.instrumented:
        problems.append("--parallel / --instrumented")
    if args.stitch_out and (10 not in requested(args) or args.cache_rate > 0):
        problems.append("--stitch_out without predictor 10 or with --cache_rate > 0 (a skip-mode service is solved in a batch of its own)")
    if args.attribute_out and (10 not in requested(args) or args.cache_rate > 0):
        problems.append("--attribute_out without predictor 10 or with --cache_rate > 0 (it works on the stitched traces, see --stitch_out)")
    if args.attribute_out and not 0.0 <= args.query_percentile < 1.0:
        problems.append("--query_percentile outside [0, 1)")
    if args.latency_out and (10 not in requested(args) or args.cache_rate > 0):
        problems.append("--latency_out without predictor 10 or with --cache_rate > 0 (it works on the stitched traces, see --stitch_out)")
    if args.latency_out and not args.attribute_out and not 0.0 <= args.query_percentile < 1.0:
        problems.append("--query_percentile outside [0, 1)")
    if args.latency_out and quantiles_of(args) is None:
        problems.append("--quantiles %s (up to 32 comma-separated numbers in [0, 1])" % args.quantiles)
    if args.cohort_service and not args.latency_out:
        problems.append("--cohort_service without --latency_out")
    if args.compare_out and not (args.latency_out and args.cohort_service):
        problems.append("--compare_out without --latency_out and --cohort_service (it compares the cohorts of that service)")
    if args.compare_out and pairs_of(args) is None:
        problems.append("--compare_pairs %s (up to 64 pairs a,b of different cohorts, separated by semicolons)" % args.compare_pairs)
    if args.compare_out and not 0 <= args.permutations <= 65536:
        problems.append("--permutations outside [0, 65536]")
    if args.compare_out and args.compare_seed < 0:
        problems.append("--compare_seed below 0")
    if args.compare_out and len(quantiles_of(args) or ()) > 8:
        problems.append("--compare_out with more than 8 --quantiles")
    if args.history and not args.latency_out:
        problems.append("--history without --latency_out (it keeps that run's distributions)")
    if args.history_cohort < 0 or (args.history_cohort != 0 and not args.history):
        problems.append("--history_cohort below 0 or without --history")
    if args.history_compare_out and not (args.history and args.latency_out):
        problems.append("--history_compare_out without --history and --latency_out (it compares cohorts of that store)")
    if args.history_compare_out and pairs_of(args) is None:
        problems.append("--compare_pairs %s (up to 64 pairs a,b of different cohorts, separated by semicolons)" % args.compare_pairs)
    if args.history_compare_out and not 0 <= args.permutations <= 65536:
        problems.append("--permutations outside [0, 65536]")
    if args.history_compare_out and args.compare_seed < 0:
        problems.append("--compare_seed below 0")
    if args.history_compare_out and len(quantiles_of(args) or ()) > 8:
        problems.append("--history_compare_out with more than 8 --quantiles")
    if args.signatures_out and (10 not in requested(args) or args.cache_rate > 0):
        problems.append("--signatures_out without predictor 10 or with --cache_rate > 0 (it works on the stitched traces, see --stitch_out)")
    if args.profiles_out and (10 not in requested(args) or args.cache_rate > 0):
        problems.append("--profiles_out without predictor 10 or with --cache_rate > 0 (it works on the stitched traces, see --stitch_out)")
    if args.class_history and not (args.profiles_out or args.signatures_out):
        problems.append("--class_history without --profiles_out or --signatures_out (it keeps that run's call graphs)")
    if args.class_history_epoch != 0 and not args.class_history:
        problems.append("--class_history_epoch without --class_history")
    if args.profiles_out and not 0.0 <= args.query_percentile < 1.0:
        problems.append("--query_percentile outside [0, 1)")
    if args.trace_filter and (10 not in requested(args) or args.cache_rate > 0):
        problems.append("--trace_filter without predictor 10 or with --cache_rate > 0 (it works on the stitched traces, see --stitch_out)")
    if args.traces_out and (10 not in requested(args) or args.cache_rate > 0):
        problems.append("--traces_out without predictor 10 or with --cache_rate > 0 (it works on the stitched traces, see --stitch_out)")
    selectors = [k for k, on in (("--traces_top", args.traces_top is not None), ("--traces_quantiles", args.traces_quantiles is not None), ("--traces_matched", args.traces_matched)) if on]
    if selectors and not args.traces_out:
        problems.append("%s without --traces_out" % selectors[0])
    if len(selectors) > 1:
        problems.append("%s: one selector of --traces_out at a time" % " and ".join(selectors))
    if args.traces_top is not None and args.traces_top < 0:
        problems.append("--traces_top is negative")
    if args.traces_matched and not args.trace_filter:
        problems.append("--traces_matched 1 without --trace_filter")
    if args.traces_quantiles is not None:
        try:
            probs = [float(x) for x in args.traces_quantiles.split(",")]
            if not probs or len(probs) > 32 or not all(0.0 <= p <= 1.0 for p in probs):
                raise ValueError
        except ValueError:
            problems.append("--traces_quantiles %s: 1 to 32 numbers in [0, 1], separated by commas" % args.traces_quantiles)
    if args.filter_out and not args.trace_filter:
        problems.append("--filter_out without --trace_filter")
    if args.confidence_out and (10 not in requested(args) or args.cache_rate > 0):
        problems.append("--confidence_out without predictor 10 or with --cache_rate > 0 (it works on the stitched traces, see --stitch_out)")
    if args.confidence_out and args.fit != "device-batch":
        problems.append("--confidence_out without --fit device-batch (the decisions are read from the batch resident on the device; the "
                        "other fits solve the services one after the other)")
    if args.confidence_out and args.min_margin != args.min_margin:
        problems.append("--min_margin nan")
    if args.infer_order and (args.cache_rate > 0 or args.compress_factor > 1):
        problems.append("--infer_order 1 with --cache_rate > 0 or --compress_factor > 1 (the search covers neither skip-mode nor load-scaled services)")
    if args.query_confident and not (args.confidence_out and args.attribute_out):
        problems.append("--query_confident 1 without --confidence_out and --attribute_out")
    return problems


def scale_load(units, args, trace_id, corpus):
    """Load scaling of every unit (helpers/transforms.py:10-40) with the per-service factor of executor.py:1086-1097."""
    from . import transforms
    from .ingest import IngestedUnit

    path = args.replicas_file or os.path.join(args.project_root, "data/misc/service_to_replica_new.pickle")
    if not os.path.exists(path):
        raise SystemExit("--compress_factor %g needs the replica table %s ({service: [replica ids]}, executor.py:912)" % (args.compress_factor, path))
    with open(path, "rb") as f:
        replicas = pickle.load(f)
    out, factors, ranks = [], [], []
    for u in units:
        owner = u.service if u.service in replicas else corpus.loop_origin(u.service)   # "...-loop" stand-ins: executor.py:1092-1096
        if owner not in replicas:
            raise SystemExit("service %s is not in the replica table %s (the reference stops here too, executor.py:1098-1101)" % (u.service, path))
        factor = transforms.load_factor(args.compress_factor, len(replicas[owner]))
        print("Process: %s  replicas: %d  dynamic load factor: %d" % (u.service, len(replicas[owner]), factor))
        keys = [trace_id(t) for t in u.in_trace]
        s = transforms.compress_unit(u.arrays, u.true_parent, factor, trace_key=keys)
        rank = np.empty(len(keys), dtype=np.int32)
        rank[np.argsort(np.asarray(keys), kind="stable")] = np.arange(len(keys), dtype=np.int32)
        factors.append(factor)
        ranks.append(rank)
        out.append(IngestedUnit(s.arrays, s.true_parent, u.in_trace[s.in_perm], u.service, u.in_ep, u.out_eps, u.in_rows[s.in_perm],
                                [r[p] for r, p in zip(u.out_rows, s.out_perm)], u.process_id))
    return out, factors, ranks


def infer_order(units, args):
    """--infer_order 1: the call-order graph of every service from its spans alone, all services in one batch per round
    (traceweaver_amd/order.py); every unit is handed on with its endpoints in the topological order of the inferred graph.
    Returns (units, cg_booleans): per service whether the inferred graph equals FindOrder's (executor.py:205-206)."""
    from . import order
    from .engine import Engine
    from .ingest import IngestedUnit

    keyed = [order.key_order_unit(u.arrays) for u in units]
    eng = Engine(args.device, lib_path=args.engine_library)
    t0 = time.time()
    found = order.infer_order(eng, [k[0] for k in keyed], seeds=[args.seed + j for j in range(len(units))])
    eng.close()
    print("Inferred the call order of %d services in %.2f s: %d rounds, %d candidate graphs solved" % (len(units), time.time() - t0, found.rounds, found.solves))
    out, same = [], []
    for j, (u, (ku, perm)) in enumerate(zip(units, keyed)):
        same.append(bool(np.array_equal(found.dags[j], u.arrays.dag[np.ix_(perm, perm)])))
        how = {h: sum(1 for x in found.logs[j] if x[2] == h) for h in order.DECIDED_BY}
        print("Call graph of service %s: %s (%d edges; pairs decided by solve %d, bound %d, reverse %d, cycle %d)" % (
            u.service, "identical to FindOrder's" if same[-1] else "differs from FindOrder's", int(found.dags[j].sum()),
            how["solve"], how["bound"], how["reverse"], how["cycle"]))
        arrays = order.permuted_unit(ku, found.dags[j])
        src = [perm[k] for k in arrays.key_rank.tolist()]           # the ingested unit's endpoint at every new position
        out.append(IngestedUnit(arrays, u.true_parent[src], u.in_trace, u.service, u.in_ep, [u.out_eps[e] for e in src], u.in_rows,
                                [u.out_rows[e] for e in src], u.process_id))
    return out, same


CONFIDENCE_EDGES = (0.0, 1.0, 2.0, 5.0)   # --confidence_out: bucket edges of the calibration table (differences of log scores)


def confidence_out(args, eng, st):
    """--confidence_out: the decisions of the resident pass over the forest just stitched from it."""
    from . import traces

    c = eng.score_traces(args.min_margin, CONFIDENCE_EDGES)
    traces.write_confidence_npz(args.confidence_out, c, st)
    print("Trace confidence: %d of %d scored traces confident (margin >= %g); %d of %d decisions not best, %d unassigned"
          % (c.n_confident, c.n_scored, args.min_margin, c.summary[3], c.summary[2], c.summary[4]))
    if args.verbose:
        for row in c.table():
            span = "some decision not best" if row["bucket"] == 0 else "min margin in [%g, %g)" % (row["from"], row["to"])
            print("    %-32s %7d whole traces, %7d exact, %8d decisions" % (span, row["trees"], row["exact"], row["decisions"]))


def trace_filter(args, eng, names, report=False):
    """--trace_filter on the forest just stitched (the row groups are set): the times and the classes its clauses read computed once,
    then the filter over the whole traces.  Returns the flag the later stages add to need_flags: traces.MATCH, 0 without the option.
    report: the predicted forest's first filter -- print the counts and write --filter_out."""
    from . import traces

    if not args.trace_filter:
        return 0
    try:
        clauses = traces.parse_filter(args.trace_filter, names)
    except ValueError as ex:
        raise SystemExit("--trace_filter: %s" % ex)
    if any(c[1] >= 4 and c[4] >= 2 for c in clauses):
        eng.attribute()                                           # (of the whole traces: its query does not name the bit, the filter leaves it)
    if any(c[1] == 3 for c in clauses):
        eng.signatures(args.signature_mode)
    f = eng.filter_traces(clauses, traces.WHOLE, 0)
    if report:
        if args.filter_out:
            traces.write_filter_npz(args.filter_out, f, names)
        print("Trace filter: %d of %d whole traces match %s" % (f.n_matched, f.n_eligible, traces.format_filter(clauses, names)))
        for row in f.table([str(x) for x in names]) if args.verbose else ():
            print("    %-8s %-48s holds on %d traces" % ("clause %d" % row["clause"] if "clause" in row else "term %d" % row["term"], row["text"], row["trees"]))
    return traces.MATCH


def traces_out(args, eng, corpus, table, pass_):
    """--traces_out: reconstructed traces of the predicted forest, extracted on the device after the other stages and written as Jaeger
    JSON or as one .npz.  The stages before it leave the predicted forest behind, except --attribute_out / --latency_out with -v
    alone (their last stitch is the true forest): then the forest, the filter and the query are made again."""
    import os

    from . import traces

    group, names = traces.groups_from_table(table, corpus)
    names = [str(x) for x in names]
    attributed = bool(args.attribute_out or args.latency_out)
    if attributed and args.verbose and not (args.signatures_out or args.profiles_out):
        eng.stitch(pass_)
        match = trace_filter(args, eng, names)
        eng.attribute(percentile=args.query_percentile, start_min=args.query_after, need_flags=traces.WHOLE | match)
    elif not (args.trace_filter or attributed or args.signatures_out or args.profiles_out):
        eng.set_row_groups(group, len(names))                     # (nobody has set them)
    need = traces.WHOLE | (traces.MATCH if args.traces_matched else 0)
    if args.traces_matched:
        x = eng.extract_traces("top", "tree", 0, need_flags=need)
    elif args.traces_quantiles is not None:
        x = eng.extract_traces("quantiles", probs=[float(p) for p in args.traces_quantiles.split(",")], need_flags=need)
    else:
        x = eng.extract_traces("top", "slowest", 20 if args.traces_top is None else args.traces_top, need_flags=need)
    os.makedirs(args.traces_out, exist_ok=True)
    if args.traces_format == "npz":
        traces.write_extracted_npz(os.path.join(args.traces_out, "traces.npz"), x, names)
    else:
        traces.write_jaeger(args.traces_out, x, corpus, table)
    print("Extracted traces: %d of %d eligible, %d rows%s -> %s" % (x.n_trees, x.n_eligible, x.summary[2], ", with self and path times" if x.has_times else "", args.traces_out))
    for j in range(min(3, x.n_trees) if args.verbose else 0):
        print(x.render(j, names))


def stitch_out(args, corpus, units, table, parents, n_traces, total, right, solved=None):
    """--stitch_out: all services in one batch, the assignments they were given, the span table's rows -> traces on the device.
    solved: the engine that still holds the batch and the pass these assignments came from (--confidence_out)."""
    from . import traces
    from .engine import Engine

    if solved is not None:
        eng = solved
        eng.set_span_rows(*traces.rows_from_units(units, table))
        st = eng.stitch(2)
        confidence_out(args, eng, st)
    else:
        eng = Engine(args.device, lib_path=args.engine_library)
        eng.load([u.arrays for u in units])
        eng.set_truth([u.true_parent for u in units], [u.in_trace for u in units], n_traces)
        eng.set_span_rows(*traces.rows_from_units(units, table))
        eng.set_parents(parents)
        st = eng.stitch(0)
    if args.trace_filter:
        group, names = traces.groups_from_table(table, corpus)
        eng.set_row_groups(group, len(names))
        trace_filter(args, eng, names, report=True)
    if args.attribute_out or args.latency_out:
        attribute_out(args, eng, st, corpus, table)
    if args.signatures_out:
        signatures_out(args, eng, corpus, table, 2 if solved is not None else 0)
    if args.profiles_out:
        profiles_out(args, eng, corpus, table, 2 if solved is not None else 0)
    if args.traces_out:
        traces_out(args, eng, corpus, table, 2 if solved is not None else 0)
    eng.close()
    if not args.stitch_out:
        return
    traces.write_npz(args.stitch_out, st, corpus, table)
    c = st.counts.tolist()
    print("Stitched traces: %d whole, %d fragments, %d with unassigned calls; exact vs ground truth: %d of %d" % (c[0], c[1], c[2], c[3], total))
    calling = {corpus.string(x) for x in np.unique(table["service"][table["kind"] == 2])}
    left = sorted(calling - {u.service for u in units})
    if left:
        print("Not in the stitch (their calls are holes, the spans below them fragments): %s" % ", ".join(left))
    elif c[3] < right:
        raise RuntimeError("stitched traces: %d exact, the accuracy reduction counts %d traces right" % (c[3], right))
    elif c[3] > right:   # bit 2 compares row sets: two requests of one service in one trace that swap their calls keep the set
        print("(%d traces hold the true spans under another assignment of calls to requests: right as a set, wrong per request)" % (c[3] - right))


def signatures_out(args, eng, corpus, table, pass_, has_truth=True):
    """--signatures_out: the true forest's signatures kept as the reference set, the predicted forest's compared with them; groups
    by service.  Without ground truth the predicted side alone."""
    from . import traces

    group, names = traces.groups_from_table(table, corpus)
    eng.set_row_groups(group, len(names))
    true = None
    if has_truth:
        eng.stitch(truth=True)
        true = eng.signatures(args.signature_mode, need_flags=traces.WHOLE | trace_filter(args, eng, names), keep_reference=True)
    eng.stitch(pass_)
    pred = eng.signatures(args.signature_mode, need_flags=traces.WHOLE | trace_filter(args, eng, names), compare=has_truth)
    traces.write_signatures_npz(args.signatures_out, names, pred, true)
    print("Call graphs (%s): %d among %d whole traces%s" % (args.signature_mode, pred.n_classes, pred.n_eligible,
                                                           "; true traces: %d among %d" % (true.n_classes, true.n_eligible) if true is not None else ""))
    if args.class_history and not args.profiles_out:
        class_history_out(args, eng, names, 1)
    if true is not None:
        print("Shape accuracy: %d of %d whole traces have the call graph of the true trace" % (pred.summary[5], pred.summary[4]))
    for row in pred.table(names)[:3 if not args.verbose else None]:
        print("  %6d traces, mean %.1f us (min %d, max %d): %s" % (
            row["trees"], row["mean_latency"], row["min_latency"], row["max_latency"],
            " | ".join("L%d %s%s x%d" % (lv, "%s>" % cg if cg is not None else "", g, k) for lv, cg, g, k in row["signature"]) or "(no service)"))


def class_history_out(args, eng, names, what):
    """--class_history: the store read into the device catalogue, the classes of the predicted forest (resident on the device, with
    what = 3 their profile too) matched against it and pushed, the catalogue written back."""
    from . import traces

    names = [str(x) for x in names]
    if os.path.exists(args.class_history):
        store, group_names = traces.read_class_history_npz(args.class_history)
        if group_names != names:
            raise SystemExit("--class_history %s: the store holds the services %s, this run %s" % (args.class_history, ", ".join(group_names), ", ".join(names)))
        if traces.SIGNATURE_MODES[store.mode] != args.signature_mode:
            raise SystemExit("--class_history %s: the store holds %s signatures, this run %s" % (args.class_history, traces.SIGNATURE_MODES[store.mode], args.signature_mode))
        eng.class_history_reset()
        eng.class_history_merge(store)
    new = int((eng.class_history_match() < 0).sum())
    _, summary = eng.class_history_push(what, args.class_history_epoch)
    c = eng.class_history()
    traces.write_class_history_npz(args.class_history, c, names)
    print("Class history: %d call graphs in this run, %d of them new; %d held over %d traces" % (summary[5], new, c.n_classes, int(c.trees.sum())))


def profiles_out(args, eng, corpus, table, pass_, has_truth=True):
    """--profiles_out: on the true and on the predicted forest stitch -> signatures -> the delay-culprit query -> class profiles;
    groups by service.  Without ground truth the predicted side alone."""
    from . import traces

    group, names = traces.groups_from_table(table, corpus)
    eng.set_row_groups(group, len(names))
    sides = []
    for truth in ([True] if has_truth else []) + [False]:
        if truth:
            eng.stitch(truth=True)
        else:
            eng.stitch(pass_)
        need = traces.WHOLE | trace_filter(args, eng, names)
        eng.signatures(args.signature_mode, need_flags=need)
        eng.attribute(percentile=args.query_percentile, start_min=args.query_after, need_flags=need)
        sides.append(eng.class_profiles())
    pred, true = sides[-1], sides[0] if has_truth else None
    traces.write_profiles_npz(args.profiles_out, names, pred, true)
    if args.class_history:
        class_history_out(args, eng, names, 3)
    print("Class profiles (%s): %d traces of %d call graphs counted, %d rows in %d entries%s" % (
        args.signature_mode, pred.summary[0], pred.summary[1], pred.summary[2], pred.summary[3],
        "; true traces: %d of %d" % (true.summary[0], true.summary[1]) if true is not None else ""))
    for row in pred.table([str(x) for x in names])[:3 if not args.verbose else None]:
        if row["top"] is None:
            print("  class %d: %d traces, mean %.1f us; no service on the path" % (row["class"], row["counted"], row["mean_latency"]))
            continue
        lv, cg, g = row["top"]
        print("  class %d: %d traces, mean %.1f us; on the path most: L%d %s%s, %.1f %% of the path time, in %.1f %% of the traces" % (
            row["class"], row["counted"], row["mean_latency"], lv, "%s>" % cg if cg is not None else "", g, 100.0 * row["top_share"], 100.0 * row["top_trees"]))


def culprit_line(a, names, head="Delay culprit"):
    g = a.culprit
    if g < 0:
        return "%s: none (%d of %d traces selected)" % (head, a.n_selected, a.n_eligible)
    total = int(a.group_path_time.sum())
    return "%s: %s, mean service latency %.1f us over %d of %d traces (critical-path share %.1f %%)" % (
        head, names[g], a.mean_latency(g), a.n_selected, a.n_eligible, 100.0 * float(a.group_path_time[g]) / total if total else 0.0)


def cohort_labels(args, corpus, table, names):
    """--cohort_service: the rows of that service labelled by the index of their operation among the service's operations (in
    ascending order of the string id), every other row -1.  The span table carries no instance column; without an operation column
    either the flag is refused."""
    if args.cohort_service not in names:
        raise SystemExit("--cohort_service %s: no such service in the span table (services: %s)" % (args.cohort_service, ", ".join(str(x) for x in names)))
    if "op_name" not in table:
        raise SystemExit("--cohort_service: the span table carries neither an operation nor an instance column to tell cohorts apart")
    service = np.asarray(table["service"])
    of = np.array([corpus.string(x) == args.cohort_service for x in np.unique(service)])[np.unique(service, return_inverse=True)[1]]
    ops, inverse = np.unique(np.asarray(table["op_name"])[of], return_inverse=True)
    label = np.full(len(service), -1, dtype=np.int32)
    label[of] = inverse
    return label, [corpus.string(x) for x in ops]


def quantile_line(d, g, head):
    """The quantiles of the span latency of group g, per cohort."""
    parts = []
    for c in range(d.n_cohorts):
        s = d.index(c, 0, g)
        if d.seg_count[s] > 0:
            parts.append("%s%s over %d spans" % ("cohort %d: " % c if d.n_cohorts > 1 else "",
                                                 ", ".join("p%g %d us" % (100 * p, d.quantile[s][j]) for j, p in enumerate(d.probs.tolist())), d.seg_count[s]))
    return "%s: %s" % (head, "; ".join(parts) if parts else "no spans")


def comparison_line(c, i, g, name):
    """Pair i of a comparison for the span latency of group g."""
    r = c.row(i, 0, g)
    a, b = c.pairs[i].tolist()
    if c.n_a[r] == 0 or c.n_b[r] == 0:
        return "Cohort %d against %d, %s span latency: no spans in one of them (%d, %d)" % (a, b, name, c.n_a[r], c.n_b[r])
    tested = c.perm_ge_ks[r] >= 0
    shifts = ", ".join("p%g %+d us%s" % (100 * p, c.quantile_shift[r][j], " (p = %.4f)" % c.p_value(j)[r] if tested else "") for j, p in enumerate(c.probs.tolist()))
    return "Cohort %d against %d, %s span latency over %d and %d spans: %s; KS %.4f at %d us%s; superiority %.4f%s" % (
        a, b, name, c.n_a[r], c.n_b[r], shifts, c.ks()[r], c.ks_at[r], " (p = %.4f)" % c.p_value("ks")[r] if tested else "",
        c.superiority()[r], " (p = %.4f)" % c.p_value("u")[r] if tested else "")


def history_out(args, eng, d, names, culprit):
    """--history / --history_compare_out: the store read into the device history, the run's distributions `d` (resident on the
    device) pushed into it, the store written back, and cohorts of it compared."""
    from . import traces

    cohorts = []
    if os.path.exists(args.history):
        source, group_names, cohorts = traces.read_history_npz(args.history)
        if group_names != [str(x) for x in names]:
            raise SystemExit("--history %s: the store holds the services %s, this run %s" % (args.history, ", ".join(group_names), ", ".join(str(x) for x in names)))
        eng.history_reset()
        eng.history_merge(source)
    added = eng.history_push([args.history_cohort + c for c in range(d.n_cohorts)])
    h = eng.history_distributions((), None)
    cohorts = cohorts + [str(c) for c in range(len(cohorts), h.n_cohorts)]
    traces.write_history_npz(args.history, h, names, cohorts)
    print("History: %d values added to cohort%s %s, %d held in %d cohorts" % (
        added[0], "s" if d.n_cohorts > 1 else "", ", ".join(str(args.history_cohort + c) for c in range(d.n_cohorts)), h.n_items, h.n_cohorts))
    if args.history_compare_out:
        pairs = pairs_of(args)
        if max(max(p) for p in pairs) >= h.n_cohorts:
            raise SystemExit("--compare_pairs %s: the store %s holds %d cohorts" % (args.compare_pairs, args.history, h.n_cohorts))
        c = eng.history_compare(pairs, quantiles_of(args), args.permutations, args.compare_seed)
        traces.write_comparison_npz(args.history_compare_out, c, names)
        print("History comparison: %d pairs, %d segments with spans in both, %d permutations of %d" % (len(pairs), c.summary[0], c.summary[3], c.summary[1]))
        for i in range(len(pairs) if culprit >= 0 else 0):
            print("History: " + comparison_line(c, i, culprit, names[culprit]))


def attribute_out(args, eng, st, corpus, table):
    """--attribute_out / --latency_out: the delay-culprit query on the forest just stitched, groups by service, and the
    distributions behind its answer."""
    from . import traces

    group, names = traces.groups_from_table(table, corpus)
    eng.set_row_groups(group, len(names))
    if args.latency_out and args.cohort_service:
        label, cohort_names = cohort_labels(args, corpus, table, names)
        eng.set_row_cohorts(label, len(cohort_names))
    query = dict(percentile=args.query_percentile, start_min=args.query_after)
    match = traces.MATCH if args.trace_filter else 0              # (stitch_out has filtered this forest)
    a = eng.attribute(need_flags=traces.WHOLE | (traces.CONFIDENT if args.query_confident else 0) | match, **query)
    if args.attribute_out:
        traces.write_attribution_npz(args.attribute_out, a, names, st)
        print(culprit_line(a, names))
    if args.latency_out:
        d = eng.distributions(quantiles_of(args))
        traces.write_distributions_npz(args.latency_out, d, names)
        print("Latency distributions: %d values in %d segments over %d traces (%d without a cohort)" % (d.n_items, d.summary[1], d.summary[2], d.summary[3]))
        if args.verbose and a.culprit >= 0:
            print(quantile_line(d, a.culprit, "Culprit span latency"))
    if args.compare_out:
        pairs = pairs_of(args)
        if max(max(p) for p in pairs) >= len(cohort_names):
            raise SystemExit("--compare_pairs %s: %s has %d cohorts (%s)" % (args.compare_pairs, args.cohort_service, len(cohort_names), ", ".join(str(x) for x in cohort_names)))
        c = eng.compare_cohorts(pairs, quantiles_of(args), args.permutations, args.compare_seed)
        traces.write_comparison_npz(args.compare_out, c, names)
        print("Cohort comparison: %d pairs, %d segments with spans in both, %d permutations of %d" % (len(pairs), c.summary[0], c.summary[3], c.summary[1]))
        for i in range(len(pairs) if a.culprit >= 0 else 0):
            print(comparison_line(c, i, a.culprit, names[a.culprit]))
    if args.history:
        history_out(args, eng, d, names, a.culprit)
    if args.verbose:
        eng.stitch(truth=True)
        b = eng.attribute(need_flags=traces.WHOLE | trace_filter(args, eng, names), **query)
        if args.attribute_out:
            print(culprit_line(b, names, "Delay culprit (true traces)"))
        if args.latency_out and b.culprit >= 0:
            print(quantile_line(eng.distributions(quantiles_of(args)), b.culprit, "Culprit span latency (true traces)"))


def run(args):
    from . import baselines
    from .engine import Engine, EngineError
    from .ingest import REFERENCE_FIX, open_directory

    if args.fix not in REFERENCE_FIX:
        raise SystemExit("--fix %d is not one of the reference's values 0..5" % args.fix)
    first_span, surgery = REFERENCE_FIX[args.fix]
    directory = args.absolute_path.rstrip("\\") if args.absolute_path else os.path.join(args.project_root, args.relative_path)
    t0 = time.time()
    # the span table of the directory is kept next to the reference's own time_order_filenames.pickle, under the same rule:
    # trusted until --clear_cache 1 (executor.py:320-339; ingest.open_directory has the guard it adds)
    corpus, counts = open_directory(directory, lib_path=args.engine_library, first_span=first_span, max_traces=args.max_traces, fix=surgery,
                                    cache=bool(args.span_cache), clear_cache=bool(args.clear_cache))
    units, skipped, n_traces = corpus.units()
    print("Loaded %d traces, %d spans in %.2f s%s (%d files rejected, %d traces filtered); %d services to solve, left out: %s"
          % (counts["traces"], counts["spans"], time.time() - t0, " from the directory's span table cache" if corpus.from_cache else "",
             counts["files_rejected"], counts["traces_filtered"], len(units), skipped))
    if not units:
        raise SystemExit("no service of this corpus can be solved (see the counts above)")
    # `several_callers` is a skip the reference performs itself (executor.py:1126-1128).  A service in which some request
    # lacks a call to an endpoint (`skip_mode`) makes the reference raise KeyError in FindOrder (executor.py:242: GetGroundTruth,
    # helpers/utils.py:22-32, leaves that request out of true_assignments[ep]) -- the only skip-mode inputs it solves are
    # the ones --cache_rate makes after FindOrder; `too_small` / `cyclic_order` raise further down (traceweaver_v3.py:1119,
    # nx.topological_sort).  Leaving such services out silently would make the figures look better than they are: stop
    lost = {k: v for k, v in skipped.items() if k != "several_callers" and v > 0}
    if lost and not args.allow_partial:
        raise SystemExit("%d service(s) of this corpus cannot be solved by the native chain: %s.  Re-run with --allow_partial 1 to "
                         "solve the others (the result files then record what was left out)." % (sum(lost.values()), lost))
    table = corpus.span_table()
    names = corpus.trace_names()
    trace_id = lambda k: corpus.string(names[k])
    cg_booleans = None
    if args.infer_order:                                           # executor.py:152-212 in place of FindOrder (:1143)
        units, cg_booleans = infer_order(units, args)
    resident = None
    if args.compress_factor > 1:                                   # executor.py:1086-1097,1146-1148
        resident = units                                           # the device scales its own copy of the table (tw_scale_load)
        units, load_factors, trace_ranks = scale_load(units, args, trace_id, corpus)
    skip_units = set()
    if args.cache_rate > 0:                                        # executor.py:1150-1152: only the service named "frontend"
        from . import skipmode
        from .ingest import IngestedUnit

        for k, u in enumerate(units):
            if u.service != "frontend":
                continue
            if u.arrays.time_scale is not None:
                raise SystemExit("--cache_rate with --compress_factor > 1 is not supported (skip mode takes integer microseconds)")
            print("cache %: ", float(args.cache_rate) * 100)
            arr, truth, kept = skipmode.cache_hits(u.arrays, u.true_parent, args.cache_rate, in_trace=u.in_trace)
            units[k] = IngestedUnit(arr, truth, u.in_trace, u.service, u.in_ep, u.out_eps, u.in_rows,
                                    [r[kept] if e == 0 else r for e, r in enumerate(u.out_rows)], u.process_id)
            skip_units.add(k)
    key = lambda row: (trace_id(table["trace"][row]), corpus.string(table["span_id"][row]))
    seen = np.zeros(n_traces, dtype=bool)
    for u in units:
        seen[u.in_trace] = True
    total = int(seen.sum())
    roots = [x for x in np.flatnonzero(table["parent"] < 0) if seen[table["trace"][x]]]

    accuracy_overall, accuracy_per_process, confidence, traces_overall, bins = {}, {}, {}, {}, {}

    def record(method, parents, bad_flags, options=None):
        """accuracy_*, e2e_*, bin_acc_* entries of one method from its parent arrays (or, for WAP5, its option lists)
        and per-trace wrong-flags."""
        true_traces, pred_traces = {}, {}
        for k, (u, par) in enumerate(zip(units, parents)):
            for i in range(u.arrays.n_in):                       # helpers/utils.py:216-252
                tid = trace_id(u.in_trace[i])
                tt, pt = true_traces.setdefault(tid, []), pred_traces.setdefault(tid, [])
                for e in range(u.arrays.E):
                    tt.append(int(u.out_rows[e][u.true_parent[e, i]]) if u.true_parent[e, i] >= 0 else None)
                    if options is not None:
                        pt.extend([int(u.out_rows[e][x]) for x in options[k][e][i]] or [None])
                    else:
                        pt.append(int(u.out_rows[e][par[e, i]]) if par[e, i] >= 0 else None)
        order = lambda rows: [key(x) if x is not None else None for x in sorted(rows, key=lambda x: float("inf") if x is None else table["start"][x])]
        traces_overall[method] = [{t: order(v) for t, v in true_traces.items()}, {t: order(v) for t, v in pred_traces.items()}]
        for name, bad in bad_flags.items():
            accuracy_overall[name] = int((~bad.astype(bool) & seen).sum()) / total * 100
            # BinAccuracyByResponseTimes (helpers/utils.py:187-214): traces ordered by the duration of their root span
            rows = sorted((int(table["duration"][x]), trace_id(table["trace"][x]), int(bad[table["trace"][x]] == 0)) for x in roots)
            acc, prev_c, prev_n, csum = [], 0, 0, np.cumsum([c for _, _, c in rows])
            for b in range(10):
                j = int(len(rows) * (b + 1) / 10 - 1)
                c, n = int(csum[j]) - prev_c, (j + 1) - prev_n
                prev_c, prev_n = prev_c + c, prev_n + n
                acc.append(((b + 1) * 100 / 10, c / n, rows[j][0] / 1000.0))
            bins[name] = acc

    for index in requested(args):
        if index == 10:
            eng = Engine(args.device, lib_path=args.engine_library)
            t1 = time.time()
            plain = [k for k in range(len(units)) if k not in skip_units]
            per, res = [None] * len(units), [None] * len(units)
            flags = np.zeros((2, n_traces), dtype=np.uint8)
            if plain and args.fit in ("sklearn", "device"):   # the reference's RNG stream replayed service by service
                from . import skipmode
                from .predictor import TraceWeaverGPU

                eng.close()
                pred = TraceWeaverGPU({}, {}, device=args.device, fit=args.fit, lib_path=args.engine_library)
                np.random.seed(args.seed)
                for k, u in enumerate(units):
                    if u.service == "frontend":   # executor.py:1150-1152: create_cache_hits reseeds (and draws) at every cache rate
                        skipmode.cache_hit_draws(u.arrays.n_in, args.cache_rate)
                    if k in skip_units:
                        continue                  # one pass, no refit: no draws (traceweaver_v3.py:1155-1156,1221)
                    _, r2 = pred.solve_arrays(u.arrays, u.true_parent, u.service)
                    pred._engine.set_truth([u.true_parent], [u.in_trace], n_traces)
                    p_, _, f_ = pred._engine.evaluate(trace_flags=True)
                    flags = np.maximum(flags, f_)
                    per[k], res[k] = p_[0], r2
                eng = pred._engine
            elif plain and resident is not None:
                # load levels on the resident table: the spans go up once, as ingested; the host transform above only
                # serves the result files and the baselines (same permutations: tests/test_load_scaling.py)
                eng.load([resident[k].arrays for k in plain])
                eng.set_truth([resident[k].true_parent for k in plain], [resident[k].in_trace for k in plain], n_traces)
                t_scale = time.time()
                perms = eng.scale_load([load_factors[k] for k in plain], trace_rank=[trace_ranks[k] for k in plain])
                for k, (ip, _, ts) in zip(plain, perms):
                    assert ts == units[k].arrays.time_scale and np.array_equal(resident[k].in_trace[ip], units[k].in_trace)
                print("Load scaling on the device: %.1f ms" % ((time.time() - t_scale) * 1e3))
            elif plain:
                eng.load([units[k].arrays for k in plain])
                eng.set_truth([units[k].true_parent for k in plain], [units[k].in_trace for k in plain], n_traces)
            if plain and args.fit == "device-batch":
                try:
                    eng.run_pass1()
                except EngineError as ex:
                    if ex.code == -7:   # TW_ERR_NAN_PARAMS, SURVEY.md hazard H3 (e.g. media_load75: 1500 files, 1001 traces kept)
                        raise SystemExit("%s\nThe reference fails on this input too (scipy.stats.tstd of one batch mean is NaN, "
                                         "traceweaver_v3.py:611). Keep a multiple-of-100-plus-anything-but-1 number of traces, "
                                         "e.g. --max_traces 1000." % ex)
                    raise
                eng.fit_mixtures(seed=args.seed)
                eng.run_pass2()
                p_, _, f_ = eng.evaluate(trace_flags=True)
                r_ = eng.results(2, fields=("parent", "unit_stats"))
                flags = np.maximum(flags, f_)
                for k, a, b in zip(plain, p_, r_):
                    per[k], res[k] = a, b
            if skip_units:   # services short of outgoing spans: the reference's one-pass skip mode (traceweaver_v3.py:1155-1156)
                from . import skipmode

                sk = sorted(skip_units)
                plans, windows = [], []
                for k, u in enumerate(units):   # one predictor object solves the services in turn and never clears its time windows:
                    if k in skip_units:         # those of every earlier service, skip budget or not, are still in it (hazard H8)
                        plans.append(skipmode.plan(eng, u.arrays, prior_windows=windows))
                        windows = list(plans[-1].windows)
                    elif u.arrays.time_scale is None:
                        windows = windows + skipmode.time_windows(u.arrays)
                eng.load([units[k].arrays for k in sk], skip=plans)
                eng.set_truth([units[k].true_parent for k in sk], [units[k].in_trace for k in sk], n_traces)
                eng.run_pass1()
                p_, _, f_ = eng.evaluate(trace_flags=True)
                r_ = eng.results(1, fields=("parent", "unit_stats"))
                flags = np.maximum(flags, f_)
                for k, a, b in zip(sk, p_, r_):
                    per[k], res[k] = a, b
            unproven = sum(r["budget_windows"] for r in res)
            if unproven:
                print("WARNING: %d window(s) hit the node budget of the exact selection search: their selection is the best one found, "
                      "not a proven optimum (DESIGN.md section 6)" % unproven)
            print("--- %s seconds --- (%d services, both passes, refit, accuracy)" % (time.time() - t1, len(units)))
            solved = eng if args.confidence_out else None          # (device-batch, no skip mode: pass 2 of every service is resident)
            if solved is None:
                eng.close()
            for u, ev, r in zip(units, per, res):
                print("Accuracy for service %s: %.3f%%\n" % (u.service, ev["accuracy"] * 100))
                print("Top K accuracy for service %s: %.3f%%\n" % (u.service, ev["topk_accuracy"] * 100))
                accuracy_per_process[(METHOD, u.process_id)] = ev["accuracy"]
                confidence[u.service] = [ev["accuracy"], r["not_best_count"], u.arrays.n_in]
            record(METHOD, [r["parent"] for r in res], {METHOD: flags[0], METHOD + "TopK": flags[1]})
            if args.stitch_out or args.attribute_out or args.confidence_out or args.latency_out or args.signatures_out or args.profiles_out or args.trace_filter or args.traces_out:
                stitch_out(args, corpus, units, table, [r["parent"] for r in res], n_traces, total, int((~flags[0].astype(bool) & seen).sum()),
                           solved=solved)
        else:
            method = BASELINES[index]
            parents, bad, all_options = [], np.zeros(n_traces, dtype=np.uint8), []
            on_device = method in ("FCFS", "vPath", "WAP5") and not skip_units
            if on_device:   # on the resident table (csrc/tw_baselines.h); skip-mode services (unsorted lists) and ArrivalOrder: host
                eng_b = Engine(args.device, lib_path=args.engine_library)
                eng_b.load([u.arrays for u in units])
                eng_b.set_truth([u.true_parent for u in units])
                if method == "WAP5":   # one predictor object for the run: delay samples accumulate per callee name over the services
                    parents, _, all_options = eng_b.wap5([u.out_eps for u in units])
                else:
                    parents = eng_b.baseline(method)
                eng_b.close()
            else:
                wap5 = baselines.WAP5()                                # one instance for the run: its state leaks across services
                fn = {"FCFS": lambda u: baselines.fcfs(u.arrays), "ArrivalOrder": lambda u: baselines.arrival_order(u.arrays),
                      "vPath": lambda u: baselines.vpath(u.arrays, u.true_parent), "WAP5": None}[method]
                for u in units:
                    if method == "WAP5":
                        all_options.append(wap5.assign(u.arrays, u.out_eps))
                        parents.append(baselines.WAP5.parent(u.arrays, all_options[-1]))
                    else:
                        parents.append(fn(u))
            for u, par in zip(units, parents):
                ok = np.all(par == u.true_parent, axis=0)
                print("Accuracy for service %s: %.3f%%\n" % (u.service, ok.mean() * 100))
                accuracy_per_process[(method, u.process_id)] = float(ok.mean())
                bad[u.in_trace[~ok]] = 1
            record(method, parents, {method: bad}, options=all_options if method == "WAP5" else None)
    for k, v in accuracy_overall.items():
        print("End-to-end accuracy for method %s: %.3f%%" % (k, v))
    if lost:
        confidence["left_out"] = dict(lost)
    if cg_booleans is not None:
        print("Inferred call graphs identical to FindOrder's: %d of %d" % (sum(cg_booleans), len(cg_booleans)))

    os.makedirs(os.path.dirname(args.results_directory) or ".", exist_ok=True)   # the name is used as a prefix, like the reference does
    suffix = "_%s_%s_%s_%s_%s.pickle" % (args.test_name, args.load_level, int(args.compress_factor), int(args.repeat_factor), args.cache_rate)
    for name, obj in (("bin_acc", bins), ("accuracy", accuracy_overall), ("e2e", traces_overall), ("confidence_scores", confidence),
                      ("process_acc", accuracy_per_process)):
        with open(args.results_directory + name + suffix, "wb") as f:       # executor.py:1235-1244: plain concatenation
            pickle.dump(obj, f, protocol=pickle.HIGHEST_PROTOCOL)
    corpus.close()
    return accuracy_overall, accuracy_per_process, confidence


def main(argv=None):
    # this is an application: it asks for the hardware queues the engine's class streams want before HIP initialises
    # (csrc/tw_engine.hip, tw_create) -- unless the user chose a value
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    args = parse_args(argv)
    problems = unsupported(args)
    if problems:
        sys.exit("traceweaver_amd.executor runs predictor 10 (%s, with or without load scaling) and the baselines 3, 4, 5, 7; not supported here: %s.\n"
                 "Use the reference's executor with TraceWeaverGPU registered in its predictor table (INTEGRATION.md section 2)."
                 % (METHOD, "; ".join(problems)))
    run(args)


if __name__ == "__main__":
    main()
