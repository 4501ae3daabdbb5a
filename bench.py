#!/usr/bin/env python3
"""Throughput of the span->parent reconstruction hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

One *step* = one full two-pass reconstruction (TraceWeaverV3.FindAssignments, traceweaver_v3.py:1087-1229)
of every service unit resident on the GPU: pass 1 (windows, Gaussian parameters, candidate enumeration,
exact per-window selection, consumption repair) -> per-edge mixture refit -> pass 2 -> accuracy against ground
truth (device reduction; the parent arrays stay in HBM).  Spans are already in HBM when the timed region starts
(tw_load_batch is outside it).  `value` = spans (incoming + outgoing handed to the engine)
per second over all ranks.

Workloads (--workload):
  media    BASELINE.json config 2 shape (default, the configuration the metric is quoted on for one GPU): the six
           accelerated services of media_microservices (E in {1,1,1,1,2,4}) scaled up with the seed-fixed synthetic
           generator in traceweaver_amd/synth.py (the shipped corpus has 1000 requests per service, which a GPU
           finishes in microseconds): by default 16 replicas of the graph x 100 000 requests per service = 25.6 M spans
           resident per GPU.  Weak scaling: every rank holds its own replicas.
  nodejs   config 3 shape: nodejs_microservices_with_arbitrary_file_io, 4 services, millisecond-granular, heavily
           interleaved.  Weak scaling.
  alibaba  config 4: ONE Alibaba-shape slice (--total-spans, default 1 M engine spans, 15 call graphs, 39 services)
           sharded per service over the ranks (sharding.shard_units, LPT on measured work), every step ends with the
           all-gather of the parent arrays (RCCL over xGMI), the path's one exchange step.  Strong
           scaling: total work is fixed.  With --verify rank 0 also solves the whole slice alone and the gathered
           parents must equal that result.

  alibaba-full  config 5: the 15 Alibaba-shape call graphs (--total-spans engine spans in all) at the six load levels of
           exps/exp5 (compress factors 1 ... 15000; a service's load factor is max(1, ceil(factor / #replicas)),
           executor.py:1089-1097, replica table generated with the corpus): every (level, service) pair is a unit; the units
           are sharded over the ranks and uploaded ONCE, all levels resident together; every step scales each copy to its
           level on the device (one tw_scale_load call), solves the whole matrix in one step and gathers the parents (RCCL on
           the engine's buffers).  Strong scaling; value = spans x levels per second.

  media-split  within-service sharding: ONE media-shape graph whose six services hold --n-in x --replicas requests each;
           every service is cut at idle moments into one part per rank (sharding.split_points / split_unit), the parts'
           gap samples are all-gathered between the passes and every rank refits on the union
           (sharding.refit_split_services), parents are gathered at the end.  Strong scaling; bit-identical to the
           unsplit run (--verify 1 checks it on rank 0).

`python bench.py --gpus N --full` with N > 1 and no --workload prints the media line (weak scaling) and, under `scale_regimes`, the two
sharded modes north_star names -- `alibaba` and `alibaba-full`, each with --verify 1 (`sharded_equals_single_gpu`).

N > 1: `python bench.py --gpus N` starts N ranks itself (re-exec under torch.distributed.run on 127.0.0.1); when the
driver has already started the ranks (RANK / WORLD_SIZE in the environment) --gpus must equal WORLD_SIZE.  One process
per GPU, rank r -> device LOCAL_RANK; the media / nodejs workloads have no data-path collective (units are
independent), the only collectives are the timing barrier / max-reduce.

A plain run only sets up, warms up, times the --steps steps, writes --dump-outputs if asked and prints the result line.
Everything else moves behind --full: the harder single-GPU regimes, the CPU baseline, the ingest / end-to-end / load-level
/ shipped-corpora legs, the measured HBM peak, the host cross-check of the device accuracy reduction, the sharded modes of
`--gpus N > 1` without --workload and the detail file (unless --detail-file names one).

--dump-outputs DIR writes what the last timed step computed (pass 2's parent arrays, a seeded sample of them when the
batch is larger, and the per-unit accuracies; see dump_outputs) as .npy files, so that two builds can be compared output
for output: with the same arguments the inputs are the same seed-fixed synthetic batch.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
# hardware queues for the engine's class streams (traceweaver_amd/csrc/tw_engine.hip, tw_create): set before torch or the engine
# initialise HIP; the ranks of `--gpus N` inherit it
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")

HBM_PEAK_GBPS = 8000.0            # MI355X_MICROARCH.md: 8.0 TB/s spec
ALG_BYTES_PER_SPAN_PER_PASS = 20  # 16 B read (start, end) + 4 B parent index written


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default=None, choices=["media", "nodejs", "alibaba", "alibaba-full", "media-split"],
                    help="default: media -- and with --full and --gpus N > 1 also the two sharded modes (alibaba, alibaba-full, each with --verify 1) under `scale_regimes`")
    ap.add_argument("--scale-regimes", type=int, default=1, help="--full, --gpus N > 1 without --workload: also run the sharded modes (0 = only the media line)")
    ap.add_argument("--levels", default="1,200,1000,4000,10000,15000",
                    help="alibaba-full: the --compress_factor values every call graph is solved at (exps/exp5/run_experiment.sh:60-156)")
    ap.add_argument("--n-in", type=int, default=100000, help="requests per service unit (media / nodejs)")
    ap.add_argument("--replicas", type=int, default=None,
                    help="copies of the service graph per GPU (media / nodejs).  Default: 16 for the media workload -- a resident batch "
                         "of 25.6 M spans (0.4 GB of timestamps in 288 GB of HBM); the kernels' tails (one 25-span window, one 4e4-tuple "
                         "span) do not grow with the batch: 4.9e8 spans/s at 4 replicas, 6.1e8 at 8, 6.8e8 at 16, 7.1e8 at 32 "
                         "(profiles/r02d_batch_sweep.json) -- 4 for the others")
    ap.add_argument("--concurrency", type=float, default=None, help="mean requests in flight per service (default: 1.6 media, 4 nodejs, 1.3 alibaba)")
    ap.add_argument("--total-spans", type=int, default=1000000, help="engine spans of the Alibaba-shape slice (whole job)")
    ap.add_argument("--verify", type=int, default=0, help="alibaba: rank 0 also solves the whole slice alone and compares the gathered parents")
    ap.add_argument("--fit", default="device", choices=["device", "sklearn"], help="mixture refit between the passes")
    ap.add_argument("--cpu-sample", type=int, default=40000, help="--full: requests per service in the CPU-baseline sample (0 = skip)")
    ap.add_argument("--cpu-procs", type=int, default=32, help="CPU baseline: also the sample in min(this, usable cores) processes at once (1 = skip)")
    ap.add_argument("--cpu-worker", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--regimes", type=int, default=1,
                    help="--full, default workload at N = 1 only: after the timed step loop, 3 steps each of the harder single-GPU regimes "
                         "(config 3 shape, the config 4 slice on one GPU, media shape at concurrency 4 and 8) on the same engine, "
                         "reported under `regimes` with their own roofline blocks")
    ap.add_argument("--end-to-end", type=int, default=1, help="--full: also time JSON -> ingest -> H2D -> two passes -> parents on the host (rank 0, N = 1)")
    ap.add_argument("--host-traces", default="20000,15000", help="traces of the hotel- and the Alibaba-shape JSON corpus of the ingest / end-to-end legs")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend (nccl = RCCL; gloo lets several ranks share one GPU for testing)")
    ap.add_argument("--sync", default="torch", choices=["torch", "engine"],
                    help="torch: torch.cuda.synchronize() around the timed region (the bench contract).  engine (N = 1 only): no torch "
                         "import -- every C-ABI call returns with its stream synchronised; what profiles/collect.sh uses, so that its "
                         "rocprofv3 passes do not spend a minute each importing torch on a fresh box")
    ap.add_argument("--detail-file", default=None, help="where the full record goes (written by default only with --full, see write_detail); the last stdout line is the compact one")
    ap.add_argument("--lib", default=None, help="TESTING ONLY: path of an alternative build of libtwgpu (the host-emulation "
                                                "library of tests/hostemu); no GPU is touched then")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: regimes, CPU baseline, host legs, measured HBM "
                         "peak, host cross-check of the accuracy, the sharded modes of --gpus N > 1, the detail file")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last step computed to DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()
    args.default_line = args.workload is None   # the driver's line: media, plus the sharded modes when N > 1 (main)
    if args.default_line:
        args.workload = "media"
    return args


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(args):
    """`python bench.py --gpus N` outside a launcher: start N ranks of this script on this node."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def fit_mixtures(eng, mode, unit_ids=None, seed=0):
    """The refit between the passes.  "device": the reference's procedure on the GPU (csrc/tw_fit.h), every unit drawing its
    k-means++ seeds from an MT19937 stream of its own (seed + global unit id), so that a unit's result does not depend on
    which units share its GPU; "sklearn": scikit-learn on the host (cross-check)."""
    from traceweaver_amd import gmm

    if mode == "device":
        ids = range(len(eng.units)) if unit_ids is None else unit_ids
        eng.fit_mixtures(unit_seeds=[seed + int(k) for k in ids])
        return
    gaps = eng.gaps()
    fitted = [gmm.fit_unit(g) for g in gaps]
    eng.set_mixtures([f[0] for f in fitted], [f[1] for f in fitted])


def one_step(eng, mode, unit_ids=None):
    eng.run_pass1()
    t1 = eng.timing()
    fit_mixtures(eng, mode, unit_ids)
    eng.run_pass2()
    t2 = eng.timing()
    res = eng.evaluate()  # accuracy vs ground truth as a device reduction (helpers/utils.py:62-97); parents stay in HBM
    return t1, t2, res


def make_units(args, seed, n_in=None, replicas=None, total_spans=None):
    from traceweaver_amd import synth

    n_in = args.n_in if n_in is None else n_in
    if replicas is None:
        replicas = args.replicas if args.replicas is not None else (16 if args.workload == "media" else 4)
    if args.workload == "media-split":
        conc = 1.6 if args.concurrency is None else args.concurrency
        u, t = synth.make_workload(seed, n_in * replicas, services=synth.MEDIA_SERVICES, replicas=1, concurrency=conc)
        name = "media_microservices shape, ONE graph (6 services, %d requests each), every service split over the ranks at idle moments, concurrency %.1f" % (
            n_in * replicas, conc)
        return u, t, name
    if args.workload == "media":
        conc = 1.6 if args.concurrency is None else args.concurrency
        u, t = synth.make_workload(seed, n_in, services=synth.MEDIA_SERVICES, replicas=replicas, concurrency=conc)
        name = "media_microservices shape (6 services, E in {1,1,1,1,2,4}), %d requests/service x %d replicas per GPU, concurrency %.1f" % (
            n_in, replicas, conc)
        return u, t, name
    if args.workload == "nodejs":
        conc = 4.0 if args.concurrency is None else args.concurrency
        u, t = synth.make_nodejs_workload(seed, n_in, concurrency=conc, replicas=replicas)
        name = "nodejs_microservices_with_arbitrary_file_io shape (4 services, E in {1,2,1,1}, ms-granular), %d requests/service x %d replicas per GPU, concurrency %.1f" % (
            n_in, replicas, conc)
        return u, t, name
    full = args.workload == "alibaba-full"
    conc = (1.0 if full else 1.3) if args.concurrency is None else args.concurrency
    u, t, _ = synth.make_alibaba_workload(10, args.total_spans if total_spans is None else total_spans, concurrency=conc)
    if full:
        name = "alibaba_microservices shape, full matrix: 15 call graphs (%d services, %d spans, ms-granular) x %d load levels (compress factors %s), sharded per service, concurrency %.1f at level 1" % (
            len(u), sum(x.n_spans for x in u), len(args.levels.split(",")), args.levels, conc)
        return u, t, name
    name = "alibaba_microservices shape, one %d-span slice (15 call graphs, %d services, ms-granular), sharded per service, concurrency %.1f" % (
        sum(x.n_spans for x in u), len(u), conc)
    return u, t, name


REGIMES = [   # (key, workload, overrides): BASELINE.json configs 3 and 4 on one GPU, and the media shape at higher load
    ("config3_nodejs", "nodejs", {"n_in": 20000, "replicas": 4}),
    ("config4_alibaba_1gpu", "alibaba", {}),
    ("media_concurrency4", "media", {"n_in": 20000, "replicas": 4, "concurrency": 4.0}),
    ("media_concurrency8", "media", {"n_in": 5000, "replicas": 4, "concurrency": 8.0}),
    # the same two BASELINE shapes with enough resident work to fill the GPU (the lines above are latency at the configs' own sizes):
    # saturated throughput of the ms-granular / deep-call-graph paths
    ("config3_nodejs_saturated", "nodejs", {"n_in": 100000, "replicas": 16}),
    ("config4_alibaba_saturated", "alibaba", {"total_spans": 16000000}),
]
# the record of the reference itself (oracle/refrun/time_reference.py, build container) that belongs to each regime's shape
REGIME_REFERENCE = {"config3_nodejs": "nodeio", "config4_alibaba_1gpu": "alibaba", "media_concurrency4": "media", "media_concurrency8": "media",
                    "config3_nodejs_saturated": "nodeio", "config4_alibaba_saturated": "alibaba"}


def reference_record(shape):
    """The reference's own throughput on a corpus of this shape: profiles/cpu_reference.json (one core; see cpu_baseline)."""
    ref = os.path.join(REPO, "profiles", "cpu_reference.json")
    if not os.path.exists(ref):
        return None
    r = json.load(open(ref)).get("shapes", {}).get(shape)
    if r is None:
        return None
    return {k: r[k] for k in ("value", "unit", "cores", "kind", "what", "spans", "find_assignments_s", "end_to_end_accuracy_pct", "measured_in") if k in r}


def run_regimes(args, eng, steps=3):
    """The harder single-GPU regimes next to the headline one, same engine, same step (two passes + refit + accuracy),
    one warm-up step then `steps` timed ones each."""
    import copy

    out = {}
    for key, workload, over in REGIMES:
        a = copy.copy(args)
        a.workload = workload
        a.concurrency = over.get("concurrency")
        units, truth, name = make_units(a, 1000, n_in=over.get("n_in"), replicas=over.get("replicas"), total_spans=over.get("total_spans"))
        spans = int(sum(u.n_spans for u in units))
        eng.load(units)
        eng.set_truth(truth)
        one_step(eng, "device")
        t0 = time.perf_counter()
        en, se, rp, ft, rounds = [], [], [], [], []
        for _ in range(steps):
            t1, t2, res = one_step(eng, "device")
            en += [t1["enumerate"], t2["enumerate"]]; se += [t1["select"], t2["select"]]; rp += [t1["repair"], t2["repair"]]
            ft.append(t2["fit"]); rounds += [t1["rounds"], t2["rounds"]]
        dt = (time.perf_counter() - t0) / steps
        stats = eng.results(2, fields=("unit_stats",))
        groups = {"k_enumerate": float(np.mean(en)), "k_select": float(np.mean(se)), "k_repair": float(np.mean(rp)), "k_fit": float(np.mean(ft))}
        dominant = max(groups, key=lambda k: groups[k] * (1 if k == "k_fit" else 2))
        achieved = ALG_BYTES_PER_SPAN_PER_PASS * spans / (groups[dominant] * 1e-3) / 1e9
        n_req = sum(u.n_in for u in units)
        out[key] = {"workload": name, "spans": spans, "value": spans / dt, "unit": "spans/s", "ms_per_step": dt * 1e3, "steps": steps,
                    "accuracy": float(sum(r["accuracy"] * u.n_in for r, u in zip(res, units)) / n_req),
                    "budget_windows": int(sum(r["budget_windows"] for r in stats)), "repaired_windows": int(sum(r["repaired_windows"] for r in stats)),
                    "windows": int(sum(r["n_windows"] for r in stats)), "dp_windows": int(sum(r["dp_windows"] for r in stats)),
                    "dfs_components": int(sum(r["dfs_components"] for r in stats)),
                    "repair_rounds_per_pass": float(np.mean(rounds)),
                    "roofline": {"bound": "hbm", "kernel": dominant, "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                 "frac": achieved / HBM_PEAK_GBPS, "kernel_ms": groups[dominant], "group_ms_per_launch": groups,
                                 "algorithmic_bytes_per_launch": float(ALG_BYTES_PER_SPAN_PER_PASS * spans), "traffic": None},
                    "cpu_baseline": {"reference": reference_record(REGIME_REFERENCE[key])}}
        if key.startswith("media_concurrency"):
            out[key]["cpu_baseline"]["note"] = ("the reference was timed on the media shape at concurrency 1.6 (at 10 x load it did not finish a "
                                                "4000-span service in 600 s, SURVEY.md 0); beyond 14 requests in flight results are pinned "
                                                "engine-vs-oracle only (DESIGN.md 8)")
    return out


def _cpu_sample(args, seed):
    """One run of the CPU oracle over the sample: (spans, seconds, services)."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import tw_oracle as T

    units, _, _ = make_units(args, seed, n_in=args.cpu_sample, replicas=1, total_spans=min(args.total_spans, 16 * args.cpu_sample))
    spans = sum(u.n_spans for u in units)
    from threadpoolctl import threadpool_limits

    t0 = time.perf_counter()
    with threadpool_limits(limits=1):   # "1 thread" includes the BLAS / OpenMP pools under the refit
        for u in units:
            svc = T.Service(u.in_start, u.in_end - u.in_start, u.out_off, u.out_start, u.out_end - u.out_start, u.dag, u.key_rank)
            T.run_service(svc)
    return spans, time.perf_counter() - t0, len(units)


def cpu_all_cores(args, seed, budget_s=90.0):
    """The same sample in one process per host core at once (every process its own copy of the sample: the services of a
    run are independent, which is how a CPU deployment of the port would use the box): aggregate spans / slowest process."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    procs = max(1, min(avail, args.cpu_procs))
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", "1", "--cpu-sample", str(args.cpu_sample), "--workload", args.workload,
           "--total-spans", str(args.total_spans)] + (["--concurrency", str(args.concurrency)] if args.concurrency is not None else [])
    t0 = time.perf_counter()
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")   # one core per process (the refit's BLAS / OpenMP pools)
    ps = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, env=env) for _ in range(procs)]
    rows = []
    deadline = time.perf_counter() + budget_s
    for p in ps:
        try:
            out, _ = p.communicate(timeout=max(1.0, deadline - time.perf_counter()))
        except subprocess.TimeoutExpired:
            p.kill()
            p.communicate()
            continue
        if p.returncode == 0 and out.strip():
            rows.append(json.loads(out.strip().split("\n")[-1]))
    if len(rows) < procs:   # a process failed or ran out of time: no figure rather than a flattering one
        return {"value": None, "cores": procs, "what": "%d of %d processes finished within %.0f s" % (len(rows), procs, budget_s)}
    slowest = max(r["seconds"] for r in rows)
    return {"value": sum(r["spans"] for r in rows) / slowest, "unit": "spans/s", "cores": len(rows), "slowest_process_s": slowest,
            "wall_s": time.perf_counter() - t0, "what": "%d processes, each the whole sample" % len(rows)}


def cpu_baseline(args, seed):
    """The CPU oracle (a C port of the reference algorithm, 1 thread) on a bounded sample of the same
    workload: same services, fewer requests per service.  Next to it the record of the reference itself (its
    Python executor, predictor index 10, HiGHS in place of Gurobi) timed in the build container on a corpus of the
    same shape: profiles/cpu_reference.json, written by oracle/refrun/time_reference.py -- /root/reference does not
    exist on the GPU box, so that figure cannot be re-measured there."""
    spans, dt, n_units = _cpu_sample(args, seed)
    out = {"value": spans / dt, "unit": "spans/s", "cores": 1, "kind": "port", "host_cores": os.cpu_count(),
           "sample": "oracle/tw_oracle.c two-pass (sklearn refit) on the same %d %s-shape services at %d requests each (%d spans, %.1f s), 1 thread"
                     % (n_units, args.workload, args.cpu_sample, spans, dt)}
    if args.cpu_procs > 1:
        out["all_cores"] = cpu_all_cores(args, seed, budget_s=max(60.0, 6.0 * dt))   # (256 processes at once did not finish in 30 x the single run on the bench box)
    ref = os.path.join(REPO, "profiles", "cpu_reference.json")
    if os.path.exists(ref):
        out["reference"] = json.load(open(ref))
    return out


def _corpus(kind, directory, n_traces):
    """Jaeger JSON files of one shape: "hotel" (hotel_reservation, Jaeger export, no span rewriting) or "alibaba" (the
    output format of the reference's alibaba-analysis parser: one record per call side, --fix 5 rewrite)."""
    from traceweaver_amd import synth

    if kind == "alibaba":
        return synth.write_alibaba_corpus(directory, 5, n_traces, concurrency=1.5), "rpc_twins"
    return synth.write_jaeger_corpus(directory, 5, n_traces, app=synth.HOTEL_APP), None


def ingest_rate(n_traces=20000, threads=0, lib=None, kind="hotel", repeats=3, corpus=None):
    """Host side of the chain, informational: Jaeger JSON files -> service units through the native
    loader (tw_corpus_*), files in the page cache.  Not part of `value` (whose inputs are resident in HBM).  The call is
    repeated on the same files (a fresh corpus each time); `value` is the best run, `runs_s` lists all of them (the first
    one pays for the page faults of the parser threads' heaps)."""
    import tempfile

    from traceweaver_amd.ingest import Corpus

    runs, counts, units = [], None, []
    with tempfile.TemporaryDirectory() as d:
        paths, fix = corpus if corpus is not None else _corpus(kind, d, n_traces)
        for _ in range(repeats):
            c = Corpus(lib_path=lib)
            t0 = time.perf_counter()
            counts = c.add_files(paths, first_span=None, max_traces=0, threads=threads, fix=fix)
            units, _, _ = c.units()
            runs.append(time.perf_counter() - t0)
            c.close()
    return {"value": counts["spans"] / min(runs), "unit": "spans/s", "threads": threads or min(os.cpu_count() or 1, 32, n_traces // 64 + 1),
            "traces": n_traces, "spans": counts["spans"], "services": len(units), "runs_s": runs,
            "what": "%s-shape Jaeger JSON (one trace per file) -> span table -> per-service SoA units, native loader" % kind}


def load_levels(device, lib=None, n_in=50000, factors=(2, 3, 5)):
    """Load levels of one corpus (exps/exp5 runs six per call graph): the reference's --compress_factor transform
    (helpers/transforms.py:10-40) on the span table resident in HBM (tw_scale_load) against host transform + upload."""
    import time

    import numpy as np

    from traceweaver_amd import synth, transforms
    from traceweaver_amd.engine import Engine

    units, truth = synth.make_workload(77, n_in, services=synth.MEDIA_SERVICES, replicas=2, concurrency=1.2)
    spans = int(sum(u.n_in * (1 + u.E) for u in units))
    eng = Engine(device, lib_path=lib)
    t0 = time.perf_counter()
    eng.load(units)
    eng.set_truth(truth)
    t_up = time.perf_counter() - t0
    eng.scale_load([factors[0]] * len(units))                                  # (first call: keeps the table as uploaded)
    t0 = time.perf_counter()
    for f in factors:
        eng.scale_load([f] * len(units))
    t_dev = (time.perf_counter() - t0) / len(factors)
    t0 = time.perf_counter()
    host = [transforms.compress_unit(u, tp, factors[-1]) for u, tp in zip(units, truth)]
    t_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = Engine(device, lib_path=lib)
    ref.load([h.arrays for h in host])
    t_reload = time.perf_counter() - t0
    eng.run_pass1(); ref.run_pass1()
    same = all(np.array_equal(a["parent"], b["parent"]) for a, b in zip(eng.results(1, fields=("parent",)), ref.results(1, fields=("parent",))))
    eng.close(); ref.close()
    return {"spans": spans, "levels": list(factors), "device_s_per_level": t_dev, "host_transform_s_per_level": t_host,
            "upload_s": t_up, "reload_s_per_level": t_reload, "same_assignments": bool(same),
            "what": "media shape, %d spans: one upload, then tw_scale_load per level (incl. permutations back to the host) vs numpy transform + upload per level" % spans}


def end_to_end(device, lib=None, n_traces=20000, threads=0, kind="hotel", repeats=3, corpus=None, cache_dir=None):
    """What a user of the command line gets, nothing resident beforehand: Jaeger JSON files (page cache) -> native ingest
    -> tw_load_batch (host -> HBM) -> pass 1 -> refit -> pass 2 -> parent arrays back on the host.  Bounded sample; not
    `value`.  The chain runs `repeats` times from the files (fresh corpus, fresh batch); the best run is quoted, all are
    listed, the phases are those of the best run."""
    import tempfile

    from traceweaver_amd import ingest
    from traceweaver_amd.engine import Engine
    from traceweaver_amd.ingest import Corpus

    runs = []
    with tempfile.TemporaryDirectory() as d:
        paths, fix = corpus if corpus is not None else _corpus(kind, d, n_traces)
        eng = Engine(device, lib_path=lib)
        if cache_dir is not None:   # the run that leaves the directory's span table cache behind is not one of the timed ones
            ingest.open_directory(cache_dir, lib_path=lib, first_span=None, max_traces=0, fix=fix, threads=threads, clear_cache=True)[0].close()
        for _ in range(repeats):
            t0 = time.perf_counter()
            if cache_dir is not None:
                c, _ = ingest.open_directory(cache_dir, lib_path=lib, first_span=None, max_traces=0, fix=fix, threads=threads)
                assert c.from_cache
            else:
                c = Corpus(lib_path=lib)
                c.add_files(paths, first_span=None, max_traces=0, threads=threads, fix=fix)
            units, _, _ = c.units()
            t1 = time.perf_counter()
            eng.load([u.arrays for u in units])
            t2 = time.perf_counter()
            eng.run_pass1()
            ta = time.perf_counter()
            g1 = eng.timing()
            eng.fit_mixtures()
            tb = time.perf_counter()
            eng.run_pass2()
            tc = time.perf_counter()
            g2 = eng.timing()
            parents = eng.results(2, fields=("parent",))
            t3 = time.perf_counter()
            # where a small solve goes: host wall time of every call, and the GPU time (HIP events) inside the two passes
            phases = {"pass1_ms": (ta - t2) * 1e3, "fit_ms": (tb - ta) * 1e3, "pass2_ms": (tc - tb) * 1e3, "parents_d2h_ms": (t3 - tc) * 1e3,
                      "pass1_gpu_ms": g1["pass"], "pass2_gpu_ms": g2["pass"], "fit_gpu_ms": g2["fit"]}
            spans = sum(u.arrays.n_spans for u in units)
            acc = float(np.mean([np.all(p["parent"] == u.true_parent, axis=0).mean() for p, u in zip(parents, units)]))
            runs.append({"total_s": t3 - t0, "ingest_s": t1 - t0, "load_s": t2 - t1, "solve_s": t3 - t2, "spans": spans, "accuracy": acc,
                         "services": len(units), "solve_phases": phases})
            c.close()
        eng.close()
    best = min(runs, key=lambda r: r["total_s"])
    return {"value": best["spans"] / best["total_s"], "unit": "spans/s", "spans": best["spans"], "traces": n_traces, "services": best["services"],
            "threads": threads or min(os.cpu_count() or 1, 32, n_traces // 64 + 1), "accuracy": best["accuracy"],
            "ingest_s": best["ingest_s"], "load_s": best["load_s"], "solve_s": best["solve_s"], "solve_phases": best["solve_phases"], "runs_s": [r["total_s"] for r in runs],
            "what": ("%s -> H2D -> pass 1 -> refit -> pass 2 -> parents on the host; %s-shape corpus, best of %d runs over the same files"
                     % ("the directory's span table cache (ingest.open_directory; executor --span_cache 1, SURVEY.md 8 f1)" if cache_dir is not None
                        else "JSON files -> native ingest", kind, repeats))}


def shipped_corpora(device, lib=None, repeats=5):
    """What a user of exps/exp1 has: every service of the 23 corpora the reference ships (1000 traces each), here the inputs the
    reference's executor handed its predictor in the frozen runs (tests/golden/ref_*.npz -- the data directory itself is not on
    the GPU box) -- all 90 services in ONE batch: pass 1 -> refit -> pass 2 -> parents on the host, best of `repeats`; beside it
    the reference's own FindAssignments wall time for the same services (recorded when the goldens were frozen: one core of the
    build container, HiGHS in place of Gurobi).  Small inputs: a solve is a chain of dependent launches, not throughput."""
    import glob

    from traceweaver_amd.engine import Engine, UnitArrays

    files = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "ref_*__*.npz")))
    if not files:
        return None
    units, truth, ref_wall = [], [], 0.0
    for f in files:
        d = np.load(f)
        order = [str(x) for x in d["partition_key_order"]]
        key_rank = np.array([order.index(str(e)) for e in d["out_eps"]], dtype=np.int32)
        units.append(UnitArrays(d["in_start"], d["in_start"] + d["in_dur"], d["out_off"], d["out_start"], d["out_start"] + d["out_dur"], d["dag"], key_rank))
        truth.append(np.asarray(d["true_parent"], dtype=np.int32))
        ref_wall += float(d["ref_wall_s"])
    spans = int(sum(u.n_spans for u in units))
    eng = Engine(device, lib_path=lib)
    runs = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        eng.load(units)
        t1 = time.perf_counter()
        eng.run_pass1()
        eng.fit_mixtures()
        eng.run_pass2()
        parents = eng.results(2, fields=("parent",))
        runs.append((time.perf_counter() - t1, t1 - t0))
    eng.close()
    solve, load = min(runs[1:])
    acc = float(np.mean([np.all(p["parent"] == tp, axis=0).mean() for p, tp in zip(parents, truth)]))
    return {"services": len(units), "corpora": len({os.path.basename(f).split("__")[0] for f in files}), "spans": spans,
            "solve_s": solve, "load_s": load, "value": spans / solve, "unit": "spans/s", "accuracy_mean_per_service": acc,
            "reference": {"find_assignments_s": ref_wall, "value": spans / ref_wall, "unit": "spans/s", "cores": 1,
                          "what": "sum of the reference's FindAssignments wall times for the same 90 services (tests/golden/*.npz ref_wall_s: "
                                  "build container, one core, HiGHS in place of Gurobi)"},
            "what": "all %d services of the shipped corpora in one batch: upload excluded, pass 1 + refit + pass 2 + parents to the host, best of %d" % (len(units), repeats)}


def profile_traffic(dominant, spans_rank):
    """HBM bytes per launch of the dominant kernel group from the newest committed rocprofv3 PMC passes
    (profiles/collect.sh) -- only if that profile was taken from exactly these kernel sources and this workload."""
    import glob

    from traceweaver_amd import build as tw_build

    tpaths = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_traffic.json")))
    if not tpaths:
        return None, None
    tj = json.load(open(tpaths[-1]))
    if tj.get("source_digest") != tw_build.source_digest():
        return None, "profile %s was taken from other kernel sources" % os.path.basename(tpaths[-1])
    g = tj["groups"].get(dominant)
    if not g or tj.get("spans_per_launch") != spans_rank:
        return None, "profile %s holds another workload" % os.path.basename(tpaths[-1])
    return g["fetch_bytes_x2"] + g["write_bytes"], os.path.basename(tpaths[-1])


DUMP_SAMPLE = 1 << 21   # parent entries --dump-outputs writes at most (2 x 16 MB as float64)


def dump_outputs(directory, parents, res):
    """--dump-outputs: what the last timed step handed its caller, as .npy files in `directory`:
    parent.npy (float64) pass 2's parent arrays of every unit ([E, n_in] each, flattened and concatenated in unit order; -1 =
    unassigned) -- all of them up to DUMP_SAMPLE entries, beyond that a fixed sample drawn with seed 0 -- and
    parent_index.npy (float64) the positions of those entries in the concatenation; accuracy.npy / topk_accuracy.npy
    (float64) the per-unit figures of the device reduction (of this rank's units)."""
    flat = np.concatenate([np.asarray(p, dtype=np.int64).ravel() for p in parents])
    if len(flat) > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(0).choice(len(flat), DUMP_SAMPLE, replace=False))
    else:
        idx = np.arange(len(flat))
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "parent.npy"), flat[idx].astype(np.float64))
    np.save(os.path.join(directory, "parent_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(directory, "accuracy.npy"), np.array([r["accuracy"] for r in res], dtype=np.float64))
    np.save(os.path.join(directory, "topk_accuracy.npy"), np.array([r["topk_accuracy"] for r in res], dtype=np.float64))


class Ctx(object):
    """What every workload of one bench process shares: the rank's place in the job, its device, the collectives."""


def setup(args):
    c = Ctx()
    c.rank = int(os.environ.get("RANK", "0"))
    c.world = int(os.environ.get("WORLD_SIZE", "1"))
    c.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if c.world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d: start one rank per GPU (or let `python bench.py --gpus N` start them)" % (args.gpus, c.world))
    c.no_torch = c.world == 1 and args.sync == "engine"
    if c.no_torch:
        c.torch = None
        # (no torch to ask for a GPU: the host-emulation build of the tests is known by its file name)
        c.emulated = args.lib is not None and os.path.basename(args.lib).endswith("_emu.so")
        c.device = 0
    else:
        import torch

        c.torch = torch
        c.emulated = args.lib is not None and not torch.cuda.is_available()
    if c.emulated:
        c.device = 0
        os.environ.setdefault("TW_TILE", "1")
        os.environ.setdefault("TW_COOP_THREADS", "1")
    elif not c.no_torch:
        ndev = c.torch.cuda.device_count()
        if ndev < 1:
            sys.exit("bench.py: no GPU visible (the HIP engine has no CPU fallback)")
        if args.backend == "nccl" and int(os.environ.get("LOCAL_WORLD_SIZE", c.world)) > ndev:
            sys.exit("bench.py: %d ranks on this node but only %d GPU(s) visible" % (int(os.environ.get("LOCAL_WORLD_SIZE", c.world)), ndev))
        c.device = c.local_rank % ndev
        c.torch.cuda.set_device(c.device)
    c.dist = None
    if c.world > 1:
        import torch.distributed as dist

        c.dist = dist
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=c.torch.device("cuda", c.device))
        else:
            dist.init_process_group(backend="gloo")
    c.red_dev = "cuda" if (args.backend == "nccl" and not c.emulated) else "cpu"
    return c


def run_workload(args, c, primary=True):
    """One workload on the ranks of this job: load, warm up, the timed step loop between barriers, the bench line (a dict
    on rank 0, None elsewhere).  `primary`: the workload the driver's line is quoted on (only it carries the single-GPU
    extras: regimes, CPU baseline, ingest / end-to-end legs)."""
    rank, world, device, dist, torch, emulated, no_torch, red_dev = c.rank, c.world, c.device, c.dist, c.torch, c.emulated, c.no_torch, c.red_dev
    from traceweaver_amd import sharding
    from traceweaver_amd.engine import Engine

    strong = args.workload in ("alibaba", "alibaba-full", "media-split")
    split = args.workload == "media-split"
    full = args.workload == "alibaba-full"
    all_units, all_truth, wl_name = make_units(args, 1000 + (0 if strong else rank))
    levels, unit_factor = [None], None
    if full:
        # exp5's load levels (exps/exp5/run_experiment.sh:60-156): every call graph at every --compress_factor; a service's load
        # factor follows from the replica table (executor.py:1089-1097).  Every (level, service) pair is a unit of its own: the
        # services are uploaded once per level and ALL levels are resident together -- one tw_scale_load call per step scales
        # each copy to its level on the device, then one step solves the whole matrix (six small solves one after the other
        # left the GPU mostly idle, and cost five more round trips through tw_scale_load)
        from traceweaver_amd import synth, transforms

        levels = [float(x) for x in args.levels.split(",")]
        replicas_all = synth.alibaba_replicas(10, len(all_units))
        n_base = len(all_units)
        unit_factor = [transforms.load_factor(f, r) for f in levels for r in replicas_all]   # unit id = level index * n_base + service
        all_units = [u for _ in levels for u in all_units]
        all_truth = [t for _ in levels for t in all_truth]
    whole_units, whole_truth = all_units, all_truth
    part_service, part_order, part_base = [], [], []
    if split:   # every service in `world` parts (fewer if it has too few idle block boundaries)
        parts, ptruth = [], []
        for sidx, (u, tp) in enumerate(zip(whole_units, whole_truth)):
            cuts = sharding.split_points(u, world)
            edges = [0] + cuts + [u.n_in]
            for k, p in enumerate(sharding.split_unit(u, cuts)):
                parts.append(p); part_service.append(sidx); part_order.append(k); part_base.append(edges[k])
                ptruth.append(np.where(tp[:, edges[k]:edges[k + 1]] >= 0, tp[:, edges[k]:edges[k + 1]] - edges[k], -1).astype(np.int32))
        all_units, all_truth = parts, ptruth
    eng = Engine(device, lib_path=args.lib)
    fit_eng = Engine(device, lib_path=args.lib) if split else None
    if strong:
        # measured work per unit: leaves enumerated by a pass over the whole slice would need a first run; the static
        # estimate is spans x endpoints, refined with the measured leaves of the warm-up pass below
        costs = [sharding.unit_cost(u) for u in all_units]
        parts = sharding.shard_units(costs, world)
        mine = parts[rank]
    else:
        mine = list(range(len(all_units)))
    units = [all_units[k] for k in mine]
    truth = [all_truth[k] for k in mine]
    spans_rank = sum(u.n_spans for u in units)
    eng.load(units)
    eng.set_truth(truth)

    on_device = dist is not None and red_dev == "cuda"   # collectives on the engine's device buffers (sharding.*_device)

    def sync():
        if not emulated and not no_torch:
            torch.cuda.synchronize()

    def barrier():
        sync()
        if world > 1:
            dist.barrier()
        sync()

    def step():
        """One step: (t1, t2, res, gathered)."""
        if full:   # the resident table, as uploaded, every copy scaled to its level (helpers/transforms.py:10-40 on the device)
            eng.scale_load([unit_factor[k] for k in mine])
        if split:   # pass 1 -> gap rows of all parts on every rank -> the same refit everywhere -> pass 2
            eng.run_pass1()
            t1 = eng.timing()
            if on_device:   # the gap rows are gathered from / joined in / refitted from device memory (RCCL on the engine's buffers)
                sharding.refit_split_services_device(eng, fit_eng, parts, all_units, part_service, part_order, whole_units, dist)
            else:
                sharding.refit_split_services(eng, fit_eng, mine, part_service, part_order, whole_units, dist=dist, device=red_dev)
            eng.run_pass2()
            t2 = eng.timing()
            t2["fit"] = fit_eng.timing()["fit"]
            res = eng.evaluate()
        else:
            t1, t2, res = one_step(eng, args.fit, mine)
        gathered = None
        if strong and on_device:   # the exchange step on the engine's own buffer: one ncclAllGather, parents on the host of rank 0 only
            gathered = sharding.gather_parents_device(eng, parts, all_units, dist, host_ranks=(0,))
        elif strong:  # (gloo / one process) the same exchange through host memory
            local = [r["parent"] for r in eng.results(2, fields=("parent",))]
            gathered = sharding.gather_parents(local, mine, len(all_units), dist=dist, device=red_dev)
        return t1, t2, res, gathered

    if strong and world > 1 and args.warmup > 0:
        # re-balance on measured work: enumerated tuples per unit from a first pass (candidate products span orders of
        # magnitude, the static estimate does not see them); every rank computes the same partition
        if full:
            eng.scale_load([unit_factor[k] for k in mine])
        eng.run_pass1()
        leaves = np.zeros(len(all_units), dtype=np.float64)
        for k, r in zip(mine, eng.results(1, fields=("leaves",))):
            leaves[k] = float(r["leaves"].sum())
        t = torch.from_numpy(leaves).to(red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        leaves = t.cpu().numpy()
        costs = [sharding.unit_cost(u, measured_leaves=float(l)) for u, l in zip(all_units, leaves)]
        parts = sharding.shard_units(costs, world)
        mine = parts[rank]
        units = [all_units[k] for k in mine]
        truth = [all_truth[k] for k in mine]
        spans_rank = sum(u.n_spans for u in units)
        eng.load(units)
        eng.set_truth(truth)

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    enum_ms, sel_ms, fit_ms, pass_ms, rep_ms, rounds = [], [], [], [], [], []
    for _ in range(args.steps):
        t1, t2, res, gathered = step()
        enum_ms += [t1["enumerate"], t2["enumerate"]]
        sel_ms += [t1["select"], t2["select"]]
        rep_ms += [t1["repair"], t2["repair"]]
        rounds += [t1["rounds"], t2["rounds"]]
        fit_ms += [t2["fit"]]
        pass_ms += [t1["pass"], t2["pass"]]
    barrier()
    dt = time.perf_counter() - t0
    stats2 = eng.results(2, fields=("unit_stats",))
    counters = np.array([sum(r[k] for r in stats2) for k in ("budget_windows", "repaired_windows", "n_windows", "cnt_unassigned")], dtype=np.float64)
    acc_sum = np.array([sum(r["correct"] for r in res), sum(r["n_in"] for r in res)], dtype=np.float64)
    per_rank_spans = [spans_rank]
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        s = torch.zeros(world, dtype=torch.float64, device=red_dev)
        s[rank] = spans_rank
        dist.all_reduce(s, op=dist.ReduceOp.SUM)
        per_rank_spans = [int(x) for x in s.cpu().tolist()]
        cc = torch.from_numpy(np.concatenate([counters, acc_sum])).to(red_dev)
        dist.all_reduce(cc, op=dist.ReduceOp.SUM)
        cc = cc.cpu().numpy()
        counters, acc_sum = cc[:4], cc[4:]
    # who ran: the process group's own view (world size, backend) and the device every rank drove -- into the detail file, so that
    # the first run on several physical GPUs can be read against what it was meant to be
    ranks_info = {"world_size": world, "backend": "none", "device_of_rank": [int(device)], "emulated": bool(emulated),
                  "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}
    if world > 1:
        dv = torch.zeros(world, dtype=torch.float64, device=red_dev)
        dv[rank] = float(device)
        dist.all_reduce(dv, op=dist.ReduceOp.SUM)
        ranks_info.update({"world_size": int(dist.get_world_size()), "backend": str(dist.get_backend()), "device_of_rank": [int(x) for x in dv.cpu().tolist()]})
    if not emulated and not no_torch:
        ranks_info["device_name"] = torch.cuda.get_device_name(device)
    spans_total = float(sum(per_rank_spans))   # (alibaba-full: every level is a reconstruction of all spans -- its units hold them)
    acc_levels = []
    if full:
        lv = np.zeros((len(levels), 2), dtype=np.float64)
        for k, r in zip(mine, res):
            lv[k // n_base] += (r["correct"], r["n_in"])
        if world > 1:
            tl = torch.from_numpy(lv).to(red_dev)
            dist.all_reduce(tl, op=dist.ReduceOp.SUM)
            lv = tl.cpu().numpy()
        acc_levels = [float(a / max(b, 1)) for a, b in lv]
    acc = float(np.mean([r["accuracy"] for r in res])) if not strong else float(acc_sum[0] / max(acc_sum[1], 1))
    host = None
    if args.full or strong or args.dump_outputs:
        host = eng.results(2, fields=("parent",))      # outside the timed region
    from traceweaver_amd import synth

    if args.full and not full:   # cross-check of the device reduction (a scaled table is re-sorted on the device together with its ground truth: the host's copy is in upload order)
        host_acc = [synth.accuracy(r["parent"], tp) for r, tp in zip(host, truth)]
        assert all(abs(a - r["accuracy"]) < 1e-12 for a, r in zip(host_acc, res)), "device accuracy reduction differs from the host's"
    if args.dump_outputs and rank == 0:   # before --verify below reloads the engine
        whole = strong and gathered is not None and all(g is not None for g in gathered)
        dump_outputs(args.dump_outputs, gathered if whole else [r["parent"] for r in host], res)
    verified = None
    if strong and gathered is not None:
        for k, p in zip(mine, host):
            assert np.array_equal(gathered[k], p["parent"]), "gathered parents differ from the local result"
        assert all(g is not None for g in gathered), "the gather left a unit out"
    if strong:
        if args.verify and rank == 0 and (world > 1 or split):
            eng.load(whole_units)
            eng.set_truth(whole_truth)
            if full:
                eng.scale_load(unit_factor)
            one_step(eng, args.fit)
            alone = eng.results(2, fields=("parent",))
            if split:   # stitch the parts of every service
                stitched = []
                for sidx in range(len(whole_units)):
                    ks = sorted((k for k in range(len(all_units)) if part_service[k] == sidx), key=lambda k: part_order[k])
                    stitched.append(np.concatenate([np.where(gathered[k] >= 0, gathered[k] + part_base[k], -1) for k in ks], axis=1))
                verified = all(np.array_equal(g, a["parent"]) for g, a in zip(stitched, alone))
            else:
                verified = all(np.array_equal(g, a["parent"]) for g, a in zip(gathered, alone))
            assert verified, "sharded result differs from the single-GPU result"
    out = None
    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = spans_total * args.steps / dt
        # dominant kernel group, measured live with HIP events on the engine's stream (tw_get_timing): the
        # enumeration / selection / repair kernels run once per pass, the refit once per step
        groups = {"k_enumerate": float(np.mean(enum_ms)), "k_select": float(np.mean(sel_ms)), "k_repair": float(np.mean(rep_ms)),
                  "k_fit": float(np.mean(fit_ms))}
        dominant = max(groups, key=lambda k: groups[k] * (1 if k == "k_fit" else 2))
        alg_bytes = float(ALG_BYTES_PER_SPAN_PER_PASS) * spans_rank  # per launch of a per-pass kernel group
        achieved = alg_bytes / (groups[dominant] * 1e-3) / 1e9
        traffic, traffic_src = (None, None) if (emulated or not primary) else profile_traffic(dominant, spans_rank)
        out = {
            "metric": "spans/sec reconstructed + assignment accuracy vs ground truth",
            "value": value, "unit": "spans/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": "int64 timestamps, f64 scores", "data": "synthetic",
            "config": {"workload": wl_name + ", two-pass reconstruction, %s mixture refit" % args.fit,
                       "spans_per_gpu": per_rank_spans[0] if len(set(per_rank_spans)) == 1 else per_rank_spans, "spans_total": int(spans_total),
                       "parallelism": "units sharded, %d rank(s), backend %s" % (world, args.backend if world > 1 else "none")},
            "accuracy": acc,
            "reference_shape": {"media": "media", "media-split": "media", "nodejs": "nodeio"}.get(args.workload, "alibaba"),
            **({"accuracy_by_level": dict(zip(args.levels.split(","), acc_levels))} if full else {}),
            "budget_windows": int(counters[0]), "repaired_windows": int(counters[1]), "windows": int(counters[2]), "unassigned": int(counters[3]),
            "repair_rounds_per_pass": float(np.mean(rounds)),
            "ranks": ranks_info,
            "gpu_pass_ms": {"pass1": float(np.mean(pass_ms[0::2])), "pass2": float(np.mean(pass_ms[1::2]))},
            "roofline": {"bound": "hbm", "kernel": dominant, "achieved": achieved, "peak": HBM_PEAK_GBPS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": traffic_src,
                         "kernel_ms": groups[dominant], "algorithmic_bytes_per_launch": alg_bytes,
                         "group_ms_per_launch": groups},
        }
        if verified is not None:
            out["sharded_equals_single_gpu"] = bool(verified)
        if args.full and primary and not emulated and world == 1:
            out["roofline"]["peak_measured"] = eng.hbm_copy_gbps()
        if args.full and primary and args.regimes and world == 1 and not emulated and args.workload == "media" and args.concurrency is None:
            out["regimes"] = run_regimes(args, eng)
        if args.full and primary and args.cpu_sample > 0 and world == 1:
            out["cpu_baseline"] = cpu_baseline(args, 1000)
            import tempfile

            n_hotel, n_ali = (int(x) for x in args.host_traces.split(","))
            for kind, n_traces, tag in (("hotel", n_hotel, ""), ("alibaba", n_ali, "_alibaba")):   # each corpus is written once
                with tempfile.TemporaryDirectory() as d:
                    corpus = _corpus(kind, d, n_traces)
                    out["ingest" + tag] = ingest_rate(lib=args.lib, kind=kind, n_traces=n_traces, corpus=corpus)
                    if args.end_to_end:
                        out["end_to_end" + tag] = end_to_end(device, lib=args.lib, kind=kind, n_traces=n_traces, corpus=corpus)
                        # the same chain on later runs over the same directory: from the span table cache the first run left in it
                        out["end_to_end_cached" + tag] = end_to_end(device, lib=args.lib, kind=kind, n_traces=n_traces, corpus=corpus, cache_dir=d)
            if args.end_to_end:
                out["load_levels"] = load_levels(device, lib=args.lib)
                out["shipped_corpora"] = shipped_corpora(device, lib=args.lib)
    eng.close()
    if fit_eng is not None:
        fit_eng.close()
    return out


def _r(x, sig=6):
    """Floats of the compact line: six significant digits."""
    if isinstance(x, float):
        return float("%.*g" % (sig, x))
    if isinstance(x, dict):
        return {k: _r(v, sig) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, sig) for v in x]
    return x


def write_detail(args, out):
    """The full record of a run: --detail-file, by default gpurun_out/bench_detail_n<N>.json under the repository (the
    directory gpurun merges back).  Returns the path relative to the repository, or None if nothing could be written."""
    path = args.detail_file or os.path.join(REPO, "gpurun_out", "bench_detail_n%d.json" % args.gpus)
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    except OSError:
        return None
    return os.path.relpath(path, REPO)


def compact_line(out, detail_path=None):
    """The one line the driver parses: the bench contract's keys, `roofline`, `cpu_baseline`, one number per regime --
    everything else is in the detail file.  Kept under 2 KB (tests/test_bench_line.py)."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
            "config", "accuracy", "accuracy_by_level", "budget_windows", "repaired_windows", "windows", "unassigned", "gpu_pass_ms",
            "sharded_equals_single_gpu")
    line = {k: out[k] for k in keep if k in out}
    # accuracy is the algorithm's accuracy against ground truth -- the assignments themselves are oracle-identical (tests/, -m gpu)
    line["accuracy_is"] = "vs ground truth; assignments == CPU oracle"
    rf = out["roofline"]
    line["roofline"] = {k: rf[k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms", "peak_measured") if k in rf}
    cb = out.get("cpu_baseline")
    if cb:
        c = {k: cb[k] for k in ("value", "unit", "cores", "kind", "sample") if k in cb}
        if cb.get("all_cores"):
            c["all_cores"] = {k: cb["all_cores"].get(k) for k in ("value", "cores")}
        ref = (cb.get("reference") or {}).get("shapes", {}).get(out.get("reference_shape", "media"))
        if ref:
            c["reference"] = {"value": ref["value"], "unit": ref["unit"], "cores": ref["cores"], "kind": "reference",
                              "measured_in": "build container, 1 core, HiGHS for Gurobi (profiles/cpu_reference.json)"}
        line["cpu_baseline"] = c
    if "regimes" in out:
        line["regimes_spans_per_s"] = {k: v["value"] for k, v in out["regimes"].items()}
    if "scale_regimes" in out:
        line["scale_regimes"] = {
            key: {**{k: r[k] for k in ("value", "ms_per_step", "scaling", "n_gpus", "accuracy", "accuracy_by_level", "budget_windows",
                                       "sharded_equals_single_gpu") if k in r},
                  "roofline": {"kernel": r["roofline"]["kernel"], "frac": r["roofline"]["frac"]}}
            for key, r in out["scale_regimes"].items()}
    for k in ("end_to_end", "end_to_end_alibaba", "shipped_corpora"):
        if out.get(k):
            line.setdefault("host_legs_spans_per_s", {})[k] = out[k]["value"]
    if detail_path:
        line["detail"] = detail_path
    return _r(line)


SCALE_REGIMES = [   # (key, workload): what `--gpus N > 1` without --workload measures next to the weak-scaling media line
    ("config4_alibaba_slice_sharded", "alibaba"),          # BASELINE config 4: one 1 M-span slice sharded per service, all-gather of parents
    ("config5_alibaba_full_sharded", "alibaba-full"),      # BASELINE config 5: 15 call graphs x 6 load levels resident, one step
]


def main():
    args = parse_args()
    if args.cpu_worker:   # a process of cpu_all_cores
        spans, dt, _ = _cpu_sample(args, 1000)
        print(json.dumps({"spans": spans, "seconds": dt}))
        return
    if args.gpus < 1:
        sys.exit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args))
    c = setup(args)
    out = run_workload(args, c, primary=True)
    if args.full and args.default_line and c.world > 1 and args.scale_regimes:
        # the driver's multi-GPU line: next to the weak-scaling media workload (no data-path collective) the two sharded modes
        # north_star names -- strong scaling, every step ends with the all-gather of the parent arrays (RCCL on the engine's
        # device buffers with backend nccl), each verified on rank 0 against the single-GPU result
        import copy

        regs = {}
        for key, workload in SCALE_REGIMES:
            a = copy.copy(args)
            a.workload, a.verify, a.concurrency, a.replicas = workload, 1, None, None
            a.steps, a.warmup = min(args.steps, 5), min(max(args.warmup, 1), 2)
            r = run_workload(a, c, primary=False)
            if c.rank == 0:
                regs[key] = {k: r[k] for k in ("value", "unit", "n_gpus", "steps", "ms_per_step", "scaling", "config", "accuracy", "budget_windows",
                                               "sharded_equals_single_gpu", "roofline", "ranks", "gpu_pass_ms") if k in r}
                if "accuracy_by_level" in r:
                    regs[key]["accuracy_by_level"] = r["accuracy_by_level"]
        if c.rank == 0:
            out["scale_regimes"] = regs
    if c.rank == 0:
        # the full record (regimes with their roofline blocks, the reference's per-shape timings, host legs) goes to a file; the LAST
        # stdout line is the compact record the driver parses (round 4's 20 KB line did not fit the driver's 8 KB tail)
        path = write_detail(args, out) if (args.full or args.detail_file) else None
        print(json.dumps(compact_line(out, path), separators=(",", ":")))
    if c.world > 1:
        c.dist.barrier()
        c.dist.destroy_process_group()


if __name__ == "__main__":
    main()
