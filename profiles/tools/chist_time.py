"""Times the class catalogue (tw_class_history_*, csrc/tw_chist.h) on one MI355X.  Writes one JSON document.

Two resident batches -- the media-shape table of profiles/prof_time.json (few classes) and an Alibaba-shape one whose callee rows are
spread over 60 groups, so that nearly every trace has a shape of its own (many classes): tw_get_timing slots 43..45 of a first push
(all insertions) and of a second push of the same batch (all hits), the wall clock of a match, and beside them the yardstick of the
same run: slot 27 of the tw_trace_signatures call (classes, comparison, per-class reduction) and slots 28..30 of tw_class_profiles,
which compute what is pushed.  The ratio is reported, not asserted.

A synthetic merge: --classes generated classes of 11 to 13 entries into a catalogue that holds as many, half of them shared: the three
slots, the bytes moved (the source's entries read twice, the matched catalogue entries once, the figures read and written) and their
share of tw_measure_hbm_copy's rate, taken in the same run.

    python profiles/tools/chist_time.py --out profiles/chist_time.json
    python profiles/tools/chist_time.py --sizes 1x500 --alibaba 4000 --classes 300 --lib <host build>    # a rehearsal without a GPU
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conf_time import span_table  # noqa: E402
from traceweaver_amd import synth, traces  # noqa: E402
from traceweaver_amd.engine import Engine  # noqa: E402

SLOTS = ("lookup", "insert", "accumulate")


def measure(eng, units, rows, group, n_groups, rounds, check):
    eng.load(units)
    eng.run_pass1()
    eng.fit_mixtures(seed=0)
    eng.run_pass2()
    eng.set_span_rows(*rows)
    eng.set_row_groups(group, n_groups)
    st = eng.stitch()
    out = {"rows": len(rows[2]), "trees": st.n_trees, "hbm_copy_gbps": eng.hbm_copy_gbps()}
    for mode in traces.SIGNATURE_MODES:
        runs = []
        for k in range(rounds + 1):
            eng.class_history_reset()
            eng.attribute(percentile=0.0)                         # (drops the profile: class_profiles computes again)
            eng.score_traces(0.0)                                 # (drops the signature result: signatures computes again)
            s = eng.signatures(mode)
            eng.class_profiles()
            run = {"sig_classes_ms": eng.signatures_timing()["classes"], "profiles_ms": eng.profiles_timing()}
            _, first = eng.class_history_push(3, 0)
            run["first_push_ms"] = eng.class_history_timing()
            _, second = eng.class_history_push(3, 1)
            run["second_push_ms"] = eng.class_history_timing()
            t0 = time.perf_counter()
            found = eng.class_history_match()
            run["match_wall_ms"] = (time.perf_counter() - t0) * 1e3
            assert first[0] == s.n_classes and second[0] == 0 and (found >= 0).all()
            yard = run["sig_classes_ms"] + sum(run["profiles_ms"].values())
            run["first_push_over_yardstick"] = sum(run["first_push_ms"].values()) / yard if yard > 0 else None
            run["second_push_over_yardstick"] = sum(run["second_push_ms"].values()) / yard if yard > 0 else None
            runs.append(run)
        best = min(runs[1:], key=lambda r: sum(r["first_push_ms"].values()))
        out[mode] = dict(best, classes=s.n_classes, entries=len(s.class_entries), capacity=eng.class_history_info()["capacity"], all=runs)
        if check:
            p = eng.class_profiles()
            out[mode]["equals_host"] = bool(eng.class_history().same_as(traces.class_history_host([(s, p, 3, 0), (s, p, 3, 1)])))
    eng.class_history_reset()
    return out


def media(eng, replicas, n_in, rounds, check):
    units, _ = synth.make_workload(7, n_in, services=synth.MEDIA_SERVICES, replicas=replicas, concurrency=1.6)
    rows, group = span_table(units)
    return measure(eng, units, rows, group, 8, rounds, check)


def alibaba(eng, total_spans, rounds):
    """The Alibaba-shape batch with the callee rows spread over 60 groups by their row number: shapes by the hundred thousand."""
    units, _, _ = synth.make_alibaba_workload(3, total_spans)
    rows, group = span_table(units)
    r = np.arange(len(group), dtype=np.int64)
    group = np.where(group >= 4, 4 + (r * 2654435761 >> 7) % 60, group).astype(np.int32)
    return measure(eng, units, rows, group, 64, rounds, False)


def generated(lo, n, n_groups=8):
    """Classes lo .. lo + n: class i has 11 + i % 3 entries (level b, 0, b mod G, 1 + two bits of i), distinct by construction."""
    ids = np.arange(lo, lo + n, dtype=np.int64)
    length = 11 + ids % 3
    off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    cls = np.repeat(ids, length)
    b = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], length)
    entries = np.stack([b, np.zeros_like(b), b % n_groups, 1 + ((cls >> (2 * b)) & 3)], axis=1).astype(np.int32)
    cell = cls * 16 + b
    figures = dict(trees=ids + 1, latency_sum=7 * ids, latency_min=ids, latency_max=ids + 9, counted=np.ones_like(ids), latency=3 * ids)
    figures.update({f: cell for f in traces.PROFILE_ENTRY_FIELDS})
    return traces.ClassHistory(off, entries, mode=0, n_groups=n_groups, **figures)


def merge(eng, n, check):
    gbps = eng.hbm_copy_gbps()
    eng.class_history_reset()
    held, src = generated(0, n), generated(n // 2, n)
    eng.class_history_merge(held, 0)
    fill = eng.class_history_timing()
    _, summary = eng.class_history_merge(src, 1)
    t = eng.class_history_timing()
    assert summary[0] == n - (n - n // 2) and summary[1] == n + n // 2
    matched = int(held.class_off[-1] - held.class_off[n // 2])   # entries of the shared classes
    ne, nc = src.n_entries, src.n_classes
    moved = {"lookup": 16 * ne + 16 * matched + 8 * (nc + 1), "insert": 2 * 16 * int(summary[2]) + 9 * 8 * (int(summary[2]) + int(summary[0])),
             "accumulate": 9 * 24 * ne + 9 * 24 * nc + 8 * ne}
    out = {"classes_held": n, "classes_source": n, "shared": n - n // 2, "entries_source": ne, "hbm_copy_gbps": gbps, "fill_ms": fill, "merge_ms": t,
           "bytes": moved, "capacity": eng.class_history_info()["capacity"],
           "of_copy_rate": {k: moved[k] / t[k] / 1e6 / gbps if t[k] > 0 and gbps > 0 else None for k in SLOTS},
           "whole_of_copy_rate": sum(moved.values()) / sum(t.values()) / 1e6 / gbps if sum(t.values()) > 0 and gbps > 0 else None}
    if check:
        out["equals_host"] = bool(eng.class_history().same_as(traces.class_history_host([(held, None, 0, 0), (src, None, 0, 1)])))
    eng.class_history_reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1x8000,16x125000", help="media shape: replicas x requests per service, comma separated; the first one is checked against the host restatement")
    ap.add_argument("--alibaba", type=int, default=4000000, help="engine spans of the Alibaba-shape batch (0: left out)")
    ap.add_argument("--classes", type=int, default=1000000, help="classes of the synthetic merge, into as many held (0: left out)")
    ap.add_argument("--rounds", type=int, default=2, help="rounds per batch and mode after a warm-up: the best first push is reported, all are listed")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    eng = Engine(0, lib_path=args.lib)
    doc = {"what": "the class catalogue on one MI355X, same batch and process: HIP events of tw_get_timing slots 43..45 (k_chist_lookup: hash and lookup; the scan "
                   "over the misses, k_chist_append, k_chist_insert and any growth and rehash, with the host's reads in between; k_chist_accumulate) of a first "
                   "push of a batch (all insertions) and of a second push of it (all hits), the wall clock of a match; beside them slot 27 (sig_classes_ms) "
                   "of the tw_trace_signatures call and slots 28..30 (profiles_ms) of the tw_class_profiles call that computed what is pushed: "
                   "*_over_yardstick = the three slots / (27 + 28 + 29 + 30).  synthetic_merge: generated classes of 11 to 13 entries merged into a catalogue "
                   "that holds as many, half of them shared; bytes = the source's entries read twice (hash, compare or append) and the matched entries "
                   "once (lookup, insert), the figures read and written (accumulate); of_copy_rate against hbm_copy_gbps of the same run."}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")

    def note(key):
        print(key, json.dumps({m: {a: doc[key][m][a] for a in ("classes", "entries", "first_push_ms", "second_push_ms", "match_wall_ms", "sig_classes_ms",
                                                                 "profiles_ms", "first_push_over_yardstick")} for m in traces.SIGNATURE_MODES}), flush=True)
        write()                                                   # (what has been measured so far survives a run that is cut short)

    for k, size in enumerate(args.sizes.split(",")):
        r, n = (int(x) for x in size.split("x"))
        doc["media_shape_%dx%d" % (r, n)] = media(eng, r, n, args.rounds, check=k == 0)
        note("media_shape_%dx%d" % (r, n))
    if args.alibaba > 0:
        doc["alibaba_shape_%d" % args.alibaba] = alibaba(eng, args.alibaba, args.rounds)
        note("alibaba_shape_%d" % args.alibaba)
    if args.classes > 0:
        doc["synthetic_merge"] = merge(eng, args.classes, check=args.classes <= 20000)
        print("synthetic_merge", json.dumps(doc["synthetic_merge"]), flush=True)
    eng.close()
    write()
    if not args.out:
        print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
