"""From parent arrays to traces: the arguments and the result of Engine.stitch (tw_stitch_traces, csrc/tw_stitch.h).

The engine answers per service: parent[e][i] = the call of endpoint e that belongs to request i.  A trace is what these
answers say together with the hops that are observed (an RPC is logged on both sides: the callee's server span names the
caller's client span).  `rows_from_units` builds what Engine.set_span_rows takes from the ingest's units and span table,
`StitchedTraces` is what Engine.stitch returns, `write_npz` stores it with the (trace id, span id) strings of every row,
and `stitch_host` restates the device's computation in numpy -- test and cross-check code; the product path is the device.

Engine.attribute (tw_attribute_traces, csrc/tw_attr.h) answers the delay-culprit query on the stitched forest: `Attribution`
is its result, `groups_from_table` the usual grouping (by service), `write_attribution_npz` stores it, and `attribute_host`
restates the definitions in plain recursive Python -- the yardstick of the tests, nothing else.

Engine.decisions / Engine.score_traces (tw_get_decisions, tw_score_traces, csrc/tw_conf.h) say which traces can be trusted:
`TraceConfidence` is the result, `decisions_host` and `confidence_host` restate the per-request and the per-tree definitions
in numpy for the tests, `write_confidence_npz` stores the result.

Engine.set_row_cohorts / Engine.distributions (tw_set_row_cohorts, tw_latency_distributions, csrc/tw_dist.h) give the populations
behind an attribution: `LatencyDistributions` is the result, `distributions_host` restates the definitions in numpy for the
tests, `compare_distributions` sets two results side by side (predicted against true, cohort against cohort) on the host,
`write_distributions_npz` stores a result.

Engine.signatures (tw_trace_signatures, csrc/tw_sig.h) groups the stitched traces by call-graph signature: `TraceSignatures` is the
result, `signatures_host` restates the definitions with dictionaries of tuples for the tests, `compare_signatures` cross-checks
tree_same on the host and gives the share of traces with the true signature, `write_signatures_npz` stores results.

Engine.class_profiles (tw_class_profiles, csrc/tw_prof.h) joins the last two: per class and signature entry the times of the selected
trees of that shape -- the aggregate trace of a class.  `ClassProfiles` is the result, `class_profiles_host` restates the definitions
with dictionaries from the host results of `signatures_host` and `attribute_host`, `write_profiles_npz` stores results.

Engine.filter_traces (tw_filter_traces, csrc/tw_filt.h) selects the stitched traces by a predicate and marks them with bit MATCH of
the device forest's flags, which all of the above select by: `clause` builds a clause, `parse_filter` / `format_filter` are the
command line's language, `TraceFilter` is the result, `filter_host` restates the definitions with loops over the rows of a tree for
the tests, `write_filter_npz` stores a result.

Engine.extract_traces (tw_extract_traces / tw_get_extracted, csrc/tw_extr.h) hands out reconstructed traces as trees: `ExtractedTraces` is
the result (every selected tree in pre-order with local parent indices; `render` draws one), `extract_host` restates the definitions
with sorted() and a recursion over the children for the tests, `write_extracted_npz` stores a result and `write_jaeger` writes every
extracted trace as a Jaeger JSON file in the shape the corpus came in.
"""
import sys

import numpy as np

WHOLE, UNASSIGNED, EXACT = 1, 2, 4   # bits of tree_flags
CONFIDENT = 8                        # ... of the forest on the device after Engine.score_traces (Engine.attribute(need_flags=WHOLE | CONFIDENT))


class StitchedTraces(object):
    """root / depth [n_rows]: root row of every row's tree and the links between the row and it; tree k (trees in
    ascending order of root row) owns tree_rows[tree_off[k]:tree_off[k + 1]], ordered by (start, row); tree_root /
    tree_latency / tree_flags [n_trees] (WHOLE: the root is a root of the span table, every other tree is a fragment;
    UNASSIGNED: some request of the tree has an endpoint without a call; EXACT, with ground truth set: whole and the same
    rows as the true trace); counts = whole traces, fragments, trees with an unassigned endpoint, exact trees (-1: no truth)."""

    FIELDS = ("root", "depth", "tree_off", "tree_rows", "tree_root", "tree_latency", "tree_flags", "counts")

    def __init__(self, root, depth, tree_off, tree_rows, tree_root, tree_latency, tree_flags, counts):
        self.root, self.depth, self.tree_off, self.tree_rows = root, depth, tree_off, tree_rows
        self.tree_root, self.tree_latency, self.tree_flags = tree_root, tree_latency, tree_flags
        self.counts = np.asarray(counts, dtype=np.int64)

    @property
    def n_trees(self):
        return len(self.tree_root)

    def __len__(self):
        return self.n_trees

    def trace(self, k):
        """Tree k: {"root", "rows" (ordered by start), "latency", "whole", "unassigned", "exact"}."""
        k = int(k)
        if not 0 <= k < self.n_trees:
            raise IndexError(k)
        f = int(self.tree_flags[k])
        return {"root": int(self.tree_root[k]), "rows": self.tree_rows[int(self.tree_off[k]):int(self.tree_off[k + 1])],
                "latency": int(self.tree_latency[k]), "whole": bool(f & WHOLE), "unassigned": bool(f & UNASSIGNED), "exact": bool(f & EXACT)}

    def __iter__(self):
        return (self.trace(k) for k in range(self.n_trees))

    def same_as(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.FIELDS)


def rows_from_units(units, table, deleted=None):
    """Arguments of Engine.set_span_rows for a batch of IngestedUnits (in load order) and Corpus.span_table():
    (in_rows, out_rows, row_link, row_kind, row_start, row_end).  `deleted`: rows of calls that were taken out of the batch
    (skipmode.cache_hits removes the calls a cache hit did not make): they are absent from the table handed over, and the
    server spans that name one of them as their caller have no observed link (-2) -- they are not roots of the table either."""
    link = np.array(table["parent"], dtype=np.int32)
    kind = np.array(table["kind"], dtype=np.uint8)
    start = np.asarray(table["start"], dtype=np.int64)
    end = start + np.asarray(table["duration"], dtype=np.int64)
    if deleted is not None and len(deleted):
        gone = np.zeros(len(link), dtype=bool)
        gone[np.asarray(deleted, dtype=np.int64)] = True
        link[(link >= 0) & gone[np.maximum(link, 0)]] = -2
        kind[gone] = 0
    return ([u.in_rows for u in units], [list(u.out_rows) for u in units], link, kind, start, end)


def stitch_host(units, parents, in_rows, out_rows, row_link, row_kind, row_start, row_end, truth=None):
    """What tw_stitch_traces computes, in plain numpy.  units: the UnitArrays of the batch, parents: per unit [E, n_in]
    (the assignment to stitch), truth: per unit the true [E, n_in] arrays when the EXACT bit is wanted."""
    row_link = np.asarray(row_link, dtype=np.int64)
    row_kind = np.asarray(row_kind)
    n = len(row_link)
    rows = np.arange(n, dtype=np.int64)

    def forest(par):
        link = np.where((row_kind == 1) & (row_link >= 0), row_link, -1)
        una = np.zeros(n, dtype=bool)
        for u, p, ir, per in zip(units, par, in_rows, out_rows):
            ir = np.asarray(ir, dtype=np.int64)
            for e in range(u.E):
                x = np.asarray(p[e], dtype=np.int64)
                ok = (x >= 0) & (x < len(per[e]))
                link[np.asarray(per[e], dtype=np.int64)[x[ok]]] = ir[ok]
                una[ir[x == -1]] = True
        root = np.where(link >= 0, link, rows)
        depth = (link >= 0).astype(np.int64)
        for _ in range(64):
            nxt = root[root]
            if np.array_equal(nxt, root):
                break
            depth = depth + depth[root]
            root = nxt
        else:
            raise ValueError("the links hold a cycle")
        if np.any((root == rows) & (link >= 0)):
            raise ValueError("the links hold a cycle")
        return root, depth, una

    root, depth, una = forest(parents)
    order = np.lexsort((rows, np.asarray(row_start), root))
    tree_root = np.unique(root)
    counts = np.bincount(root, minlength=n)[tree_root]
    tree_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    k_of = np.searchsorted(tree_root, root)
    latest = np.full(len(tree_root), np.iinfo(np.int64).min, dtype=np.int64)
    np.maximum.at(latest, k_of, np.asarray(row_end, dtype=np.int64))
    whole = (row_kind[tree_root] == 1) & (row_link[tree_root] == -1)
    t_una = np.zeros(len(tree_root), dtype=bool)
    t_una[k_of[una]] = True
    flags = whole * WHOLE + t_una * UNASSIGNED
    n_exact = -1
    if truth is not None:
        t_root = forest(truth)[0]
        bad = np.zeros(n, dtype=bool)
        diff = t_root != root
        bad[root[diff]] = True
        bad[t_root[diff]] = True
        exact = whole & ~bad[tree_root]
        flags = flags + exact * EXACT
        n_exact = int(exact.sum())
    counts4 = np.array([int(whole.sum()), int(len(tree_root) - whole.sum()), int(t_una.sum()), n_exact], dtype=np.int64)
    return StitchedTraces(root.astype(np.int32), depth.astype(np.int32), tree_off, order.astype(np.int32), tree_root.astype(np.int32),
                          latest - np.asarray(row_start, dtype=np.int64)[tree_root], flags.astype(np.uint8), counts4)


def write_npz(path, stitched, corpus, table=None):
    """The stitched traces as one .npz that can be read without the corpus: the arrays of StitchedTraces plus, per row of
    the span table, the trace id the span was logged under (`row_trace_id`), its span id, service and start / end."""
    table = corpus.span_table() if table is None else table
    names = corpus.trace_names()
    trace_ids = np.array([corpus.string(x) for x in names])
    service_ids, inverse = np.unique(np.asarray(table["service"]), return_inverse=True)
    services = np.array([corpus.string(x) for x in service_ids])
    start = np.asarray(table["start"], dtype=np.int64)
    with open(path, "wb") as f:
        np.savez_compressed(
            f, root=stitched.root, depth=stitched.depth, tree_off=stitched.tree_off, tree_rows=stitched.tree_rows,
            tree_root=stitched.tree_root, tree_latency=stitched.tree_latency, tree_flags=stitched.tree_flags, counts=stitched.counts,
            row_trace_id=trace_ids[np.asarray(table["trace"])], row_span_id=np.array([corpus.string(x) for x in table["span_id"]]),
            row_service=services[inverse], row_kind=np.asarray(table["kind"]), row_start=start,
            row_end=start + np.asarray(table["duration"], dtype=np.int64))


GROUP_COLUMNS = ("path_time", "path_rows", "self_time", "span_time", "span_rows", "trees", "top_trees")


class Attribution(object):
    """link / self_time / path_time [n_rows]: the stitched links, every row's own time (duration less the union of its
    children) and its share of its tree's critical path; tree_top_group / tree_selected / tree_path_rows [n_trees]; groups
    [7, n_groups] = GROUP_COLUMNS over the selected trees (also as attributes group_<column>); summary = eligible trees,
    selected trees, rank k, latency at rank k, culprit (include/traceweaver_amd.h has the definitions)."""

    FIELDS = ("link", "self_time", "path_time", "tree_top_group", "tree_selected", "tree_path_rows", "groups", "summary")

    def __init__(self, link, self_time, path_time, tree_top_group, tree_selected, tree_path_rows, groups, summary):
        self.link, self.self_time, self.path_time = link, self_time, path_time
        self.tree_top_group, self.tree_selected, self.tree_path_rows = tree_top_group, tree_selected, tree_path_rows
        self.groups = np.asarray(groups, dtype=np.int64)
        self.summary = np.asarray(summary, dtype=np.int64)
        for c, name in enumerate(GROUP_COLUMNS):
            setattr(self, "group_" + name, self.groups[c])

    n_eligible = property(lambda self: int(self.summary[0]))
    n_selected = property(lambda self: int(self.summary[1]))
    rank = property(lambda self: int(self.summary[2]))
    rank_latency = property(lambda self: int(self.summary[3]))
    culprit = property(lambda self: int(self.summary[4]))

    def mean_latency(self, g):
        """Mean service latency of group g over the selected trees (us), nan without a row."""
        n = int(self.group_span_rows[g])
        return float(self.group_span_time[g]) / n if n else float("nan")

    def table(self, names=None):
        """One dict per group: its name, GROUP_COLUMNS, mean_latency and path_share (of the selected trees' latency)."""
        total = int(self.group_path_time.sum())
        return [dict([("group", g if names is None else names[g])] + [(c, int(self.groups[i][g])) for i, c in enumerate(GROUP_COLUMNS)] +
                     [("mean_latency", self.mean_latency(g)), ("path_share", float(self.group_path_time[g]) / total if total else 0.0)])
                for g in range(self.groups.shape[1])]

    def same_as(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.FIELDS)


def groups_from_table(table, corpus=None):
    """(row_group, names): the rows of a span table grouped by interned service, groups in ascending order of the service's
    string id; names are the services' strings when the corpus is given, their string ids otherwise."""
    ids, inverse = np.unique(np.asarray(table["service"]), return_inverse=True)
    names = [corpus.string(x) for x in ids] if corpus is not None else [int(x) for x in ids]
    return inverse.astype(np.int32), names


def critical_paths_host(children, start, end, roots):
    """(path_time, walked) of the forest with these child lists, the walk of include/traceweaver_amd.h from every root: recursive
    and obvious, for the restatements (end already clamped to start)."""
    n = len(start)
    path_time = np.zeros(n, dtype=np.int64)
    walked = np.zeros(n, dtype=bool)

    def walk(p, lo, hi):
        walked[p] = True
        cursor = hi
        while True:
            best = None
            for c in children[p]:
                cs = max(start[c], lo)
                ce = min(end[c], cursor)
                if cs < cursor and ce > cs and (best is None or (-ce, cs, c) < best[0]):
                    best = ((-ce, cs, c), c, cs, ce)
            if best is None:
                break
            _, c, cs, ce = best
            path_time[p] += cursor - ce
            walk(c, cs, ce)
            cursor = cs
        path_time[p] += cursor - lo

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 20000))
    try:
        for r in roots:
            walk(int(r), start[int(r)], end[int(r)])
    finally:
        sys.setrecursionlimit(limit)
    return path_time, walked


def attribute_host(stitched, link, row_start, row_end, row_group, n_groups, percentile=0.0, start_min=None, start_max=None,
                   need_flags=WHOLE, skip_flags=UNASSIGNED):
    """What tw_attribute_traces computes, restated from the definitions: recursive and obvious, for the tests."""
    link = np.asarray(link, dtype=np.int64)
    start = [int(x) for x in row_start]
    end = [max(int(e), s) for e, s in zip(row_end, start)]
    group = [int(x) for x in row_group]
    n = len(link)
    children = [[] for _ in range(n)]
    for c in range(n):
        if link[c] >= 0:
            children[int(link[c])].append(c)
    self_time = np.zeros(n, dtype=np.int64)
    for p in range(n):
        clipped = sorted((max(start[c], start[p]), min(end[c], end[p])) for c in children[p])
        covered, reach = 0, start[p]
        for cs, ce in clipped:
            if ce > cs:
                covered += max(0, ce - max(cs, reach))
                reach = max(reach, ce)
        self_time[p] = end[p] - start[p] - covered
    path_time, walked = critical_paths_host(children, start, end, stitched.tree_root)
    nt = stitched.n_trees
    top = np.full(nt, -1, dtype=np.int32)
    path_rows = np.zeros(nt, dtype=np.int32)
    per_tree = []
    for k in range(nt):
        rows = [int(r) for r in stitched.tree_rows[int(stitched.tree_off[k]):int(stitched.tree_off[k + 1])]]
        sums = {}
        for r in rows:
            if walked[r]:
                path_rows[k] += 1
                if group[r] >= 0:
                    sums[group[r]] = sums.get(group[r], 0) + int(path_time[r])
        if sums:
            top[k] = min(sums, key=lambda g: (-sums[g], g))
        per_tree.append((rows, sums))
    flags = np.asarray(stitched.tree_flags).astype(np.int64)
    eligible = [k for k in range(nt) if (flags[k] & need_flags) == need_flags and (flags[k] & skip_flags) == 0]
    eligible.sort(key=lambda k: (int(stitched.tree_latency[k]), k))
    rank = int(percentile * len(eligible))
    lo = -2 ** 63 if start_min is None else int(start_min)
    hi = 2 ** 63 - 1 if start_max is None else int(start_max)
    selected = np.zeros(nt, dtype=np.uint8)
    for k in eligible[rank:]:
        if lo <= start[int(stitched.tree_root[k])] < hi:
            selected[k] = 1
    groups = np.zeros((len(GROUP_COLUMNS), n_groups), dtype=np.int64)
    for k in np.flatnonzero(selected):
        rows, sums = per_tree[k]
        for r in rows:
            g = group[r]
            if g < 0:
                continue
            if walked[r]:
                groups[0, g] += path_time[r]
                groups[1, g] += 1
            groups[2, g] += self_time[r]
            groups[3, g] += end[r] - start[r]
            groups[4, g] += 1
        for g in sums:
            groups[5, g] += 1
        if top[k] >= 0:
            groups[6, top[k]] += 1
    on = [g for g in range(n_groups) if groups[1, g] > 0]
    culprit = min(on, key=lambda g: (-int(groups[0, g]), g)) if on else -1
    summary = [len(eligible), int(selected.sum()), rank, int(stitched.tree_latency[eligible[rank]]) if eligible else 0, culprit]
    return Attribution(link.astype(np.int32), self_time, path_time, top, selected, path_rows, groups, summary)


def write_attribution_npz(path, attribution, names, stitched):
    """The attribution as one .npz next to the one write_npz stores: its arrays, the group names, and the trees' roots
    and latencies so that the selection can be read without the stitched file."""
    a = attribution
    with open(path, "wb") as f:
        np.savez_compressed(
            f, link=a.link, self_time=a.self_time, path_time=a.path_time, tree_top_group=a.tree_top_group, tree_selected=a.tree_selected,
            tree_path_rows=a.tree_path_rows, groups=a.groups, group_columns=np.array(GROUP_COLUMNS), summary=a.summary,
            group_names=np.array([str(x) for x in names]), mean_latency=np.array([a.mean_latency(g) for g in range(a.groups.shape[1])]),
            tree_root=stitched.tree_root, tree_latency=stitched.tree_latency, tree_flags=stitched.tree_flags)


CALIB_COLUMNS = ("trees", "exact", "decisions")


class TraceConfidence(object):
    """rank / list_n / margin [requests of the batch]: the decision of every request (Engine.decisions); row_request [n_rows]:
    the request whose incoming span the row is, -1 none; per tree of the stitch tree_decisions / tree_not_best /
    tree_unassigned (counts), tree_min_margin (the smallest margin that is not NaN, +inf without one), tree_weakest_row (the
    incoming span of the request that attains it, the smallest row on ties, -1 without one) and tree_confident (decisions > 0,
    none of them not-best, min_margin >= threshold); calib [len(edges) + 2, 3] = CALIB_COLUMNS over the whole trees with a
    decision -- bucket 0: some decision is not the best of its list, bucket 1 + j: min_margin has passed j edges; the exact
    column is -1 without ground truth; summary = scored trees, confident trees, decisions, not-best, unassigned."""

    FIELDS = ("rank", "list_n", "margin", "row_request", "tree_decisions", "tree_not_best", "tree_unassigned", "tree_min_margin",
              "tree_weakest_row", "tree_confident", "calib", "summary")

    def __init__(self, rank, list_n, margin, row_request, tree_decisions, tree_not_best, tree_unassigned, tree_min_margin,
                 tree_weakest_row, tree_confident, calib, summary, threshold=0.0, edges=()):
        self.rank, self.list_n, self.margin, self.row_request = rank, list_n, margin, row_request
        self.tree_decisions, self.tree_not_best, self.tree_unassigned = tree_decisions, tree_not_best, tree_unassigned
        self.tree_min_margin, self.tree_weakest_row, self.tree_confident = tree_min_margin, tree_weakest_row, tree_confident
        self.calib = np.asarray(calib, dtype=np.int64)
        self.summary = np.asarray(summary, dtype=np.int64)
        self.threshold = float(threshold)
        self.edges = np.asarray(edges, dtype=np.float64)

    n_scored = property(lambda self: int(self.summary[0]))
    n_confident = property(lambda self: int(self.summary[1]))

    def same_as(self, other):
        """Bit for bit: the doubles are compared as the integers they are stored as, so that NaN and the infinities count."""
        bits = lambda a: np.asarray(a).view(np.int64) if np.asarray(a).dtype == np.float64 else np.asarray(a)
        return all(np.array_equal(bits(getattr(self, k)), bits(getattr(other, k))) for k in self.FIELDS)

    def table(self):
        """One dict per bucket of the calibration table: its range of min_margin, CALIB_COLUMNS and the share of exact trees."""
        lo = ["not best"] + [float("-inf")] + self.edges.tolist()
        hi = [None] + self.edges.tolist() + [float("inf")]
        return [dict([("bucket", b), ("from", lo[b]), ("to", hi[b])] + [(c, int(self.calib[b][i])) for i, c in enumerate(CALIB_COLUMNS)] +
                     [("exact_share", float(self.calib[b][1]) / int(self.calib[b][0]) if self.calib[b][0] > 0 and self.calib[b][1] >= 0 else float("nan"))])
                for b in range(len(self.calib))]


def margin_key(margin):
    """uint64 keys of binary64 values, ascending in the order -inf < ... < -0 < +0 < ... < +inf (conf_key of csrc/tw_conf.h)."""
    b = np.ascontiguousarray(margin, dtype=np.float64).view(np.uint64)
    return np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(1 << 63))


def decisions_host(result):
    """The per-request definition of include/traceweaver_amd.h on one unit's candidate lists: `result` holds chosen [n],
    topk_n [n] and topk_score [n, K] of the list the selection chose from (the layout of the oracle's run_pass: its topk_*,
    not topk2_*).  Returns {rank, list_n, margin}."""
    chosen = np.asarray(result["chosen"], dtype=np.int32)
    n = np.asarray(result["topk_n"], dtype=np.int32)
    s = np.asarray(result["topk_score"], dtype=np.float64)
    margin = np.full(len(chosen), np.nan, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for g, c in enumerate(chosen.tolist()):
            if c == 0:
                margin[g] = s[g, 0] - s[g, 1] if n[g] > 1 else np.inf
            elif c > 0:
                margin[g] = s[g, c] - s[g, 0]
    margin[np.isnan(margin)] = np.nan                             # one NaN: the sign of inf - inf differs between machines
    return {"rank": chosen.copy(), "list_n": n.copy(), "margin": margin}


def confidence_host(stitched, in_rows, rank, margin, threshold=0.0, edges=(), list_n=None):
    """What tw_score_traces computes from the decisions, restated from the definitions in plain numpy, for the tests.  in_rows,
    rank, margin: per request of the batch (flat, or one array per unit)."""
    flat = lambda a, dt: np.concatenate([np.asarray(x, dtype=dt).ravel() for x in a]) if isinstance(a, (list, tuple)) else np.asarray(a, dtype=dt)
    in_rows, rank, margin = flat(in_rows, np.int64), flat(rank, np.int32), flat(margin, np.float64)
    list_n = np.zeros(len(rank), dtype=np.int32) if list_n is None else flat(list_n, np.int32)
    edges = np.asarray(edges, dtype=np.float64).ravel()
    nt = stitched.n_trees
    row_request = np.full(len(stitched.root), -1, dtype=np.int32)
    row_request[in_rows] = np.arange(len(in_rows), dtype=np.int32)
    dec, nb, una = (np.zeros(nt, dtype=np.int32) for _ in range(3))
    min_margin = np.full(nt, np.inf, dtype=np.float64)
    weakest = np.full(nt, -1, dtype=np.int32)
    for k in range(nt):
        g = row_request[stitched.tree_rows[int(stitched.tree_off[k]):int(stitched.tree_off[k + 1])]]
        g = g[g >= 0]
        dec[k], nb[k], una[k] = len(g), int((rank[g] != 0).sum()), int((rank[g] < 0).sum())
        g = g[~np.isnan(margin[g])]
        if len(g):
            key = margin_key(margin[g])
            at = g[key == key.min()]
            min_margin[k] = margin[at[0]]
            weakest[k] = in_rows[at].min()
    confident = (dec > 0) & (nb == 0) & (min_margin >= threshold)
    flags = np.asarray(stitched.tree_flags).astype(np.int64)
    has_truth = int(stitched.counts[3]) >= 0
    calib = np.zeros((len(edges) + 2, 3), dtype=np.int64)
    for k in range(nt):
        if (flags[k] & WHOLE) and dec[k] > 0:
            b = 0 if nb[k] > 0 else 1 + int(sum(1 for x in edges if min_margin[k] >= x))
            calib[b, 0] += 1
            calib[b, 1] += 1 if flags[k] & EXACT else 0
            calib[b, 2] += dec[k]
    if not has_truth:
        calib[:, 1] = -1
    summary = [int((dec > 0).sum()), int(confident.sum()), int(dec.sum()), int(nb.sum()), int(una.sum())]
    return TraceConfidence(rank, list_n, margin, row_request, dec, nb, una, min_margin, weakest, confident.astype(np.uint8), calib, summary,
                           threshold, edges)


def write_confidence_npz(path, confidence, stitched):
    """The confidence of the stitched traces as one .npz next to the one write_npz stores: the arrays of TraceConfidence, the
    query (threshold, edges) and the trees' roots and flags, so that it can be read without the stitched file."""
    c = confidence
    with open(path, "wb") as f:
        np.savez_compressed(
            f, threshold=np.float64(c.threshold), edges=c.edges, calib_columns=np.array(CALIB_COLUMNS),
            tree_root=stitched.tree_root, tree_flags=stitched.tree_flags, **{k: getattr(c, k) for k in TraceConfidence.FIELDS})


METRICS = ("span_latency", "self_time", "path_time", "trace_latency")
EMPTY = np.iinfo(np.int64).min       # quantile of an empty segment


class LatencyDistributions(object):
    """The populations behind an attribution, per segment = (cohort c, metric m of METRICS, group g), index c * (3 G + 1) + m * G
    + g, the trace-latency segment (no group) last within a cohort: tree_cohort [n_trees] (the smallest label >= 0 among the
    tree's rows, -1 none: such a tree is counted nowhere); seg_count / seg_sum [n_seg]; values [n_items], of which segment s
    owns values[seg_off[s]:seg_off[s + 1]], ascending; quantile [n_seg, len(probs)] (the value at index min(n - 1, int(p * n)),
    EMPTY for an empty segment); hist [n_seg, len(edges) + 1] (bin of v = the number of edges <= v); summary = items, non-empty
    segments, selected trees counted, selected trees left out (include/traceweaver_amd.h has the definitions)."""

    FIELDS = ("tree_cohort", "seg_count", "seg_sum", "seg_off", "values", "quantile", "hist", "summary")

    def __init__(self, tree_cohort, seg_count, seg_sum, seg_off, values, quantile, hist, summary, n_cohorts, n_groups, probs=(), edges=()):
        self.tree_cohort, self.seg_count, self.seg_sum, self.seg_off, self.values = tree_cohort, seg_count, seg_sum, seg_off, values
        self.quantile, self.hist = quantile, hist
        self.summary = np.asarray(summary, dtype=np.int64)
        self.n_cohorts, self.n_groups = int(n_cohorts), int(n_groups)
        self.probs = np.asarray(probs, dtype=np.float64)
        self.edges = np.asarray(edges, dtype=np.int64)

    n_items = property(lambda self: int(self.summary[0]))
    n_seg = property(lambda self: self.n_cohorts * (3 * self.n_groups + 1))

    def index(self, cohort, metric, group=None):
        m = METRICS.index(metric) if isinstance(metric, str) else int(metric)
        if not (0 <= cohort < self.n_cohorts and 0 <= m < 4 and (m == 3 or 0 <= group < self.n_groups)):
            raise IndexError((cohort, metric, group))
        return cohort * (3 * self.n_groups + 1) + m * self.n_groups + (0 if m == 3 else int(group))

    def segment(self, cohort, metric, group=None):
        """The sorted values of one segment, a view of `values`."""
        s = self.index(cohort, metric, group)
        return self.values[int(self.seg_off[s]):int(self.seg_off[s + 1])]

    def cohort(self, c):
        """Cohort c alone, in the layout of a result with one cohort (compare_distributions(d.cohort(0), d.cohort(1)))."""
        per = 3 * self.n_groups + 1
        a, b = c * per, (c + 1) * per
        lo, hi = int(self.seg_off[a]), int(self.seg_off[b])
        count = self.seg_count[a:b]
        summary = [hi - lo, int((count > 0).sum()), int(count[-1]), int(self.summary[2] + self.summary[3] - count[-1])]
        return LatencyDistributions(np.where(self.tree_cohort == c, 0, -1).astype(np.int32), count, self.seg_sum[a:b], self.seg_off[a:b + 1] - lo,
                                    self.values[lo:hi], self.quantile[a:b], self.hist[a:b], summary, 1, self.n_groups, self.probs, self.edges)

    def table(self, names=None):
        """One dict per non-empty segment: cohort, metric, group (None for the trace latency), count, mean and the quantiles as
        p<percent>."""
        rows, per = [], 3 * self.n_groups + 1
        for s in np.flatnonzero(self.seg_count > 0).tolist():
            c, rest = divmod(s, per)
            m, g = (3, None) if rest == 3 * self.n_groups else divmod(rest, self.n_groups)
            rows.append(dict([("cohort", c), ("metric", METRICS[m]), ("group", g if names is None or g is None else names[g]),
                              ("count", int(self.seg_count[s])), ("mean", float(self.seg_sum[s]) / int(self.seg_count[s]))] +
                             [("p%g" % (100 * p), int(self.quantile[s][j])) for j, p in enumerate(self.probs.tolist())]))
        return rows

    def same_as(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.FIELDS)


def distributions_host(stitched, attribution, row_start, row_end, row_group, n_groups, row_cohort=None, n_cohorts=1,
                       probs=(0.5, 0.9, 0.95, 0.99), edges=None):
    """What tw_latency_distributions computes, restated from the definitions in plain Python and numpy, for the tests.  The
    attribution is the one the device call follows (its link, self_time, path_time and tree_selected are read)."""
    start = np.asarray(row_start, dtype=np.int64)
    end = np.maximum(np.asarray(row_end, dtype=np.int64), start)
    group = np.asarray(row_group, dtype=np.int64)
    n, nt, G = len(start), stitched.n_trees, int(n_groups)
    children = [[] for _ in range(n)]
    for c, p in enumerate(np.asarray(attribution.link).tolist()):
        if p >= 0:
            children[p].append(c)
    _, walked = critical_paths_host(children, start.tolist(), end.tolist(), stitched.tree_root)
    tree_cohort = np.zeros(nt, dtype=np.int32)
    if row_cohort is not None:
        label = np.asarray(row_cohort, dtype=np.int64)
        for k in range(nt):
            x = label[stitched.tree_rows[int(stitched.tree_off[k]):int(stitched.tree_off[k + 1])]]
            tree_cohort[k] = x[x >= 0].min() if (x >= 0).any() else -1
    else:
        n_cohorts = 1
    per = 3 * G + 1
    items = [[] for _ in range(n_cohorts * per)]
    counted = left = 0
    for k in np.flatnonzero(np.asarray(attribution.tree_selected)).tolist():
        c = int(tree_cohort[k])
        if c < 0:
            left += 1
            continue
        counted += 1
        for r in stitched.tree_rows[int(stitched.tree_off[k]):int(stitched.tree_off[k + 1])].tolist():
            g = int(group[r])
            if g < 0:
                continue
            items[c * per + g].append(int(end[r] - start[r]))
            items[c * per + G + g].append(int(attribution.self_time[r]))
            if walked[r]:
                items[c * per + 2 * G + g].append(int(attribution.path_time[r]))
        items[c * per + 3 * G].append(int(stitched.tree_latency[k]))
    probs = np.asarray(probs, dtype=np.float64).ravel()
    edges = np.asarray(() if edges is None else edges, dtype=np.int64).ravel()
    n_seg = len(items)
    seg_count = np.array([len(x) for x in items], dtype=np.int64)
    seg_sum = np.array([sum(x) for x in items], dtype=np.int64)
    seg_off = np.concatenate([[0], np.cumsum(seg_count)]).astype(np.int64)
    values = np.array([v for x in items for v in sorted(x)], dtype=np.int64)
    quantile = np.full((n_seg, len(probs)), EMPTY, dtype=np.int64)
    hist = np.zeros((n_seg, len(edges) + 1), dtype=np.int64)
    for s, x in enumerate(items):
        x = sorted(x)
        for j, p in enumerate(probs.tolist()):
            if x:
                quantile[s, j] = x[min(len(x) - 1, int(p * float(len(x))))]
        for v in x:
            hist[s, sum(1 for edge in edges.tolist() if v >= edge)] += 1
    summary = [len(values), int((seg_count > 0).sum()), counted, left]
    return LatencyDistributions(tree_cohort, seg_count, seg_sum, seg_off, values, quantile, hist, summary, n_cohorts, G, probs, edges)


def compare_distributions(a, b):
    """Two results with the same segment layout side by side, per segment: quantile_diff [n_seg, n_q] = b's quantile less a's (0
    where either segment is empty), both [n_seg] = neither is empty, and cdf_gap [n_seg] = the largest |F_a(x) - F_b(x)| over the
    union of both value sets, F(x) = the share of values <= x (nan where either is empty).  On the host, in numpy: it compares any
    two results, predicted against true among them, which are two different resident states.  Cohort against cohort of one result
    is compared on the device, with a permutation test: Engine.compare_cohorts (tw_compare_cohorts)."""
    if (a.n_cohorts, a.n_groups) != (b.n_cohorts, b.n_groups) or not np.array_equal(a.probs, b.probs):
        raise ValueError("the two results differ in their segments or probs")
    both = (np.asarray(a.seg_count) > 0) & (np.asarray(b.seg_count) > 0)
    diff = np.where(both[:, None], np.asarray(b.quantile) - np.where(both[:, None], a.quantile, 0), 0).astype(np.int64)
    gap = np.full(a.n_seg, np.nan, dtype=np.float64)
    for s in np.flatnonzero(both).tolist():
        x = a.values[int(a.seg_off[s]):int(a.seg_off[s + 1])]
        y = b.values[int(b.seg_off[s]):int(b.seg_off[s + 1])]
        at = np.union1d(x, y)
        gap[s] = np.abs(np.searchsorted(x, at, side="right") / float(len(x)) - np.searchsorted(y, at, side="right") / float(len(y))).max()
    return {"quantile_diff": diff, "both": both, "cdf_gap": gap}


def write_distributions_npz(path, distributions, names):
    """The distributions as one .npz next to the one write_attribution_npz stores: the arrays of LatencyDistributions, the
    layout (n_cohorts, n_groups, metrics, group names) and the query (probs, edges)."""
    d = distributions
    with open(path, "wb") as f:
        np.savez_compressed(
            f, n_cohorts=np.int64(d.n_cohorts), n_groups=np.int64(d.n_groups), metrics=np.array(METRICS), group_names=np.array([str(x) for x in names]),
            probs=d.probs, edges=d.edges, **{k: getattr(d, k) for k in LatencyDistributions.FIELDS})


def history_host(parts, probs=(), edges=None):
    """What the history holds after Engine.history_push / history_merge of `parts`, in turn, on an empty history
    (tw_history_push, tw_history_distributions), restated with numpy and Python integers, for the tests.  parts: a list of
    (LatencyDistributions, cohort_map); cohort_map [n_cohorts of the part] names the history cohort a cohort of the part goes to,
    -1 = not kept, None = the identity.  Returns a LatencyDistributions of C_h = 1 + the largest entry cohorts: every segment
    the sorted concatenation of what was pushed into it; tree_cohort is empty; summary = items, non-empty segments, C_h, parts."""
    if not parts:
        raise ValueError("history_host: no parts")
    G = parts[0][0].n_groups
    per = 3 * G + 1
    maps = []
    for d, cohort_map in parts:
        m = list(range(d.n_cohorts)) if cohort_map is None else [int(x) for x in cohort_map]
        kept = [h for h in m if h >= 0]
        if d.n_groups != G or len(m) != d.n_cohorts or min(m + [0]) < -1 or len(set(kept)) != len(kept):
            raise ValueError("history_host: a part does not fit (groups, the length of its map, an entry below -1 or a repeated one)")
        maps.append(m)
    C = max([0] + [1 + h for m in maps for h in m])
    items = [[] for _ in range(C * per)]
    for (d, _), m in zip(parts, maps):
        for c, h in enumerate(m):
            if h >= 0:
                for r in range(per):
                    s = c * per + r
                    items[h * per + r].extend(int(v) for v in d.values[int(d.seg_off[s]):int(d.seg_off[s + 1])])
    probs = np.asarray(probs, dtype=np.float64).ravel()
    edges = np.asarray(() if edges is None else edges, dtype=np.int64).ravel()
    n_seg = len(items)
    items = [sorted(x) for x in items]
    seg_count = np.array([len(x) for x in items], dtype=np.int64)
    seg_sum = np.array([((sum(x) + (1 << 63)) % (1 << 64)) - (1 << 63) for x in items], dtype=np.int64)     # two's complement, wrapping
    seg_off = np.concatenate([[0], np.cumsum(seg_count)]).astype(np.int64)
    values = np.array([v for x in items for v in x], dtype=np.int64)
    quantile = np.full((n_seg, len(probs)), EMPTY, dtype=np.int64)
    hist = np.zeros((n_seg, len(edges) + 1), dtype=np.int64)
    for s, x in enumerate(items):
        for j, p in enumerate(probs.tolist()):
            if x:
                quantile[s, j] = x[min(len(x) - 1, int(p * float(len(x))))]
        if x:
            hist[s] = np.bincount(np.searchsorted(edges, np.array(x, dtype=np.int64), side="right"), minlength=len(edges) + 1)
    summary = [len(values), int((seg_count > 0).sum()), C, len(parts)]
    return LatencyDistributions(np.zeros(0, dtype=np.int32), seg_count, seg_sum, seg_off, values, quantile, hist, summary, C, G, probs, edges)


def write_history_npz(path, history, group_names, cohort_names=None):
    """A history read back (Engine.history_distributions) as one .npz: seg_off, values, C_h, G and the names of the groups and
    of the cohorts (default: their numbers).  read_history_npz gives what Engine.history_merge takes."""
    h = history
    cohorts = [str(c) for c in range(h.n_cohorts)] if cohort_names is None else [str(x) for x in cohort_names]
    if len(cohorts) != h.n_cohorts or len(group_names) != h.n_groups:
        raise ValueError("write_history_npz: the names do not match the history's cohorts and groups")
    with open(path, "wb") as f:
        np.savez_compressed(f, C_h=np.int64(h.n_cohorts), G=np.int64(h.n_groups), seg_off=np.asarray(h.seg_off, dtype=np.int64),
                            values=np.asarray(h.values, dtype=np.int64), group_names=np.array([str(x) for x in group_names]),
                            cohort_names=np.array(cohorts))


def read_history_npz(path):
    """-> ((n_cohorts, n_groups, seg_off, values), group_names, cohort_names): the first is an argument of Engine.history_merge."""
    with np.load(path) as z:
        C, G = int(z["C_h"]), int(z["G"])
        seg_off, values = z["seg_off"].astype(np.int64), z["values"].astype(np.int64)
        group_names, cohort_names = [str(x) for x in z["group_names"].tolist()], [str(x) for x in z["cohort_names"].tolist()]
    if len(seg_off) != C * (3 * G + 1) + 1 or len(values) != int(seg_off[-1]) or len(group_names) != G or len(cohort_names) != C:
        raise ValueError("%s: not a history (the arrays do not match C_h and G)" % path)
    return (C, G, seg_off, values), group_names, cohort_names


class CohortComparison(object):
    """Pairs of cohorts compared segment by segment (include/traceweaver_amd.h has the definitions): row = pair * (3 G + 1) + m * G +
    g compares A = segment (a, m, g) with B = segment (b, m, g) of pairs[pair] = (a, b).  n_a, n_b [n_rows]; ks_gap = #{A <= x} n_b
    - #{B <= x} n_a at ks_at, the smallest x where its magnitude is greatest; u2 = 2 #{A_i < B_j} + #{A_i = B_j}; quantile_shift
    [n_rows, len(probs)] = Q_B - Q_A; perm_ge_ks, perm_ge_u, perm_ge_q: of n_perm permutations of the pooled values those at least
    as extreme as the observed statistic, -1 where the row was not permuted (a side empty, more than max_pool values, n_perm = 0);
    summary = rows with both sides non-empty, rows permuted, pooled items permuted, n_perm."""

    FIELDS = ("n_a", "n_b", "ks_gap", "ks_at", "u2", "quantile_shift", "perm_ge_ks", "perm_ge_u", "perm_ge_q", "summary")

    def __init__(self, n_a, n_b, ks_gap, ks_at, u2, quantile_shift, perm_ge_ks, perm_ge_u, perm_ge_q, summary, pairs, probs, n_groups, n_perm):
        self.n_a, self.n_b, self.ks_gap, self.ks_at, self.u2, self.quantile_shift = n_a, n_b, ks_gap, ks_at, u2, quantile_shift
        self.perm_ge_ks, self.perm_ge_u, self.perm_ge_q = perm_ge_ks, perm_ge_u, perm_ge_q
        self.summary = np.asarray(summary, dtype=np.int64)
        self.pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        self.probs = np.asarray(probs, dtype=np.float64)
        self.n_groups, self.n_perm = int(n_groups), int(n_perm)

    n_rows = property(lambda self: len(self.pairs) * (3 * self.n_groups + 1))

    def row(self, pair_index, metric, group=None):
        m = METRICS.index(metric) if isinstance(metric, str) else int(metric)
        if not (0 <= pair_index < len(self.pairs) and 0 <= m < 4 and (m == 3 or 0 <= group < self.n_groups)):
            raise IndexError((pair_index, metric, group))
        return pair_index * (3 * self.n_groups + 1) + m * self.n_groups + (0 if m == 3 else int(group))

    def _both(self):
        return (np.asarray(self.n_a) > 0) & (np.asarray(self.n_b) > 0)

    def _over_pairs(self, x):
        both = self._both()
        prod = np.where(both, np.asarray(self.n_a, dtype=np.float64) * np.asarray(self.n_b, dtype=np.float64), 1.0)
        return np.where(both, np.asarray(x, dtype=np.float64) / prod, np.nan)

    def ks(self):
        """The two-sample KS statistic |ks_gap| / (n_a n_b) per row, nan where a side is empty."""
        return self._over_pairs(np.abs(np.asarray(self.ks_gap, dtype=np.float64)))

    def superiority(self):
        """u2 / (2 n_a n_b) per row: the probability that a value of B exceeds one of A, ties counted half; nan where a side is empty."""
        return self._over_pairs(np.asarray(self.u2, dtype=np.float64) / 2.0)

    def p_value(self, which):
        """(1 + ge) / (1 + n_perm) per row for "ks", "u" or the index of a prob; nan where the row was not permuted."""
        ge = self.perm_ge_ks if which == "ks" else self.perm_ge_u if which == "u" else np.asarray(self.perm_ge_q)[:, int(which)]
        ge = np.asarray(ge, dtype=np.float64)
        return np.where(ge >= 0, (1.0 + ge) / (1.0 + self.n_perm), np.nan)

    def table(self, names=None):
        """One dict per row with both sides non-empty: pair, metric, group (None for the trace latency), the sizes, ks, ks_at,
        superiority, the shifts as shift_p<percent> and, where permuted, p_ks, p_u and p_shift_p<percent>."""
        rows, per = [], 3 * self.n_groups + 1
        ks, sup = self.ks(), self.superiority()
        pv = {"ks": self.p_value("ks"), "u": self.p_value("u")}
        pq = [self.p_value(j) for j in range(len(self.probs))]
        for i in np.flatnonzero(self._both()).tolist():
            pi, rest = divmod(i, per)
            m, g = (3, None) if rest == 3 * self.n_groups else divmod(rest, self.n_groups)
            d = dict([("pair", tuple(self.pairs[pi].tolist())), ("metric", METRICS[m]), ("group", g if names is None or g is None else names[g]),
                      ("n_a", int(self.n_a[i])), ("n_b", int(self.n_b[i])), ("ks", float(ks[i])), ("ks_at", int(self.ks_at[i])),
                      ("superiority", float(sup[i]))] +
                     [("shift_p%g" % (100 * p), int(self.quantile_shift[i][j])) for j, p in enumerate(self.probs.tolist())])
            if self.perm_ge_ks[i] >= 0:
                d.update([("p_ks", float(pv["ks"][i])), ("p_u", float(pv["u"][i]))] +
                         [("p_shift_p%g" % (100 * p), float(pq[j][i])) for j, p in enumerate(self.probs.tolist())])
            rows.append(d)
        return rows

    def same_as(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.FIELDS)


_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15


def _mix64(x):
    """splitmix64's finaliser."""
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def permutation_labels_host(N, n_a, seed, row, p):
    """Permutation p of row `row`: a list of N labels, 0 = the pooled value at that position goes to A', 1 = to B'; exactly n_a
    zeros.  Selection sampling along the pooled values: item k goes to A' iff (h_k * (N - k)) >> 64 < n_a - (given so far)."""
    key = _mix64((_mix64((seed + _GOLD * (row + 1)) & _M64) + _GOLD * (p + 1)) & _M64)
    labels, c = [], 0
    for k in range(N):
        h = _mix64((key + _GOLD * (k + 1)) & _M64)
        if (h * (N - k)) >> 64 < n_a - c:
            labels.append(0)
            c += 1
        else:
            labels.append(1)
    return labels


def two_sample_host(A, B, probs):
    """ks_gap, ks_at, u2 and the quantile shifts of two non-empty ascending lists of integers, from the definitions."""
    import bisect

    na, nb = len(A), len(B)
    gap, at = 0, None
    for x in sorted(set(A) | set(B)):
        g = bisect.bisect_right(A, x) * nb - bisect.bisect_right(B, x) * na
        if at is None or abs(g) > abs(gap):
            gap, at = g, x
    u2 = 0
    for v in A:
        hi = bisect.bisect_right(B, v)
        u2 += 2 * (nb - hi) + (hi - bisect.bisect_left(B, v))
    shifts = [B[min(nb - 1, int(p * float(nb)))] - A[min(na - 1, int(p * float(na)))] for p in probs]
    return gap, at, u2, shifts


def compare_cohorts_host(distributions, pairs=((0, 1),), probs=(0.5, 0.95, 0.99), permutations=0, seed=0, max_pool=0):
    """What tw_compare_cohorts computes, restated from the definitions in plain Python integers, from a LatencyDistributions (with
    its values) alone, for the tests."""
    d = distributions
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    probs = [float(p) for p in np.asarray(probs, dtype=np.float64).ravel().tolist()]
    per, nq, n_perm = 3 * d.n_groups + 1, len(probs), int(permutations)
    n_rows = len(pairs) * per
    out = {k: np.zeros(n_rows, dtype=np.int64) for k in ("n_a", "n_b", "ks_gap", "u2")}
    out["ks_at"] = np.full(n_rows, EMPTY, dtype=np.int64)
    out["quantile_shift"] = np.zeros((n_rows, nq), dtype=np.int64)
    out["perm_ge_ks"], out["perm_ge_u"] = np.full(n_rows, -1, dtype=np.int64), np.full(n_rows, -1, dtype=np.int64)
    out["perm_ge_q"] = np.full((n_rows, nq), -1, dtype=np.int64)
    both = permuted = items = 0
    for row in range(n_rows):
        pi, r = divmod(row, per)
        sa, sb = int(pairs[pi][0]) * per + r, int(pairs[pi][1]) * per + r
        A = d.values[int(d.seg_off[sa]):int(d.seg_off[sa + 1])].tolist()
        B = d.values[int(d.seg_off[sb]):int(d.seg_off[sb + 1])].tolist()
        na, nb = len(A), len(B)
        out["n_a"][row], out["n_b"][row] = na, nb
        if na == 0 or nb == 0:
            continue
        both += 1
        gap, at, u2, shifts = two_sample_host(A, B, probs)
        out["ks_gap"][row], out["ks_at"][row], out["u2"][row] = gap, at, u2
        out["quantile_shift"][row] = shifts
        N = na + nb
        if n_perm == 0 or (max_pool > 0 and N > max_pool):
            continue
        permuted += 1
        items += N
        M = sorted(A + B)
        ge_ks = ge_u = 0
        ge_q = [0] * nq
        for p in range(n_perm):
            labels = permutation_labels_host(N, na, int(seed), row, p)
            A2 = [v for v, l in zip(M, labels) if l == 0]
            B2 = [v for v, l in zip(M, labels) if l == 1]
            g2, _, u, s2 = two_sample_host(A2, B2, probs)
            ge_ks += abs(g2) >= abs(gap)
            ge_u += abs(u - na * nb) >= abs(u2 - na * nb)
            for j in range(nq):
                ge_q[j] += abs(s2[j]) >= abs(shifts[j])
        out["perm_ge_ks"][row], out["perm_ge_u"][row] = ge_ks, ge_u
        out["perm_ge_q"][row] = ge_q
    return CohortComparison(summary=[both, permuted, items, n_perm], pairs=pairs, probs=probs, n_groups=d.n_groups, n_perm=n_perm, **out)


def write_comparison_npz(path, comparison, names):
    """The comparison as one .npz next to the one write_distributions_npz stores: the arrays of CohortComparison, the layout (pairs,
    n_groups, metrics, group names) and the query (probs, n_perm)."""
    c = comparison
    with open(path, "wb") as f:
        np.savez_compressed(
            f, pairs=c.pairs, n_groups=np.int64(c.n_groups), metrics=np.array(METRICS), group_names=np.array([str(x) for x in names]),
            probs=c.probs, n_perm=np.int64(c.n_perm), **{k: getattr(c, k) for k in CohortComparison.FIELDS})


SIGNATURE_MODES = ("levels", "edges")
NOT_COMPARED = 255                   # tree_same of a tree that is not eligible or whose root row the reference set does not hold


class TraceSignatures(object):
    """The trees of a stitch grouped by call-graph signature (include/traceweaver_amd.h has the definitions): row_level [n_rows]
    (server rows: the server rows above them, -1 otherwise); tree_class (-1 not eligible), tree_items, tree_same (1 / 0 against
    the reference set, NOT_COMPARED otherwise) [n_trees]; per class, numbered by their first tree, class_rep, class_trees,
    class_latency_sum / _min / _max; class c owns class_entries[class_off[c]:class_off[c + 1]], rows (level, caller group, group,
    count) -- the caller group is 0 in mode "levels"; summary = eligible trees, classes, items, entries, compared trees, same
    trees (the last two -1 without a comparison).  tree_root (not compared by same_as) names the trees' root rows."""

    FIELDS = ("row_level", "tree_class", "tree_items", "tree_same", "class_rep", "class_trees", "class_latency_sum", "class_latency_min",
              "class_latency_max", "class_off", "class_entries", "summary")

    def __init__(self, row_level, tree_class, tree_items, tree_same, class_rep, class_trees, class_latency_sum, class_latency_min,
                 class_latency_max, class_off, class_entries, summary, mode=0, tree_root=None):
        self.row_level, self.tree_class, self.tree_items, self.tree_same = row_level, tree_class, tree_items, tree_same
        self.class_rep, self.class_trees, self.class_latency_sum = class_rep, class_trees, class_latency_sum
        self.class_latency_min, self.class_latency_max, self.class_off = class_latency_min, class_latency_max, class_off
        self.class_entries = np.asarray(class_entries, dtype=np.int32).reshape(-1, 4)
        self.summary = np.asarray(summary, dtype=np.int64)
        self.mode = int(mode)
        self.tree_root = None if tree_root is None else np.asarray(tree_root, dtype=np.int32)

    n_classes = property(lambda self: len(self.class_rep))
    n_eligible = property(lambda self: int(self.summary[0]))

    def entries(self, c):
        """The signature of class c: an [n, 4] view of class_entries."""
        c = int(c)
        if not 0 <= c < self.n_classes:
            raise IndexError(c)
        return self.class_entries[int(self.class_off[c]):int(self.class_off[c + 1])]

    def signature(self, c):
        """... as a tuple of (level, caller group, group, count) tuples."""
        return tuple(tuple(int(x) for x in row) for row in self.entries(c))

    def by_root(self):
        """{root row: signature} of the eligible trees: what keep_reference stores, the `reference` of signatures_host."""
        sigs = [self.signature(c) for c in range(self.n_classes)]
        return {int(r): sigs[int(c)] for r, c in zip(self.tree_root.tolist(), self.tree_class.tolist()) if c >= 0}

    def table(self, names=None):
        """One dict per class, sorted by class_trees descending (ties: the class number): class, rep, trees, share of the eligible
        trees, mean / min / max latency, and the signature as a list of (level, caller, group, count) with the groups' names."""
        name = lambda g: g if names is None or g < 0 else names[g]
        rows = []
        for c in sorted(range(self.n_classes), key=lambda c: (-int(self.class_trees[c]), c)):
            n = int(self.class_trees[c])
            sig = [(lv, name(cg) if self.mode == 1 else None, name(g), k) for lv, cg, g, k in self.signature(c)]
            rows.append({"class": c, "rep": int(self.class_rep[c]), "trees": n, "share": float(n) / max(self.n_eligible, 1),
                         "mean_latency": float(self.class_latency_sum[c]) / n, "min_latency": int(self.class_latency_min[c]),
                         "max_latency": int(self.class_latency_max[c]), "signature": sig})
        return rows

    def same_as(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.FIELDS)


def signatures_host(stitched, link, row_kind, row_group, n_groups, mode=0, need_flags=WHOLE, skip_flags=0, reference=None):
    """What tw_trace_signatures computes, restated from the definitions in plain Python: ancestors walked one by one, signatures
    as tuples in a dictionary, no hash of our own.  link: the stitched links (Attribution.link, or test code's own); reference:
    {root row: signature} (TraceSignatures.by_root of the call that kept the reference set) for tree_same."""
    mode = SIGNATURE_MODES.index(mode) if isinstance(mode, str) else int(mode)
    link = [int(x) for x in link]
    kind = [int(x) for x in row_kind]
    group = [int(x) for x in row_group]
    n, nt = len(link), stitched.n_trees
    assert all(-1 <= g < n_groups for g in group)
    level = np.full(n, -1, dtype=np.int32)
    caller = [-1] * n
    for r in range(n):
        if kind[r] != 1:
            continue
        above, p = [], link[r]
        while p >= 0:
            if kind[p] == 1:
                above.append(p)
            p = link[p]
        level[r] = len(above)
        caller[r] = group[above[0]] if above else -1
    flags = np.asarray(stitched.tree_flags).astype(np.int64)
    tree_class = np.full(nt, -1, dtype=np.int32)
    tree_items = np.zeros(nt, dtype=np.int64)
    tree_same = np.full(nt, NOT_COMPARED, dtype=np.uint8)
    classes, sigs, members = {}, [], []
    for t in range(nt):
        rows = stitched.tree_rows[int(stitched.tree_off[t]):int(stitched.tree_off[t + 1])].tolist()
        items = sorted((int(level[r]), caller[r] if mode == 1 else 0, group[r]) for r in rows if kind[r] == 1 and group[r] >= 0)
        tree_items[t] = len(items)
        if not ((flags[t] & need_flags) == need_flags and (flags[t] & skip_flags) == 0):
            continue
        sig = []
        for it in items:
            if sig and sig[-1][0] == it:
                sig[-1][1] += 1
            else:
                sig.append([it, 1])
        sig = tuple(it + (k,) for it, k in sig)
        if sig not in classes:                                    # trees ascend: the first tree of a class is its rep
            classes[sig] = len(sigs)
            sigs.append(sig)
            members.append([])
        tree_class[t] = classes[sig]
        members[classes[sig]].append(t)
        if reference is not None and int(stitched.tree_root[t]) in reference:
            tree_same[t] = 1 if reference[int(stitched.tree_root[t])] == sig else 0
    lat = np.asarray(stitched.tree_latency, dtype=np.int64)
    class_off = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    entries = np.array([e for s in sigs for e in s], dtype=np.int32).reshape(-1, 4)
    eligible = tree_class >= 0
    compared = [int((tree_same != NOT_COMPARED).sum()), int((tree_same == 1).sum())] if reference is not None else [-1, -1]
    summary = [int(eligible.sum()), len(sigs), int(tree_items[eligible].sum()), len(entries)] + compared
    return TraceSignatures(level, tree_class, tree_items, tree_same, np.array([m[0] for m in members], dtype=np.int32),
                           np.array([len(m) for m in members], dtype=np.int64), np.array([lat[m].sum() for m in members], dtype=np.int64),
                           np.array([lat[m].min() for m in members], dtype=np.int64), np.array([lat[m].max() for m in members], dtype=np.int64),
                           class_off, entries, summary, mode, stitched.tree_root)


def compare_signatures(pred, true):
    """The host-side cross-check of tree_same: the eligible trees of `pred` matched with those of `true` by root row, their entry
    lists compared.  Returns {"tree_same" [trees of pred] as the device writes it, "compared", "same", "share" = same / compared
    (nan without a compared tree): the share of the matched traces that have the true signature}."""
    if pred.mode != true.mode:
        raise ValueError("the two results were computed in different modes")
    ref = true.by_root()
    sigs = [pred.signature(c) for c in range(pred.n_classes)]
    same = np.full(len(pred.tree_class), NOT_COMPARED, dtype=np.uint8)
    for t, (r, c) in enumerate(zip(pred.tree_root.tolist(), pred.tree_class.tolist())):
        if c >= 0 and r in ref:
            same[t] = 1 if ref[r] == sigs[c] else 0
    compared, ok = int((same != NOT_COMPARED).sum()), int((same == 1).sum())
    return {"tree_same": same, "compared": compared, "same": ok, "share": float(ok) / compared if compared else float("nan")}


def write_signatures_npz(path, names, pred, true=None):
    """The signatures as one .npz: the arrays of TraceSignatures of the predicted forest (and, prefixed true_, of the true one),
    the trees' root rows, the mode, the group names, and with both sides shape_accuracy = the share of the compared traces whose
    signature is the true one."""
    out = {"mode": np.array(SIGNATURE_MODES[pred.mode]), "group_names": np.array([str(x) for x in names]), "tree_root": pred.tree_root}
    out.update({k: getattr(pred, k) for k in TraceSignatures.FIELDS})
    if true is not None:
        out.update({"true_" + k: getattr(true, k) for k in TraceSignatures.FIELDS})
        out["true_tree_root"] = true.tree_root
        compared, same = int(pred.summary[4]), int(pred.summary[5])
        out["shape_accuracy"] = np.float64(float(same) / compared if compared > 0 else float("nan"))
    with open(path, "wb") as f:
        np.savez_compressed(f, **out)


PROFILE_TABLE_CELLS = 512            # TW_PROF_TABLE_CELLS of csrc/tw_prof.h: entries a workgroup of the sweep keeps in LDS; beyond it, global cells
PROFILE_ENTRY_FIELDS = ("rows", "span_time", "span_min", "span_max", "self_time", "path_time", "path_rows", "path_trees", "offset")
PROFILE_CLASS_FIELDS = ("class_counted", "class_latency", "class_path_time", "class_top_entry")


class ClassProfiles(object):
    """The aggregate trace of every call-graph class (include/traceweaver_amd.h has the definitions), over the counted trees = the
    trees with a class that the attribution selected.  Per entry of the signatures' class_entries (int64 [n_entries]): rows,
    span_time, span_min / span_max (INT64_MAX / INT64_MIN without a row), self_time, path_time, path_rows (rows on the critical
    path), path_trees (counted trees with such a row at the entry), offset (sum of the rows' starts less their tree's).  Per class
    (int64 [n_classes]): class_counted, class_latency, class_path_time, class_top_entry (the global index of the entry with the
    largest path_time among those with a row on the path, -1 none).  summary = counted trees, classes with one, counted item rows,
    entries with a row, classed trees that are not selected, selected trees without a class.  class_off / class_entries / mode
    (not compared by same_as) are those of the signature result the profile belongs to."""

    FIELDS = PROFILE_ENTRY_FIELDS + PROFILE_CLASS_FIELDS + ("summary",)

    def __init__(self, rows, span_time, span_min, span_max, self_time, path_time, path_rows, path_trees, offset, class_counted, class_latency,
                 class_path_time, class_top_entry, summary, class_off=None, class_entries=None, mode=0):
        self.rows, self.span_time, self.span_min, self.span_max, self.self_time = rows, span_time, span_min, span_max, self_time
        self.path_time, self.path_rows, self.path_trees, self.offset = path_time, path_rows, path_trees, offset
        self.class_counted, self.class_latency, self.class_path_time, self.class_top_entry = class_counted, class_latency, class_path_time, class_top_entry
        self.summary = np.asarray(summary, dtype=np.int64)
        self.class_off = np.zeros(len(class_counted) + 1, dtype=np.int64) if class_off is None else np.asarray(class_off, dtype=np.int64)
        self.class_entries = np.asarray(() if class_entries is None else class_entries, dtype=np.int32).reshape(-1, 4)
        self.mode = int(mode)

    n_entries = property(lambda self: len(self.rows))
    n_classes = property(lambda self: len(self.class_counted))
    n_counted = property(lambda self: int(self.summary[0]))

    def entry(self, i):
        """Entry i (global index): its class, (level, caller group, group, count) and PROFILE_ENTRY_FIELDS, as a dict."""
        i = int(i)
        if not 0 <= i < self.n_entries:
            raise IndexError(i)
        lv, cg, g, k = (int(x) for x in self.class_entries[i])
        out = {"entry": i, "class": int(np.searchsorted(self.class_off, i, side="right")) - 1, "level": lv, "caller": cg, "group": g, "count": k}
        out.update({f: int(getattr(self, f)[i]) for f in PROFILE_ENTRY_FIELDS})
        return out

    def profile(self, c):
        """The aggregate trace of class c: its entries in signature order, each as entry() gives it."""
        c = int(c)
        if not 0 <= c < self.n_classes:
            raise IndexError(c)
        return [self.entry(i) for i in range(int(self.class_off[c]), int(self.class_off[c + 1]))]

    def table(self, names=None):
        """One dict per class with a counted tree, sorted by class_counted descending (ties: the class number): class, counted,
        mean_latency, path_time, top_entry (global index, -1 none), top = (level, caller, service) of that entry with the groups'
        names (the caller None in mode "levels"), top_share = its share of the class' path time, top_trees = path_trees /
        class_counted of it: in how many of the class' counted traces the entry is on the critical path."""
        name = lambda g: g if names is None or g < 0 else names[g]
        rows = []
        for c in sorted(np.flatnonzero(np.asarray(self.class_counted) > 0).tolist(), key=lambda c: (-int(self.class_counted[c]), c)):
            n, i, total = int(self.class_counted[c]), int(self.class_top_entry[c]), int(self.class_path_time[c])
            row = {"class": c, "counted": n, "mean_latency": float(self.class_latency[c]) / n, "path_time": total, "top_entry": i, "top": None,
                   "top_share": 0.0, "top_trees": 0.0}
            if i >= 0:
                lv, cg, g, _ = (int(x) for x in self.class_entries[i])
                row.update({"top": (lv, name(cg) if self.mode == 1 else None, name(g)), "top_share": float(self.path_time[i]) / total if total else 0.0,
                            "top_trees": float(self.path_trees[i]) / n})
            rows.append(row)
        return rows

    def same_as(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.FIELDS)


def class_profiles_host(stitched, signatures, attribution, link, row_kind, row_start, row_end, row_group):
    """What tw_class_profiles computes, restated from the definitions with dictionaries, for the tests.  signatures, attribution: the
    host results of signatures_host and attribute_host on the same forest and groups (tree_class, row_level, the entries and the
    mode of the first; tree_selected, self_time and path_time of the second); nothing the device computed is read."""
    link = [int(x) for x in link]
    kind = [int(x) for x in row_kind]
    group = [int(x) for x in row_group]
    start = [int(x) for x in row_start]
    end = [max(int(e), s) for e, s in zip(row_end, start)]
    children = [[] for _ in link]
    for c, p in enumerate(link):
        if p >= 0:
            children[p].append(c)
    _, walked = critical_paths_host(children, start, end, stitched.tree_root)   # the rows attribute_host counts in group_path_rows
    sig, mode = signatures, signatures.mode
    ne, nc = len(sig.class_entries), sig.n_classes
    index = {}
    for c in range(nc):
        for j, (lv, cg, g, _) in enumerate(sig.signature(c)):
            index[(c, lv, cg, g)] = int(sig.class_off[c]) + j
    cells = {f: {} for f in PROFILE_ENTRY_FIELDS}
    counted, latency = {}, {}
    add = lambda f, i, v: cells[f].__setitem__(i, cells[f].get(i, 0) + v)
    idle = loose = n_rows = 0
    for t in range(stitched.n_trees):
        c, sel = int(sig.tree_class[t]), int(attribution.tree_selected[t]) != 0
        idle += 1 if c >= 0 and not sel else 0
        loose += 1 if c < 0 and sel else 0
        if c < 0 or not sel:
            continue
        counted[c] = counted.get(c, 0) + 1
        latency[c] = latency.get(c, 0) + int(stitched.tree_latency[t])
        root, on_path = int(stitched.tree_root[t]), set()
        for r in stitched.tree_rows[int(stitched.tree_off[t]):int(stitched.tree_off[t + 1])].tolist():
            if kind[r] != 1 or group[r] < 0:
                continue
            cg = 0
            if mode == 1:
                p = link[r]
                while p >= 0 and kind[p] != 1:
                    p = link[p]
                cg = group[p] if p >= 0 else -1
            i = index[(c, int(sig.row_level[r]), cg, group[r])]
            d = end[r] - start[r]
            n_rows += 1
            add("rows", i, 1)
            add("span_time", i, d)
            cells["span_min"][i] = min(cells["span_min"].get(i, d), d)
            cells["span_max"][i] = max(cells["span_max"].get(i, d), d)
            add("self_time", i, int(attribution.self_time[r]))
            add("offset", i, start[r] - start[root])
            if walked[r]:
                add("path_time", i, int(attribution.path_time[r]))
                add("path_rows", i, 1)
                on_path.add(i)
        for i in on_path:
            add("path_trees", i, 1)
    empty = {"span_min": np.iinfo(np.int64).max, "span_max": np.iinfo(np.int64).min}
    arrays = [np.array([cells[f].get(i, empty.get(f, 0)) for i in range(ne)], dtype=np.int64) for f in PROFILE_ENTRY_FIELDS]
    rows, path_time, path_rows = arrays[0], arrays[5], arrays[6]
    class_path_time, class_top = np.zeros(nc, dtype=np.int64), np.full(nc, -1, dtype=np.int64)
    for c in range(nc):
        a, b = int(sig.class_off[c]), int(sig.class_off[c + 1])
        assert rows[a:b].tolist() == [int(k) * counted.get(c, 0) for k in sig.class_entries[a:b, 3]], c     # the invariant
        class_path_time[c] = path_time[a:b].sum()
        on = [i for i in range(a, b) if path_rows[i] > 0]
        if on:
            class_top[c] = min(on, key=lambda i: (-int(path_time[i]), i))
    summary = [sum(counted.values()), len(counted), n_rows, int((rows > 0).sum()), idle, loose]
    return ClassProfiles(*(arrays + [np.array([counted.get(c, 0) for c in range(nc)], dtype=np.int64),
                                     np.array([latency.get(c, 0) for c in range(nc)], dtype=np.int64), class_path_time, class_top, summary]),
                         class_off=sig.class_off, class_entries=sig.class_entries, mode=mode)


def write_profiles_npz(path, names, pred, true=None):
    """The class profiles as one .npz: the arrays of ClassProfiles of the predicted forest (and, prefixed true_, of the true one), the
    entries they belong to (class_off, class_entries), the mode and the group names."""
    out = {"mode": np.array(SIGNATURE_MODES[pred.mode]), "group_names": np.array([str(x) for x in names])}
    for prefix, p in (("", pred), ("true_", true)):
        if p is not None:
            out.update({prefix + k: getattr(p, k) for k in ClassProfiles.FIELDS + ("class_off", "class_entries")})
    with open(path, "wb") as f:
        np.savez_compressed(f, **out)


INT64_MAX, INT64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def _wrap64(x):
    """A Python integer as the int64 the device's wrapping sum holds."""
    return ((int(x) + (1 << 63)) % (1 << 64)) - (1 << 63)


class ClassHistory(object):
    """The class catalogue (include/traceweaver_amd.h has the definitions): call-graph classes whose ids hold across batches.
    Class k owns class_entries[class_off[k]:class_off[k + 1]], rows (level, caller group, group, count).  Per class (int64):
    trees, latency_sum, latency_min / latency_max (INT64_MAX / INT64_MIN without a tree) of the signature results pushed;
    counted, latency of the class profiles pushed; first_epoch, last_epoch, seen (the pushes and merges whose source held the
    class).  Per entry (int64): PROFILE_ENTRY_FIELDS, added up (span_min / span_max: the least and the greatest).  Derived:
    class_path_time, class_top_entry (the catalogue's global index of the entry with the largest path_time among those with a
    row on the path, -1 none).  A figure that is None (a source of Engine.class_history_merge only) adds nothing."""

    CLASS_FIELDS = ("trees", "latency_sum", "latency_min", "latency_max", "counted", "latency", "first_epoch", "last_epoch", "seen")
    ENTRY_FIELDS = PROFILE_ENTRY_FIELDS
    DERIVED_FIELDS = ("class_path_time", "class_top_entry")
    FIELDS = ("class_off", "class_entries") + CLASS_FIELDS + ENTRY_FIELDS + DERIVED_FIELDS

    def __init__(self, class_off, class_entries, trees=None, latency_sum=None, latency_min=None, latency_max=None, counted=None, latency=None,
                 first_epoch=None, last_epoch=None, seen=None, rows=None, span_time=None, span_min=None, span_max=None, self_time=None,
                 path_time=None, path_rows=None, path_trees=None, offset=None, class_path_time=None, class_top_entry=None, mode=0, n_groups=0):
        self.class_off = np.asarray(class_off, dtype=np.int64)
        self.class_entries = np.asarray(class_entries, dtype=np.int32).reshape(-1, 4)
        given = dict(locals())
        for k in self.CLASS_FIELDS + self.ENTRY_FIELDS + self.DERIVED_FIELDS:
            setattr(self, k, None if given[k] is None else np.asarray(given[k], dtype=np.int64))
        self.mode, self.n_groups = int(mode), int(n_groups)

    n_classes = property(lambda self: len(self.class_off) - 1)
    n_entries = property(lambda self: len(self.class_entries))

    @classmethod
    def from_batch(cls, signatures, profiles, n_groups):
        """One batch as a source of Engine.class_history_merge / a part's figures: a TraceSignatures and, or None, the
        ClassProfiles that belongs to it."""
        s, p = signatures, profiles
        extra = {} if p is None else dict({f: getattr(p, f) for f in PROFILE_ENTRY_FIELDS}, counted=p.class_counted, latency=p.class_latency)
        return cls(s.class_off, s.class_entries, s.class_trees, s.class_latency_sum, s.class_latency_min, s.class_latency_max, mode=s.mode,
                   n_groups=n_groups, **extra)

    def entries(self, k):
        """The signature of class k: an [n, 4] view of class_entries."""
        k = int(k)
        if not 0 <= k < self.n_classes:
            raise IndexError(k)
        return self.class_entries[int(self.class_off[k]):int(self.class_off[k + 1])]

    def signature(self, k):
        """... as a tuple of (level, caller group, group, count) tuples."""
        return tuple(tuple(int(x) for x in row) for row in self.entries(k))

    def profile(self, k):
        """The aggregate trace of class k over everything pushed: its entries in signature order, each a dict of the entry's global
        index, (level, caller, group, count) and ENTRY_FIELDS."""
        out = []
        for i in range(int(self.class_off[int(k)]), int(self.class_off[int(k) + 1])):
            lv, cg, g, n = (int(x) for x in self.class_entries[i])
            row = {"entry": i, "class": int(k), "level": lv, "caller": cg, "group": g, "count": n}
            row.update({f: int(getattr(self, f)[i]) for f in self.ENTRY_FIELDS})
            out.append(row)
        return out

    def figures(self, k):
        """The per-class figures of class k, the derived ones and its entries' figures (lists in signature order), as a dict -- the
        top entry as its position within the class, so that catalogues which number their classes differently compare equal."""
        k = int(k)
        a, b = int(self.class_off[k]), int(self.class_off[k + 1])
        out = {f: int(getattr(self, f)[k]) for f in self.CLASS_FIELDS + ("class_path_time",)}
        top = int(self.class_top_entry[k])
        out["top_entry"] = top - a if top >= 0 else -1
        out.update({f: [int(x) for x in getattr(self, f)[a:b]] for f in self.ENTRY_FIELDS})
        return out

    def by_signature(self):
        """{signature tuple: figures(k)}: what two catalogues are compared through where their ids legitimately differ."""
        return {self.signature(k): self.figures(k) for k in range(self.n_classes)}

    def table(self, names=None):
        """One dict per class, sorted by trees descending (ties: the id): id, trees, share of all trees, mean / min / max latency
        (None without a tree), first / last epoch, seen, top_entry (global index, -1 none) with top = its (level, caller,
        service) and top_share = its share of the class' path time, and the signature with the groups' names (the caller None in
        mode "levels")."""
        name = lambda g: g if names is None or g < 0 else names[g]                      # noqa: E731
        total = max(int(np.asarray(self.trees).sum()), 1)
        rows = []
        for k in sorted(range(self.n_classes), key=lambda k: (-int(self.trees[k]), k)):
            n, i, path = int(self.trees[k]), int(self.class_top_entry[k]), int(self.class_path_time[k])
            sig = [(lv, name(cg) if self.mode == 1 else None, name(g), c) for lv, cg, g, c in self.signature(k)]
            row = {"id": k, "trees": n, "share": float(n) / total, "mean_latency": float(self.latency_sum[k]) / n if n else None,
                   "min_latency": int(self.latency_min[k]) if n else None, "max_latency": int(self.latency_max[k]) if n else None,
                   "first_epoch": int(self.first_epoch[k]), "last_epoch": int(self.last_epoch[k]), "seen": int(self.seen[k]), "top_entry": i, "top": None,
                   "top_share": 0.0, "signature": sig}
            if i >= 0:
                lv, cg, g, _ = (int(x) for x in self.class_entries[i])
                row.update({"top": (lv, name(cg) if self.mode == 1 else None, name(g)), "top_share": float(self.path_time[i]) / path if path else 0.0})
            rows.append(row)
        return rows

    def same_as(self, other):
        return self.mode == other.mode and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.FIELDS)


def class_history_host(parts):
    """What the class catalogue holds after Engine.class_history_push / class_history_merge of `parts`, in turn, on an empty
    catalogue, restated with a dict keyed by the signature tuple and Python integers, for the tests.  parts: a list of (source,
    profiles, what, epoch); source is a TraceSignatures (profiles: the ClassProfiles that belongs to it, or None; what as
    tw_class_history_push takes it) or a ClassHistory (a merge: profiles and what are not read, every figure that is not None is
    added; first_epoch / last_epoch / seen None = epoch and 1).  The first part fixes the mode -- and, from a ClassHistory, the
    number of groups the entries are checked against.  Raises ValueError for what the device refuses with TW_ERR_ARG."""
    ids, sigs, cls, cells = {}, [], [], []
    mode, G = None, None
    for src, prof, what, epoch in parts:
        merge = isinstance(src, ClassHistory)
        if not merge and what not in (1, 2, 3):
            raise ValueError("class_history_host: what outside {1, 2, 3}")
        if mode is not None and src.mode != mode:
            raise ValueError("class_history_host: a part of another mode")
        if merge:
            if src.n_groups < 1 or (G is not None and src.n_groups != G):
                raise ValueError("class_history_host: a part of another number of groups")
            off = [int(x) for x in src.class_off]
            if off[0] != 0 or any(b < a for a, b in zip(off, off[1:])) or off[-1] != src.n_entries:
                raise ValueError("class_history_host: class_off does not start at 0, decreases or does not end at the entries")
            seen_sigs = set()
            for k in range(src.n_classes):
                sig = src.signature(k)
                keys = [e[:3] for e in sig]
                ok = all(a < b for a, b in zip(keys, keys[1:])) and all(
                    0 <= lv < (1 << 16) and 0 <= g < src.n_groups and c >= 1 and (-1 <= cg < src.n_groups if src.mode == 1 else cg == 0) for lv, cg, g, c in sig)
                if not ok or sig in seen_sigs:
                    raise ValueError("class_history_host: an entry out of range, entries that do not ascend or two equal classes in a source")
                seen_sigs.add(sig)
            G = src.n_groups
        mode = src.mode
        get = (lambda f: getattr(src, f)) if merge else (lambda f: None)
        if not merge:
            per_class = {}
            if what & 1:
                per_class.update(trees=src.class_trees, latency_sum=src.class_latency_sum, latency_min=src.class_latency_min, latency_max=src.class_latency_max)
            if what & 2:
                per_class.update(counted=prof.class_counted, latency=prof.class_latency)
            get = lambda f: per_class.get(f) if f in ClassHistory.CLASS_FIELDS else (getattr(prof, f) if what & 2 else None)   # noqa: E731
        for k in range(src.n_classes):
            sig = src.signature(k)
            if sig not in ids:
                ids[sig] = len(sigs)
                sigs.append(sig)
                cls.append(dict(trees=0, latency_sum=0, latency_min=INT64_MAX, latency_max=INT64_MIN, counted=0, latency=0, first_epoch=INT64_MAX,
                                last_epoch=INT64_MIN, seen=0))
                cells.append([{f: INT64_MAX if f == "span_min" else INT64_MIN if f == "span_max" else 0 for f in PROFILE_ENTRY_FIELDS} for _ in sig])
            c = cls[ids[sig]]
            for f in ("trees", "latency_sum", "counted", "latency"):
                if get(f) is not None:
                    c[f] += int(get(f)[k])
            if get("latency_min") is not None:
                c["latency_min"] = min(c["latency_min"], int(get("latency_min")[k]))
            if get("latency_max") is not None:
                c["latency_max"] = max(c["latency_max"], int(get("latency_max")[k]))
            first, last, seen = (get(f) if merge else None for f in ("first_epoch", "last_epoch", "seen"))
            c["first_epoch"] = min(c["first_epoch"], int(epoch) if first is None else int(first[k]))
            c["last_epoch"] = max(c["last_epoch"], int(epoch) if last is None else int(last[k]))
            c["seen"] += 1 if seen is None else int(seen[k])
            for j in range(len(sig)):
                i, cell = int(src.class_off[k]) + j, cells[ids[sig]][j]
                for f in PROFILE_ENTRY_FIELDS:
                    if get(f) is not None:
                        v = int(get(f)[i])
                        cell[f] = min(cell[f], v) if f == "span_min" else max(cell[f], v) if f == "span_max" else cell[f] + v
    if mode is None:
        raise ValueError("class_history_host: no parts")
    off = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    entries = np.array([e for s in sigs for e in s], dtype=np.int32).reshape(-1, 4)
    per_class = [np.array([_wrap64(c[f]) for c in cls], dtype=np.int64) for f in ClassHistory.CLASS_FIELDS]
    per_entry = [np.array([_wrap64(cell[f]) for cs in cells for cell in cs], dtype=np.int64) for f in PROFILE_ENTRY_FIELDS]
    path_time, path_rows = per_entry[5], per_entry[6]
    class_path_time, class_top = np.zeros(len(sigs), dtype=np.int64), np.full(len(sigs), -1, dtype=np.int64)
    for k in range(len(sigs)):
        a, b = int(off[k]), int(off[k + 1])
        class_path_time[k] = _wrap64(sum(int(x) for x in path_time[a:b]))
        on = [i for i in range(a, b) if path_rows[i] != 0]
        if on:
            class_top[k] = min(on, key=lambda i: (-int(path_time[i]), i))
    return ClassHistory(off, entries, *(per_class + per_entry + [class_path_time, class_top]), mode=mode, n_groups=0 if G is None else G)


def write_class_history_npz(path, catalogue, group_names):
    """A catalogue read back (Engine.class_history) as one .npz: the arrays of ClassHistory.FIELDS, the mode and the names of the
    groups.  read_class_history_npz gives what Engine.class_history_merge takes."""
    c = catalogue
    if len(group_names) != c.n_groups:
        raise ValueError("write_class_history_npz: the names do not match the catalogue's groups")
    with open(path, "wb") as f:
        np.savez_compressed(f, mode=np.array(SIGNATURE_MODES[c.mode]), n_groups=np.int64(c.n_groups), group_names=np.array([str(x) for x in group_names]),
                            **{k: getattr(c, k) for k in ClassHistory.FIELDS})


def read_class_history_npz(path):
    """-> (ClassHistory, group_names): the first is an argument of Engine.class_history_merge."""
    with np.load(path) as z:
        mode, G = SIGNATURE_MODES.index(str(z["mode"])), int(z["n_groups"])
        names = [str(x) for x in z["group_names"].tolist()]
        c = ClassHistory(*[z[k] for k in ClassHistory.FIELDS], mode=mode, n_groups=G)
    sizes = [len(getattr(c, k)) for k in ClassHistory.CLASS_FIELDS + ClassHistory.DERIVED_FIELDS] + [len(c.class_off) - 1]
    if len(names) != G or set(sizes) != {c.n_classes} or {len(getattr(c, k)) for k in ClassHistory.ENTRY_FIELDS} != {c.n_entries} or \
            (len(c.class_off) and int(c.class_off[-1]) != c.n_entries):
        raise ValueError("%s: not a class catalogue (the arrays do not match its classes, entries and groups)" % path)
    return c, names


# ---- traces selected by a predicate: Engine.filter_traces (tw_filter_traces, csrc/tw_filt.h) ---------------------------------------
MATCH = 16                           # bit of the device forest's tree_flags after Engine.filter_traces (Engine.attribute(need_flags=WHOLE | MATCH))
FILTER_MAX_CLAUSES, FILTER_MAX_TERMS = 16, 8
FILTER_SUBJECTS = ("latency", "rows", "start", "class", "group", "edge")
FILTER_METRICS = ("count", "span", "self", "path", "onpath")     # of a group / edge clause: rows, duration, self_time, path_time, rows on the critical path
FILTER_REDUCES = ("sum", "min", "max")
NO_VALUE = INT64_MIN                 # clause_value of a min / max over no rows


def clause(subject, lo=None, hi=None, term=0, group=-1, caller=-1, metric="count", reduce="sum", negate=False):
    """One clause of a filter, the tuple Engine.filter_traces takes: (term, subject, group, caller, metric, reduce, negate, lo, hi).
    subject: one of FILTER_SUBJECTS; "group" reads group (-1: every counted row), "edge" group and caller (-1: no caller); metric
    and reduce by name (FILTER_METRICS, FILTER_REDUCES).  The clause holds where lo <= value <= hi (None: unbounded), then negated."""
    index = lambda names, x: names.index(x) if isinstance(x, str) else int(x)
    return (int(term), index(FILTER_SUBJECTS, subject), int(group), int(caller), index(FILTER_METRICS, metric), index(FILTER_REDUCES, reduce),
            1 if negate else 0, INT64_MIN if lo is None else int(lo), INT64_MAX if hi is None else int(hi))


def format_clause(c, names=None):
    """A clause tuple in the language of parse_filter (groups by name when `names` is given, by number otherwise)."""
    term, subject, group, caller, metric, reduce, negate, lo, hi = (int(x) for x in c)
    name = lambda g, none: none if g < 0 else (str(g) if names is None else str(names[g]))
    if subject < 4:
        what = FILTER_SUBJECTS[subject]
    else:
        what = FILTER_METRICS[metric] + ("" if reduce == 0 else "." + FILTER_REDUCES[reduce])
        what += "[%s]" % name(group, "*") if subject == 4 else "[%s>%s]" % (name(caller, "-"), name(group, "*"))
    if lo == hi:
        cmp_ = "==%d" % lo
    elif hi == INT64_MAX:
        cmp_ = ">=%d" % lo
    elif lo == INT64_MIN:
        cmp_ = "<=%d" % hi
    else:
        cmp_ = " in %d..%d" % (lo, hi)
    return ("!" if negate else "") + what + cmp_


def format_filter(clauses, names=None):
    """Clause tuples as one expression: the terms in ascending order joined by ' | ', a term's clauses by ' & '."""
    terms = sorted({int(c[0]) for c in clauses})
    return " | ".join(" & ".join(format_clause(c, names) for c in clauses if int(c[0]) == k) for k in terms)


def parse_filter(expr, names):
    """The command line's filter language -> clause tuples.  `|` separates terms (numbered from 0), `&` the clauses of a term, a
    leading `!` negates.  A clause is SUBJECT COMPARISON with SUBJECT one of latency, rows, start, class, METRIC[.REDUCE][SERVICE]
    (a group clause; `*` = any counted service) or METRIC[.REDUCE][CALLER>SERVICE] (an edge clause; `-` = no caller), METRIC one of
    count, span, self, path, onpath, REDUCE one of sum (the default), min, max, the brackets literal; COMPARISON one of >=V, <=V,
    ==V, `in LO..HI`, integers in microseconds.  names: the groups' names (services) in group order.  ValueError names the piece
    that is wrong: an unknown service, subject, metric or reduction, a ninth term, a seventeenth clause."""
    import re

    names = [str(x) for x in names]

    def service(x, piece, star):
        x = x.strip()
        if x == star:
            return -1
        if x not in names:
            raise ValueError("filter clause %r: unknown service %r" % (piece, x))
        return names.index(x)

    out = []
    terms = str(expr).split("|")
    for k, term in enumerate(terms):
        if k >= FILTER_MAX_TERMS:
            raise ValueError("filter term %d (%r): at most %d terms" % (k + 1, term.strip(), FILTER_MAX_TERMS))
        for piece in term.split("&"):
            piece = piece.strip()
            m = re.match(r"^(!?)\s*([a-z]+)(?:\.([a-z]+))?\s*(?:\[([^\]]*)\])?\s*(>=|<=|==|in\s)\s*(.+)$", piece)
            if m is None:
                raise ValueError("filter clause %r: not of the form [!]SUBJECT (>=|<=|==|in) VALUE" % piece)
            if len(out) >= FILTER_MAX_CLAUSES:
                raise ValueError("filter clause %d (%r): at most %d clauses" % (len(out) + 1, piece, FILTER_MAX_CLAUSES))
            neg, what, red, inside, op, value = m.groups()
            try:
                if op.strip() == "in":
                    lo, hi = (int(x) for x in value.split(".."))
                else:
                    v = int(value)
                    lo, hi = {">=": (v, None), "<=": (None, v), "==": (v, v)}[op]
            except ValueError:
                raise ValueError("filter clause %r: %r is no integer (or LO..HI after `in`)" % (piece, value.strip()))
            if lo is not None and hi is not None and lo > hi:
                raise ValueError("filter clause %r: LO > HI" % piece)
            if inside is None:
                if what not in FILTER_SUBJECTS[:4] or red is not None:
                    raise ValueError("filter clause %r: unknown subject %r (latency, rows, start, class, or METRIC[SERVICE])" % (piece, what + ("." + red if red else "")))
                out.append(clause(what, lo, hi, term=k, negate=bool(neg)))
                continue
            if what not in FILTER_METRICS:
                raise ValueError("filter clause %r: unknown metric %r (%s)" % (piece, what, ", ".join(FILTER_METRICS)))
            if red is not None and red not in FILTER_REDUCES:
                raise ValueError("filter clause %r: unknown reduction %r (%s)" % (piece, red, ", ".join(FILTER_REDUCES)))
            red = red or "sum"
            if what in ("count", "onpath") and red != "sum":
                raise ValueError("filter clause %r: %s is a count, it has no %s" % (piece, what, red))
            if ">" in inside:
                caller, callee = inside.split(">", 1)
                if what not in ("count", "span"):
                    raise ValueError("filter clause %r: an edge has count and span only, not %r" % (piece, what))
                if callee.strip() == "*":
                    raise ValueError("filter clause %r: an edge names its callee" % piece)
                out.append(clause("edge", lo, hi, term=k, group=service(callee, piece, None), caller=service(caller, piece, "-"), metric=what, reduce=red,
                                  negate=bool(neg)))
            else:
                out.append(clause("group", lo, hi, term=k, group=service(inside, piece, "*"), metric=what, reduce=red, negate=bool(neg)))
    return out


class TraceFilter(object):
    """What Engine.filter_traces returns (include/traceweaver_amd.h has the definitions): tree_match uint8 [n_trees]; match_trees
    int32, the matched trees in ascending order; clause_value int64 [n_trees, n_clauses] (NO_VALUE: a min / max over no rows);
    clause_trees int64 [n_clauses]: eligible trees on which the clause holds; term_trees int64 [FILTER_MAX_TERMS]: eligible trees on
    which every clause of the term holds (0 for a term without a clause); summary = eligible trees, matched trees, sum / min / max of
    their latency (INT64_MAX / INT64_MIN without a match), their rows.  clauses (not compared by same_as): the query's tuples."""

    FIELDS = ("tree_match", "match_trees", "clause_value", "clause_trees", "term_trees", "summary")

    def __init__(self, tree_match, match_trees, clause_value, clause_trees, term_trees, summary, clauses=()):
        self.tree_match, self.match_trees, self.clause_trees, self.term_trees = tree_match, match_trees, clause_trees, term_trees
        self.clauses = [tuple(int(x) for x in c) for c in clauses]
        self.clause_value = np.asarray(clause_value, dtype=np.int64).reshape(len(tree_match), len(self.clauses))
        self.summary = np.asarray(summary, dtype=np.int64)

    n_eligible = property(lambda self: int(self.summary[0]))
    n_matched = property(lambda self: int(self.summary[1]))

    def matched(self):
        """The matched trees, ascending (match_trees)."""
        return self.match_trees

    def table(self, names=None):
        """One dict per clause ({"clause", "term", "text", "trees"}) and then one per term with a clause ({"term", "text", "trees"}):
        the eligible trees it holds on, and its text in the language of parse_filter."""
        rows = [{"clause": j, "term": c[0], "text": format_clause(c, names), "trees": int(self.clause_trees[j])} for j, c in enumerate(self.clauses)]
        for k in sorted({c[0] for c in self.clauses}):
            rows.append({"term": k, "text": " & ".join(format_clause(c, names) for c in self.clauses if c[0] == k), "trees": int(self.term_trees[k])})
        return rows

    def same_as(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.FIELDS)


def write_filter_npz(path, result, names):
    """A TraceFilter as one .npz: its arrays, the clauses as an [n, 9] int64 table (the columns of clause()), the expression in
    the language of parse_filter and the group names."""
    out = {k: getattr(result, k) for k in TraceFilter.FIELDS}
    out.update({"clauses": np.array(result.clauses, dtype=np.int64).reshape(-1, 9), "expression": np.array(format_filter(result.clauses, names)),
                "group_names": np.array([str(x) for x in names])})
    with open(path, "wb") as f:
        np.savez_compressed(f, **out)


def filter_host(stitched, link, row_kind, row_start, row_end, row_group, n_groups, clauses, need_flags=WHOLE, skip_flags=0, attribution=None,
                signatures=None):
    """What tw_filter_traces computes, restated from the definitions in plain Python, for the tests: a loop over the rows of every
    tree per clause, dictionaries for the counts.  attribution: the host result of attribute_host on the same forest (self_time,
    path_time; the rows on the critical path are walked again here), needed by the metrics self, path and onpath; signatures: the
    result of signatures_host whose tree_class a class clause reads.  ValueError where the device refuses."""
    link = [int(x) for x in link]
    kind = [int(x) for x in row_kind]
    group = [int(x) for x in row_group]
    start = [int(x) for x in row_start]
    end = [max(int(e), s) for e, s in zip(row_end, start)]
    clauses = [tuple(int(x) for x in c) for c in clauses]
    if len(clauses) > FILTER_MAX_CLAUSES:
        raise ValueError("more than %d clauses" % FILTER_MAX_CLAUSES)
    walked = None
    for term, subject, g, cg, metric, reduce, negate, lo, hi in clauses:
        if not (0 <= term < FILTER_MAX_TERMS and 0 <= subject <= 5 and lo <= hi):
            raise ValueError("term, subject or bounds out of range")
        if subject >= 4:
            edge = subject == 5
            if not (0 <= metric <= (1 if edge else 4) and 0 <= reduce <= 2 and (-1 if not edge else 0) <= g < n_groups and (not edge or -1 <= cg < n_groups)):
                raise ValueError("group, caller, metric or reduce out of range")
            if metric in (0, 4) and reduce != 0:
                raise ValueError("a count is summed")
            if metric >= 2 and attribution is None:
                raise ValueError("a clause on times without an attribution")
            if metric == 4 and walked is None:
                children = [[] for _ in link]
                for c, p in enumerate(link):
                    if p >= 0:
                        children[p].append(c)
                _, walked = critical_paths_host(children, start, end, stitched.tree_root)
        if subject == 3 and signatures is None:
            raise ValueError("a class clause without signatures")

    def caller_group(r):                                          # the group of the nearest server row above r, -1 without one
        p = link[r]
        while p >= 0:
            if kind[p] == 1:
                return group[p]
            p = link[p]
        return -1

    def row_value(r, metric):
        if metric == 0:
            return 1
        if metric == 1:
            return end[r] - start[r]
        if metric == 2:
            return int(attribution.self_time[r])
        if metric == 3:
            return int(attribution.path_time[r])
        return 1 if walked[r] else 0

    nt, nc = stitched.n_trees, len(clauses)
    flags = np.asarray(stitched.tree_flags).astype(np.int64)
    value = np.full((nt, nc), NO_VALUE, dtype=np.int64)
    match = np.zeros(nt, dtype=np.uint8)
    clause_trees, term_trees = {}, {}
    used = sorted({c[0] for c in clauses})
    eligible = 0
    for t in range(nt):
        rows = [int(r) for r in stitched.tree_rows[int(stitched.tree_off[t]):int(stitched.tree_off[t + 1])]]
        holds = []
        for j, (term, subject, g, cg, metric, reduce, negate, lo, hi) in enumerate(clauses):
            if subject == 0:
                v = int(stitched.tree_latency[t])
            elif subject == 1:
                v = len(rows)
            elif subject == 2:
                v = start[int(stitched.tree_root[t])]
            elif subject == 3:
                v = int(signatures.tree_class[t])
            else:
                if subject == 4:
                    picked = [r for r in rows if (group[r] >= 0 if g < 0 else group[r] == g)]
                else:
                    picked = [r for r in rows if kind[r] == 1 and group[r] == g and caller_group(r) == cg]
                values = [row_value(r, metric) for r in picked]
                if reduce == 0:
                    v = _wrap64(sum(values))
                elif not values:
                    v = None
                else:
                    v = min(values) if reduce == 1 else max(values)
            if v is not None:
                value[t, j] = v
            holds.append(v is not None and ((lo <= v <= hi) != bool(negate)))
        if not ((flags[t] & need_flags) == need_flags and (flags[t] & skip_flags) == 0):
            continue
        eligible += 1
        for j, h in enumerate(holds):
            if h:
                clause_trees[j] = clause_trees.get(j, 0) + 1
        good = [k for k in used if all(h for h, c in zip(holds, clauses) if c[0] == k)]
        for k in good:
            term_trees[k] = term_trees.get(k, 0) + 1
        match[t] = 1 if (nc == 0 or good) else 0
    listed = [t for t in range(nt) if match[t]]
    lat = [int(stitched.tree_latency[t]) for t in listed]
    n_rows = sum(int(stitched.tree_off[t + 1]) - int(stitched.tree_off[t]) for t in listed)
    summary = [eligible, len(listed), _wrap64(sum(lat)), min(lat) if lat else INT64_MAX, max(lat) if lat else INT64_MIN, n_rows]
    return TraceFilter(match, np.array(listed, dtype=np.int32), value, np.array([clause_trees.get(j, 0) for j in range(nc)], dtype=np.int64),
                       np.array([term_trees.get(k, 0) for k in range(FILTER_MAX_TERMS)], dtype=np.int64), summary, clauses)


# ---- reconstructed traces handed out as trees: exemplars, pre-order rows (tw_extract_traces, csrc/tw_extr.h) ----
EXTRACT_MODES = ("top", "quantiles", "list")
EXTRACT_ORDERS = ("tree", "slowest", "fastest")
EXTRACT_MAX_PROBS = 32               # TW_EXTR_MAX_PROBS
EXTRACT_MAX_LIST = 1 << 20           # TW_EXTR_MAX_LIST
EXTRACT_SINGLE_ROWS = 256            # kExtrCap of csrc/tw_extr.h: a tree of more rows is taken by the single-tree route (summary[4] counts them)


def _extract_code(names, x, what):
    if isinstance(x, str):
        if x not in names:
            raise ValueError("%s %r is none of %s" % (what, x, ", ".join(names)))
        return names.index(x)
    return int(x)


class ExtractedTraces(object):
    """What Engine.extract_traces returns (include/traceweaver_amd.h has the definitions): a packed sub-forest.  Output tree j owns the
    positions out_off[j] .. out_off[j + 1] of the per-row columns, its rows in pre-order (children by (start, row)); per tree sel_tree
    (the source tree), sel_root, sel_latency, sel_start, sel_flags; per row: row (span-table row), parent (local index, -1 for the
    root, always smaller than the row's own), depth, subtree (rows of the subtree, itself included), kind (1 the hop above was
    observed, 2 predicted, 0 absent), group (-1 without row groups), start, end, self_time / path_time (empty where the result holds
    no times: summary[5] == 0).  summary = eligible trees, selected trees, their rows, the rows of the largest, the trees taken by the
    single-tree route, 1 if the times are held."""

    TREE_FIELDS = ("sel_tree", "sel_root", "sel_latency", "sel_start", "sel_flags")
    ROW_FIELDS = ("row", "parent", "depth", "subtree", "kind", "group", "start", "end", "self_time", "path_time")
    FIELDS = TREE_FIELDS + ("out_off",) + ROW_FIELDS + ("summary",)
    DTYPES = {"sel_tree": np.int32, "sel_root": np.int32, "sel_flags": np.uint8, "row": np.int32, "parent": np.int32, "depth": np.int32,
              "subtree": np.int32, "kind": np.uint8, "group": np.int32}       # every other field: int64

    def __init__(self, summary, **columns):
        for k in self.FIELDS[:-1]:
            setattr(self, k, np.asarray(columns[k], dtype=self.DTYPES.get(k, np.int64)))
        self.summary = np.asarray(summary, dtype=np.int64)

    n_trees = property(lambda self: len(self.sel_tree))
    n_eligible = property(lambda self: int(self.summary[0]))
    has_times = property(lambda self: bool(self.summary[5]))

    def __len__(self):
        return self.n_trees

    def trace(self, j):
        """Output tree j: a dict of its columns ({"tree", "root", "latency", "start_time", "flags"} and the per-row arrays)."""
        j = int(j)
        if not 0 <= j < self.n_trees:
            raise IndexError(j)
        a, b = int(self.out_off[j]), int(self.out_off[j + 1])
        out = {"tree": int(self.sel_tree[j]), "root": int(self.sel_root[j]), "latency": int(self.sel_latency[j]), "start_time": int(self.sel_start[j]),
               "flags": int(self.sel_flags[j])}
        for k in self.ROW_FIELDS:
            col = getattr(self, k)
            out[k] = col[a:b] if len(col) else col
        return out

    def children(self, j, i):
        """Local indices of the children of row i of output tree j, in their order: i + 1, then from sibling to sibling by `subtree`."""
        a = int(self.out_off[j])
        out, c, end = [], i + 1, i + int(self.subtree[a + i])
        while c < end:
            out.append(c)
            c += int(self.subtree[a + c])
        return out

    def render(self, j, names=None):
        """Output tree j as an indented text waterfall, one line per row: the group's name (names[group]; the row number without
        one), the start as an offset from the root's, the duration, self / path time where held, `*` on a predicted hop."""
        t = self.trace(j)
        lines = ["trace %d: tree %d, root row %d, %d rows, latency %d us%s" % (j, t["tree"], t["root"], len(t["row"]), t["latency"],
                                                                                "" if t["flags"] & WHOLE else " (fragment)")]
        for i in range(len(t["row"])):
            g = int(t["group"][i])
            name = str(names[g]) if names is not None and 0 <= g < len(names) else ("group %d" % g if g >= 0 else "row %d" % int(t["row"][i]))
            text = "%s%s%s +%d us, %d us" % ("  " * (int(t["depth"][i]) + 1), "* " if int(t["kind"][i]) == 2 else "", name,
                                             int(t["start"][i]) - t["start_time"], max(int(t["end"][i]) - int(t["start"][i]), 0))
            if self.has_times:
                text += " (self %d, path %d)" % (int(t["self_time"][i]), int(t["path_time"][i]))
            lines.append(text)
        return "\n".join(lines)

    def same_as(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.FIELDS)


def extract_host(stitched, link, row_kind, row_start, row_end, row_group=None, mode="top", order="slowest", limit=0, probs=(), trees=None,
                 need_flags=WHOLE, skip_flags=0, attribution=None, single_rows=EXTRACT_SINGLE_ROWS):
    """What tw_extract_traces / tw_get_extracted compute, restated from the definitions in plain Python, for the tests: the selection
    with sorted(), the pre-order by recursion over children().  stitched.tree_flags: the flags as the device holds them (CONFIDENT,
    MATCH included where a query names them).  row_group None: no row groups are resident.  attribution: the host result whose self /
    path times are gathered.  single_rows: kExtrCap of the build (summary[4] counts the selected trees beyond it).  ValueError where
    the device returns TW_ERR_ARG."""
    import math

    mode, order = _extract_code(EXTRACT_MODES, mode, "mode"), _extract_code(EXTRACT_ORDERS, order, "order")
    nt = stitched.n_trees
    latency = [int(x) for x in stitched.tree_latency]
    flags = [int(x) for x in stitched.tree_flags]
    if mode not in (0, 1, 2):
        raise ValueError("mode out of range")
    eligible = [t for t in range(nt) if (flags[t] & need_flags) == need_flags and (flags[t] & skip_flags) == 0]
    if mode == 0:
        if order not in (0, 1, 2):
            raise ValueError("order out of range")
        if int(limit) < 0:
            raise ValueError("limit is negative")
        key = {0: lambda t: t, 1: lambda t: (-latency[t], t), 2: lambda t: (latency[t], t)}[order]
        chosen = sorted(eligible, key=key)
        if int(limit) > 0:
            chosen = chosen[:int(limit)]
        n_eligible = len(eligible)
    elif mode == 1:
        probs = [float(p) for p in probs]
        if len(probs) > EXTRACT_MAX_PROBS:
            raise ValueError("more than %d probs" % EXTRACT_MAX_PROBS)
        if any(math.isnan(p) or p < 0.0 or p > 1.0 for p in probs):
            raise ValueError("a prob outside [0, 1]")
        by_latency = sorted(eligible, key=lambda t: (latency[t], t))
        n = len(by_latency)
        chosen = [by_latency[min(n - 1, int(p * float(n)))] for p in probs] if n else []
        n_eligible = n
    else:
        chosen = [int(t) for t in ([] if trees is None else trees)]
        if len(chosen) > EXTRACT_MAX_LIST:
            raise ValueError("more than 2^20 listed trees")
        if any(t < 0 or t >= nt for t in chosen):
            raise ValueError("a listed tree outside [0, n_trees)")
        n_eligible = nt
    link = [int(x) for x in link]
    start = [int(x) for x in row_start]
    cols = {k: [] for k in ExtractedTraces.FIELDS[:-1]}
    cols["out_off"].append(0)
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 100000))
    largest = single = 0
    for t in chosen:
        rows = [int(r) for r in stitched.tree_rows[int(stitched.tree_off[t]):int(stitched.tree_off[t + 1])]]
        root = int(stitched.tree_root[t])
        kids = {r: [] for r in rows}
        for c in rows:
            if link[c] >= 0:
                kids[link[c]].append(c)
        local, base = {}, len(cols["row"])

        def visit(p):
            """Emits p and its subtree; returns the subtree's rows."""
            at = len(cols["row"])
            local[p] = at - base
            cols["row"].append(p)
            cols["parent"].append(-1 if p == root else local[link[p]])
            cols["subtree"].append(0)
            count = 1
            for c in sorted(kids[p], key=lambda c: (start[c], c)):
                count += visit(c)
            cols["subtree"][at] = count
            return count

        visit(root)
        cols["out_off"].append(len(cols["row"]))
        largest = max(largest, len(rows))
        single += len(rows) > single_rows
        cols["sel_tree"].append(t)
        cols["sel_root"].append(root)
        cols["sel_latency"].append(latency[t])
        cols["sel_start"].append(start[root])
        cols["sel_flags"].append(flags[t])
    for r in cols["row"]:
        cols["depth"].append(int(stitched.depth[r]))
        cols["kind"].append(int(row_kind[r]))
        cols["group"].append(-1 if row_group is None else int(row_group[r]))
        cols["start"].append(start[r])
        cols["end"].append(int(row_end[r]))
        if attribution is not None:
            cols["self_time"].append(int(attribution.self_time[r]))
            cols["path_time"].append(int(attribution.path_time[r]))
    summary = [n_eligible, len(chosen), len(cols["row"]), largest, single, 1 if attribution is not None else 0]
    return ExtractedTraces(summary, **cols)


def write_extracted_npz(path, extracted, names):
    """An ExtractedTraces as one .npz: its arrays and the group names."""
    out = {k: getattr(extracted, k) for k in ExtractedTraces.FIELDS}
    out["group_names"] = np.array([str(x) for x in names])
    with open(path, "wb") as f:
        np.savez_compressed(f, **out)


def write_jaeger(directory, extracted, corpus, table=None):
    """The extracted traces as Jaeger JSON, one file per output tree in the shape the loader reads ({"data": [{"traceID", "spans",
    "processes"}]}): every span keeps the corpus's spanID, operationName, startTime and duration and gets a processID whose process
    names its service; span.kind (server / client) from `kind`; a CHILD_OF reference to the local parent's span on every row but the
    root; the tag tw.hop = observed | predicted (from `kind`), tw.self_us / tw.path_us where the times are held.  traceID =
    "tw-" + the root's span id; a tree that was written before (a LIST with duplicates) gets the suffix -<j>.  Ground truth is not
    consulted: the references are the reconstructed links.  Returns the paths."""
    import json
    import os

    table = corpus.span_table() if table is None else table
    os.makedirs(directory, exist_ok=True)
    seen, paths = set(), []
    for j in range(extracted.n_trees):
        t = extracted.trace(j)
        sid = [corpus.string(table["span_id"][r]) for r in t["row"]]
        tid = "tw-" + sid[0]
        if tid in seen:
            tid += "-%d" % j
        seen.add(tid)
        processes, spans = {}, []
        for i, r in enumerate(t["row"]):
            service = corpus.string(table["service"][r])
            pid = processes.setdefault(service, "p%d" % (len(processes) + 1))
            kind = int(t["kind"][i])
            p = int(t["parent"][i])
            tags = [{"key": "span.kind", "type": "string", "value": "client" if kind == 2 else "server"},
                    {"key": "tw.hop", "type": "string", "value": "predicted" if kind == 2 else "observed"}]
            if extracted.has_times:
                tags += [{"key": "tw.self_us", "type": "int64", "value": int(t["self_time"][i])}, {"key": "tw.path_us", "type": "int64", "value": int(t["path_time"][i])}]
            spans.append({"traceID": tid, "spanID": sid[i], "operationName": corpus.string(table["op_name"][r]),
                          "references": [] if p < 0 else [{"refType": "CHILD_OF", "traceID": tid, "spanID": sid[p]}],
                          "startTime": int(table["start"][r]), "duration": int(table["duration"][r]), "tags": tags, "logs": [], "processID": pid, "warnings": None})
        doc = {"data": [{"traceID": tid, "spans": spans, "processes": {pid: {"serviceName": s, "tags": []} for s, pid in processes.items()}, "warnings": None}]}
        paths.append(os.path.join(directory, tid + ".json"))
        with open(paths[-1], "w") as f:
            json.dump(doc, f)
    return paths
