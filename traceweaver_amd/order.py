"""The call-order DAG from timestamps alone: the reference's greedy search, run for all units at once.

Replaces: FindConstraintsUsingFit (executor.py:152-212).  Every solve of this engine takes a call-order DAG, and the only
other producer of one is FindOrder (executor.py:214-285; `Engine.find_order`, `synth.find_order`), which reads the true
assignment.  The reference's answer for a user who only has spans is a search: walk the ordered endpoint pairs (a, b), a != b,
in partition-key order; skip the pair if b -> a is already in the graph; otherwise add a -> b, run FindAssignments under the
candidate graph and keep the edge iff no request is left unassigned (cnt_unassigned <= 0).  That is up to E(E-1) full solves
per service -- the loop this engine makes cheap:

  * `Engine.order_bound` (csrc/tw_order.h, k_order_bound): a necessary condition per pair from the timestamps alone.  A pair
    with viol[a, b] > 0 is proven to fail the reference's test; its solve is never run (decided_by "bound").
  * `Engine.order_stage` uploads the spans once; `Engine.order_load` gathers them on the device into the topological order of
    every candidate graph (k_order_gather), so a candidate costs no upload.
  * every round solves the next candidate of EVERY unit that is still searching in one batch: at most E(E-1) <= 56 rounds for
    the whole batch, whatever the number of units.

The loop lives in Python on purpose: it makes E^2 small decisions per unit, and the refit between the two passes is the
caller's choice here as everywhere in this package.

Differences to the reference, all stated in the log:
  * a pair a -> b that would close a cycle longer than two (b reaches a over several edges) makes the reference raise in
    nx.topological_sort (traceweaver_v1.py:39).  Here the pair is rejected and logged as "cycle".
  * the reference's first solve, of the edgeless graph (executor.py:176-180), decides nothing and is not run.
  * pairs rejected by the bound are not solved; their cnt_unassigned is not known (None in the log).
Limits: no skip mode, no load-scaled units, no parts of split services (tw_order_stage refuses them); one engine's batch; the
result depends on the pair order exactly as the reference's does (an edge kept early constrains the solves of later pairs).
"""
import numpy as np

from .engine import UnitArrays

DECIDED_BY = ("solve", "bound", "reverse", "cycle")


def ordered_pairs(E):
    """for osp_1 in keys: for osp_2 in keys: if osp_1 != osp_2 (executor.py:182-184)."""
    return [(a, b) for a in range(E) for b in range(E) if a != b]


def topological_order(dag):
    """nx.topological_sort (traceweaver_v1.py:37-39) of the graph `dag` [E, E] whose nodes were inserted in index (partition
    key) order and whose edges were added in the order the search adds them -- pairs (a, b) in key order, so a node's
    successors are met in ascending index order.  networkx yields generation after generation, a generation in the order in
    which its nodes lost their last predecessor.  Raises ValueError on a cycle."""
    dag = np.asarray(dag)
    E = dag.shape[0]
    indeg = [int(dag[:, c].sum()) for c in range(E)]
    order = [a for a in range(E) if indeg[a] == 0]
    h = 0
    while h < len(order):
        a = order[h]
        h += 1
        for c in range(E):
            if dag[a, c]:
                indeg[c] -= 1
                if indeg[c] == 0:
                    order.append(c)
    if len(order) != E:
        raise ValueError("the candidate graph has a cycle")
    return order


class _LazyPermuted(UnitArrays):
    """A staged unit seen in the topological order of a candidate graph; the permuted outgoing arrays are only built when read."""

    def __init__(self, base, order, dag, key_rank):
        self.time_scale, self.part = base.time_scale, base.part
        self.in_start, self.in_end = base.in_start, base.in_end
        self.E, self.n_in = base.E, base.n_in
        lens = np.diff(base.out_off)[order]
        self.out_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.dag, self.key_rank = dag, key_rank
        self._base, self._order = base, order

    def __getattr__(self, name):
        if name in ("out_start", "out_end"):
            b = self._base
            src = getattr(b, name)
            val = np.ascontiguousarray(np.concatenate([src[b.out_off[e]:b.out_off[e + 1]] for e in self._order]))
            setattr(self, name, val)
            return val
        raise AttributeError(name)


def permuted_unit(unit, dag_key, lazy=False):
    """`unit` (endpoints in key order) as the solver takes it under the graph dag_key [E, E] (key order): endpoints in
    topological_order(dag_key), dag in that order, key_rank[k] = key index of the k-th endpoint."""
    dag_key = np.asarray(dag_key, dtype=np.uint8).reshape(unit.E, unit.E)
    order = topological_order(dag_key)
    dag = np.ascontiguousarray(dag_key[np.ix_(order, order)])
    key_rank = np.array(order, dtype=np.int32)
    if lazy:
        return _LazyPermuted(unit, order, dag, key_rank)
    seg = lambda a: np.concatenate([a[unit.out_off[e]:unit.out_off[e + 1]] for e in order])
    off = np.concatenate([[0], np.cumsum(np.diff(unit.out_off)[order])])
    return UnitArrays(unit.in_start, unit.in_end, off, seg(unit.out_start), seg(unit.out_end), dag, key_rank,
                      time_scale=unit.time_scale, part=unit.part)


def key_order_unit(unit):
    """A loaded-form unit (endpoints in some topological order, key_rank = their key index) back in partition-key order.
    Returns (unit in key order with an empty dag, perm) with perm[k] = the unit's endpoint that has key index k."""
    perm = [int(x) for x in np.argsort(unit.key_rank, kind="stable")]
    seg = lambda a: np.concatenate([a[unit.out_off[e]:unit.out_off[e + 1]] for e in perm])
    off = np.concatenate([[0], np.cumsum(np.diff(unit.out_off)[perm])])
    u = UnitArrays(unit.in_start, unit.in_end, off, seg(unit.out_start), seg(unit.out_end), np.zeros((unit.E, unit.E), np.uint8),
                   time_scale=unit.time_scale, part=unit.part)
    return u, perm


def order_bound_host(units):
    """numpy restatement of tw_order_bound: per unit int64 [E, E], viol[a, b] = the number of requests r for which no pair
    (x of a, y of b) has in_start[r] <= start <= end <= in_end[r] for both spans and end_a[x] <= start_b[y].  With m_e(r) the
    earliest end and M_e(r) the latest start among endpoint e's spans contained in r: violated iff m_a(r) > M_b(r), or either
    endpoint has no contained span."""
    out = []
    big, small = np.iinfo(np.int64).max, np.iinfo(np.int64).min
    for u in units:
        E, n = u.E, u.n_in
        m = np.full((E, n), big, dtype=np.int64)
        M = np.full((E, n), small, dtype=np.int64)
        for e in range(E):
            s, t = u.out_start[u.out_off[e]:u.out_off[e + 1]], u.out_end[u.out_off[e]:u.out_off[e + 1]]
            for r in range(n):
                inside = (s >= u.in_start[r]) & (t <= u.in_end[r])
                if inside.any():
                    m[e, r], M[e, r] = t[inside].min(), s[inside].max()
        viol = np.zeros((E, E), dtype=np.int64)
        for a in range(E):
            for b in range(E):
                if a != b:
                    viol[a, b] = int(np.count_nonzero(m[a] > M[b]))
        out.append(viol)
    return out


def _reaches(dag, src, dst):
    """True iff dst can be reached from src over the edges of dag."""
    seen, todo = {src}, [src]
    while todo:
        x = todo.pop()
        if x == dst:
            return True
        for y in np.flatnonzero(dag[x]).tolist():
            if y not in seen:
                seen.add(y)
                todo.append(y)
    return False


class _Search(object):
    """The state of one unit's walk over its ordered pairs."""

    def __init__(self, E, viol):
        self.dag = np.zeros((E, E), dtype=np.uint8)
        self.pairs = ordered_pairs(E)
        self.pos = 0
        self.viol = viol
        self.log = []
        self.pending = None

    def advance(self):
        """Walks on to the next pair that needs a solve, logging the ones decided without one.  Returns False at the end."""
        while self.pos < len(self.pairs):
            a, b = self.pairs[self.pos]
            self.pos += 1
            if self.dag[b, a]:                                        # executor.py:186
                self.log.append((a, b, "reverse", None))
            elif self.viol is not None and self.viol[a, b] > 0:
                self.log.append((a, b, "bound", None))
            elif _reaches(self.dag, b, a):                            # the reference raises here (nx.topological_sort)
                self.log.append((a, b, "cycle", None))
            else:
                self.pending = (a, b)
                return True
        self.pending = None
        return False

    def candidate(self):
        d = self.dag.copy()
        d[self.pending] = 1
        return d

    def decide(self, cnt_unassigned):
        a, b = self.pending
        if cnt_unassigned <= 0:                                       # executor.py:197
            self.dag[a, b] = 1
        self.log.append((a, b, "solve", int(cnt_unassigned)))
        self.pending = None


class InferredOrder(object):
    """dags: per unit uint8 [E, E] in key order (the reference's best_graph as a matrix; not transitively closed unless the
    search closed it).  logs: per unit the list of (a, b, decided_by, cnt_unassigned) in pair order, decided_by one of
    DECIDED_BY, cnt_unassigned = pass 2's count for "solve" and None otherwise; an edge is in the graph iff its entry is a
    "solve" with cnt_unassigned <= 0.  rounds: batched solves run; solves: candidate graphs solved, over all units."""

    def __init__(self, dags, logs, rounds, solves, viol=None):
        self.dags, self.logs, self.rounds, self.solves, self.viol = dags, logs, int(rounds), int(solves), viol

    def graph(self, k, names=None):
        """Unit k's graph as the reference builds it: nodes in key order, edges in the order the search kept them."""
        import networkx as nx

        E = self.dags[k].shape[0]
        names = list(range(E)) if names is None else list(names)
        g = nx.DiGraph()
        g.add_nodes_from(names)
        for a, b, how, cnt in self.logs[k]:
            if how == "solve" and cnt <= 0:
                g.add_edge(names[a], names[b])
        return g


def infer_order_host(units, solve, use_bound=True):
    """The same loop around any two-pass solver: solve(unit) -> cnt_unassigned of pass 2, for `unit` = permuted_unit(unit in key
    order, candidate graph).  Unit after unit; rounds = the largest number of solves of a unit (what the batched loop needs)."""
    viol = order_bound_host(units) if use_bound else [None] * len(units)
    dags, logs, per_unit = [], [], []
    for u, v in zip(units, viol):
        s, n = _Search(u.E, v), 0
        while s.advance():
            s.decide(solve(permuted_unit(u, s.candidate())))
            n += 1
        dags.append(s.dag)
        logs.append(s.log)
        per_unit.append(n)
    return InferredOrder(dags, logs, max(per_unit) if per_unit else 0, sum(per_unit), viol if use_bound else None)


def infer_order(engine, units, seeds=None, mixtures=None, use_bound=True, batch_size=100, batch_size_mis=30):
    """The search for all `units` (UnitArrays, endpoints in partition-key order; dag / key_rank are not read) on `engine`.

    Every round, each unit that is still searching contributes its next real candidate; the round runs order_load -> pass 1 ->
    refit -> pass 2 over those units only, and a unit keeps the edge iff its pass-2 cnt_unassigned is <= 0.
    Refit: by default tw_fit_mixtures_seeded with seeds[k] for unit k (default: k) -- a unit's result does not depend on which
    units share its rounds.  mixtures = callable(unit, gaps) -> (mix_n [nslot], mix_p [nslot, 5, 3]) supplies the tables
    instead (unit = the permuted unit, gaps = its [nslot, n_in] pass-1 gap rows, NaN = none)."""
    units = list(units)
    seeds = list(range(len(units))) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != len(units):
        raise ValueError("one seed per unit")
    engine.order_stage(units, batch_size=batch_size, batch_size_mis=batch_size_mis)
    viol = engine.order_bound(units) if use_bound else [None] * len(units)
    search = [_Search(u.E, v) for u, v in zip(units, viol)]
    rounds = solves = 0
    while True:
        active = [k for k, s in enumerate(search) if s.advance()]
        if not active:
            break
        engine.order_load(active, [search[k].candidate() for k in active])
        engine.run_pass1()
        if mixtures is None:
            engine.fit_mixtures(unit_seeds=[seeds[k] for k in active])
        else:
            tables = [mixtures(u, g) for u, g in zip(engine.units, engine.gaps())]
            engine.set_mixtures([t[0] for t in tables], [t[1] for t in tables])
        engine.run_pass2()
        res = engine.results(2, fields=("unit_stats",))
        for k, r in zip(active, res):
            search[k].decide(r["cnt_unassigned"])
        rounds += 1
        solves += len(active)
    return InferredOrder([s.dag for s in search], [s.log for s in search], rounds, solves, viol if use_bound else None)
