"""The call-order DAG from timestamps alone (csrc/tw_order.h, traceweaver_amd/order.py): the necessary-condition table against
its numpy restatement (host-emulation build on the CPU, the HIP build under -m gpu), the staged load against a plain load, and
the batched search against the same loop around the CPU oracle -- the yardstick is the oracle loop, not the true DAG."""
import numpy as np
import pytest

import parity
from traceweaver_amd import order, synth
from traceweaver_amd.engine import Engine, EngineError, UnitArrays

TW_ERR_ARG, TW_ERR_UNSUPPORTED = -1, -2

# (seed, n_in, shape, concurrency) of the search tests.  The seeds were chosen with the oracle loop alone (on the CPU) so that
# the conditions of test_oracle_loop_conditions hold: a unit with both a kept and a rejected solved candidate (the last one), a
# pair rejected by the bound (par2), and at concurrency <= 2 the graph FindOrder gives.
SEARCH = [(1, 120, "chain3", 1.5), (2, 120, "par2", 2), (5, 100, "diamond", 2), (5, 100, "chain3", 4)]
SEARCH_IDS = ["chain3-c1.5", "par2-c2", "diamond-c2", "chain3-c4"]


def search_units():
    return [synth.make_unit(seed, n, shape=shape, concurrency=conc)[0] for seed, n, shape, conc in SEARCH]


def oracle_solve(unit):
    return parity.oracle_two_pass(parity.oracle_service(unit))[2]["cnt_unassigned"]


def det_mixtures(unit, gaps):
    """parity.deterministic_mixture over the gap rows of a unit: the tables parity.oracle_two_pass builds for the oracle."""
    mix_n = np.zeros(unit.nslot, np.int32)
    mix_p = np.zeros((unit.nslot, 5, 3))
    for q, row in enumerate(gaps):
        d = row[~np.isnan(row)]
        if len(d):
            mix_n[q], mix_p[q] = parity.deterministic_mixture(d)
    return mix_n, mix_p


_ORACLE = {}


def oracle_loop(use_bound=True):
    """The host loop around the oracle for the four search units: computed once, shared, never changed."""
    if use_bound not in _ORACLE:
        _ORACLE[use_bound] = order.infer_order_host(search_units(), oracle_solve, use_bound=use_bound)
    return _ORACLE[use_bound]


# ---------------------------------------------------------------------------------------------------------------------------
# inputs of the bound


def shortened_unit():
    """chain3 at low interleaving with five spans of endpoint 1 taken out: the requests that made them contain none of its spans."""
    u, _ = synth.make_unit(31, 80, shape="chain3", concurrency=1.1)
    keep = np.ones(u.n_in, dtype=bool)
    keep[20:25] = False
    seg = lambda a, e: a[u.out_off[e]:u.out_off[e + 1]]
    starts = [seg(u.out_start, 0), seg(u.out_start, 1)[keep], seg(u.out_start, 2)]
    ends = [seg(u.out_end, 0), seg(u.out_end, 1)[keep], seg(u.out_end, 2)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in starts])])
    return UnitArrays(u.in_start, u.in_end, off, np.concatenate(starts), np.concatenate(ends), u.dag)


def bound_cases():
    mk = lambda seed, n, shape, conc, gran=1: synth.make_unit(seed, n, shape=shape, concurrency=conc, granularity_us=gran)[0]
    cases = [("n%d" % n, [mk(40 + n, n, "chain3", 3)]) for n in (1, 64, 65, 257)]   # wavefront edges
    cases.append(("E1", [mk(51, 50, "single", 2)]))                                  # an empty table
    cases.append(("E8", [mk(52, 100, "mix8", 1.3)]))
    cases.append(("ms-granular", [mk(53, 150, "chain3", 4, 1000)]))                   # end == start counts as ordered
    cases.append(("shortened", [shortened_unit()]))
    cases.append(("three-units", [mk(54, 70, "par2", 2), mk(55, 130, "mix7", 1.5), mk(56, 65, "single", 3)]))   # offsets
    return cases


BOUND_CASES = bound_cases()


def check_bound(eng, units):
    got, want = eng.order_bound(units), order.order_bound_host(units)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int64 and g.shape == (units[k].E, units[k].E)
        assert np.array_equal(g, w), "unit %d:\n%s\n%s" % (k, g, w)
    return want


def check_bound_properties(name, units, want):
    if name == "E1":
        assert want[0].shape == (1, 1) and want[0][0, 0] == 0
    if name == "ms-granular":   # the true order holds with end == start in some request, and is not violated
        u = units[0]
        assert (u.out_end[u.out_off[0]:u.out_off[1]][:, None] == u.out_start[u.out_off[1]:u.out_off[2]][None, :]).any()
        assert want[0][0, 1] == 0 and want[0][1, 2] == 0 and want[0][0, 2] == 0
    if name == "shortened":     # every pair with the shortened endpoint is violated in the requests that hold none of its spans
        assert (want[0][1, [0, 2]] >= 5).all() and (want[0][[0, 2], 1] >= 5).all() and want[0][0, 2] == 0
    if name == "E8":            # lightly interleaved: the table is FindOrder's relation
        assert np.array_equal(want[0] == 0, (units[0].dag | np.eye(8, dtype=np.uint8)).astype(bool))


def check_unsorted(eng):
    u, _ = synth.make_unit(57, 40, shape="chain2", concurrency=2)
    eng.order_bound([u])
    out_start, in_start = u.out_start.copy(), u.in_start.copy()
    out_start[[45, 46]] = out_start[[46, 45]]   # two spans of endpoint 1 swapped
    in_start[[5, 6]] = in_start[[6, 5]]
    assert out_start[45] > out_start[46] and in_start[5] > in_start[6]
    for bad in (UnitArrays(u.in_start, u.in_end, u.out_off, out_start, u.out_end, u.dag),
                UnitArrays(in_start, u.in_end, u.out_off, u.out_start, u.out_end, u.dag)):
        with pytest.raises(EngineError) as ex:
            eng.order_bound([bad])
        assert ex.value.code == TW_ERR_ARG
    wide = UnitArrays(u.in_start, u.in_end, np.arange(10, dtype=np.int64) * 0, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((9, 9), np.uint8))
    with pytest.raises(EngineError) as ex:
        eng.order_bound([wide])
    assert ex.value.code == TW_ERR_UNSUPPORTED


def check_refusals(eng):
    u, _ = synth.make_unit(58, 40, shape="chain2", concurrency=2)
    eng.order_stage([u])
    refused = {
        "skip mode": lambda: eng.order_stage([u], skip=[None]),
        "short endpoint": lambda: eng.order_stage([shortened_unit()]),
        "load-scaled": lambda: eng.order_stage([UnitArrays(u.in_start, u.in_end, u.out_off, u.out_start, u.out_end, u.dag, time_scale=0.125)]),
        "split service": lambda: eng.order_stage([UnitArrays(u.in_start, u.in_end, u.out_off, u.out_start, u.out_end, u.dag, part=UnitArrays.AFTER_CUT)]),
        "E = 9": lambda: eng.order_stage([UnitArrays(u.in_start, u.in_end, np.arange(10, dtype=np.int64) * u.n_in, np.tile(u.out_start[:u.n_in], 9),
                                                     np.tile(u.out_end[:u.n_in], 9), np.zeros((9, 9), np.uint8))]),
    }
    for name, call in refused.items():
        with pytest.raises(EngineError) as ex:
            call()
        assert ex.value.code == TW_ERR_UNSUPPORTED, name
    cyc = np.zeros((2, 2), np.uint8)
    cyc[0, 1] = cyc[1, 0] = 1
    eng.order_stage([u])
    with pytest.raises(EngineError) as ex:
        eng.order_load([0], [cyc])
    assert ex.value.code == TW_ERR_ARG


def two_pass(eng, units):
    """parity.check_units' engine side on a batch that is already loaded."""
    eng.run_pass1()
    r1, gaps, gauss = eng.results(1), eng.gaps(), eng.gauss_params()
    tables = [det_mixtures(u, g) for u, g in zip(units, gaps)]
    eng.set_mixtures([t[0] for t in tables], [t[1] for t in tables])
    eng.run_pass2()
    return r1, gaps, gauss, eng.results(2)


def assert_same_results(a, b):
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for p, q in zip(x, y):
            if isinstance(p, dict):
                assert sorted(p) == sorted(q)
                for key in p:
                    assert np.array_equal(p[key], q[key], equal_nan=isinstance(p[key], np.ndarray) and p[key].dtype.kind == "f"), key
            else:
                assert np.array_equal(p, q, equal_nan=True)


def check_order_load(lib_path):
    """After order_load the two-pass results equal those of a plain load of the same permuted units -- on a graph whose
    topological order is not the key order, and on a subset of the staged units."""
    units = [synth.make_unit(61, 90, shape="chain3", concurrency=2)[0], synth.make_unit(62, 70, shape="par2", concurrency=2)[0],
             synth.make_unit(63, 80, shape="diamond", concurrency=1.5)[0]]
    rev = lambda u: UnitArrays(u.in_start, u.in_end, u.out_off, np.concatenate([u.out_start[u.out_off[e]:u.out_off[e + 1]] for e in range(u.E)[::-1]]),
                               np.concatenate([u.out_end[u.out_off[e]:u.out_off[e + 1]] for e in range(u.E)[::-1]]), u.dag)
    staged = [rev(units[0]), units[1], rev(units[2])]   # key order = the reverse of the call order for units 0 and 2
    dags = [units[0].dag[::-1, ::-1].copy(), np.zeros((2, 2), np.uint8), units[2].dag[::-1, ::-1].copy()]
    dags[0][2, 0] = 0                                   # (not transitively closed: 2 -> 1 -> 0 only)
    eng = Engine(0, lib_path=lib_path)
    eng.order_stage(staged)
    out = []
    for active in ([0, 1, 2], [0, 2]):
        want_units = [order.permuted_unit(staged[k], dags[k]) for k in active]
        assert [u.key_rank.tolist() for u in want_units][0] == [2, 1, 0]
        eng.order_load(active, [dags[k] for k in active])
        for u, w in zip(eng.units, want_units):
            for name in ("in_start", "in_end", "out_off", "out_start", "out_end", "dag", "key_rank"):
                assert np.array_equal(getattr(u, name), getattr(w, name)), name
        got = two_pass(eng, want_units)
        eng.load(want_units)
        assert_same_results(got, two_pass(eng, want_units))
        out.append(got)
    eng.close()
    assert out[0][3][0]["cnt_unassigned"] == out[1][3][0]["cnt_unassigned"]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU tier


@pytest.fixture
def emu_engine(emu_lib, monkeypatch):
    # one host thread per lane, workgroups of 256 for the flat kernels: the ballots of k_order_bound run as they are written
    monkeypatch.setenv("TW_EMU_LANES", "1")
    monkeypatch.setenv("TW_COOP_THREADS", "64")
    eng = Engine(0, lib_path=emu_lib)
    yield eng
    eng.close()


@pytest.mark.parametrize("name,units", BOUND_CASES, ids=[c[0] for c in BOUND_CASES])
def test_bound_equals_restatement_emu(emu_engine, name, units):
    check_bound_properties(name, units, check_bound(emu_engine, units))


def test_bound_refuses_unsorted_lists_emu(emu_engine):
    check_unsorted(emu_engine)


def test_stage_refusals_emu(emu_engine):
    check_refusals(emu_engine)


def test_order_load_equals_plain_load_emu(emu_lib):
    check_order_load(emu_lib)


def test_topological_order_is_networkx(oracle):
    """order.topological_order against nx.topological_sort on every graph the search can reach for E <= 4 (edges added in pair
    order), and on random acyclic subsets of the pairs for E = 8."""
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(7)
    n_checked = 0
    for E, trials in ((1, 1), (2, 4), (3, 64), (4, 400), (8, 300)):
        pairs = order.ordered_pairs(E)
        for t in range(trials):
            pick = [(t >> j) & 1 for j in range(len(pairs))] if E <= 3 else (rng.random(len(pairs)) < rng.choice([0.15, 0.3, 0.5])).tolist()
            g = nx.DiGraph()
            g.add_nodes_from(range(E))
            dag = np.zeros((E, E), np.uint8)
            for (a, b), on in zip(pairs, pick):
                if on and not g.has_edge(b, a) and not nx.has_path(g, b, a):
                    g.add_edge(a, b)
                    dag[a, b] = 1
            assert order.topological_order(dag) == list(nx.topological_sort(g))
            n_checked += 1
    assert n_checked > 700
    with pytest.raises(ValueError):
        order.topological_order(np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], np.uint8))


def test_oracle_loop_conditions(oracle):
    """What the four search inputs must show, checked with the oracle alone."""
    r, units = oracle_loop(), search_units()
    kept = lambda log: [x for x in log if x[2] == "solve" and x[3] <= 0]
    rejected = lambda log: [x for x in log if x[2] == "solve" and x[3] > 0]
    assert any(kept(log) and rejected(log) for log in r.logs)
    assert any(x[2] == "bound" for log in r.logs for x in log)
    for k, (_, _, _, conc) in enumerate(SEARCH):
        if conc <= 2:   # make_unit hands the unit over in FindOrder's own topological order: its dag is in key order here
            assert np.array_equal(r.dags[k], units[k].dag), SEARCH_IDS[k]
    for k, log in enumerate(r.logs):
        assert [(a, b) for a, b, _, _ in log] == order.ordered_pairs(units[k].E)
        assert all(how in order.DECIDED_BY for _, _, how, _ in log)
        dag = np.zeros_like(r.dags[k])
        for a, b, _, _ in kept(log):
            dag[a, b] = 1
        assert np.array_equal(dag, r.dags[k])
    assert r.solves == sum(len(kept(log)) + len(rejected(log)) for log in r.logs) and r.rounds <= 12
    nobound = oracle_loop(use_bound=False)
    assert all(np.array_equal(a, b) for a, b in zip(r.dags, nobound.dags))
    assert nobound.solves > r.solves


def test_search_equals_oracle_loop_emu(emu_lib):
    """The batched search on the host-emulation build for the two lightest inputs (the whole set runs under -m gpu)."""
    units = search_units()[:2]
    eng = Engine(0, lib_path=emu_lib)
    got = order.infer_order(eng, units, mixtures=det_mixtures)
    eng.close()
    want = oracle_loop()
    assert got.logs == want.logs[:2]
    assert all(np.array_equal(a, b) for a, b in zip(got.dags, want.dags[:2]))


def test_executor_infer_order_flag(emu_lib, tmp_path, capsys):
    """--infer_order 1 on a lightly loaded hotel-shaped corpus: both services get FindOrder's graph from their spans alone, and
    the run's figures are those of the run that reads the graph from the true assignments; refused with cache hits / load scaling."""
    from traceweaver_amd import executor

    synth.write_jaeger_corpus(str(tmp_path / "data" / "app"), 5, 60, app=synth.HOTEL_APP, concurrency=1.3)
    argv = lambda cache="0", *more: ["--relative_path", "data/app/", "--cache_rate", cache, "--fix", "2", "--results_directory", str(tmp_path / "out") + "/",
                                     "--project_root", str(tmp_path), "--engine_library", emu_lib, "--fit", "device-batch", "--clear_cache", "1"] + list(more)
    plain = executor.run(executor.parse_args(argv()))
    capsys.readouterr()
    inferred = executor.run(executor.parse_args(argv("0", "--infer_order", "1")))
    text = capsys.readouterr().out
    assert "Call graph of service frontend: identical to FindOrder's (3 edges" in text
    assert "Call graph of service search: identical to FindOrder's (1 edges" in text
    assert "Inferred call graphs identical to FindOrder's: 2 of 2" in text
    assert inferred == plain
    assert not executor.unsupported(executor.parse_args(argv("0", "--infer_order", "1")))
    for refused in (argv("0.1", "--infer_order", "1"), argv("0", "--infer_order", "1", "--compress_factor", "2")):
        assert any("--infer_order" in p for p in executor.unsupported(executor.parse_args(refused)))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU tier


@pytest.fixture
def gpu_engine():
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,units", BOUND_CASES, ids=[c[0] for c in BOUND_CASES])
def test_bound_equals_restatement(gpu_engine, name, units):
    check_bound_properties(name, units, check_bound(gpu_engine, units))


@pytest.mark.gpu
def test_bound_refuses_unsorted_lists(gpu_engine):
    check_unsorted(gpu_engine)


@pytest.mark.gpu
def test_stage_refusals(gpu_engine):
    check_refusals(gpu_engine)


@pytest.mark.gpu
def test_order_load_equals_plain_load():
    check_order_load(None)


@pytest.mark.gpu
def test_search_equals_oracle_loop(gpu_engine, oracle):
    """infer_order with the deterministic tables == infer_order_host around parity.oracle_two_pass: the same log entry for
    entry, every cnt_unassigned equal, and the same DAG, for the four inputs in one batch."""
    got = order.infer_order(gpu_engine, search_units(), mixtures=det_mixtures)
    want = oracle_loop()
    for k, name in enumerate(SEARCH_IDS):
        assert got.logs[k] == want.logs[k], name
        assert np.array_equal(got.dags[k], want.dags[k]), name
    assert got.solves == want.solves and got.rounds == want.rounds and got.rounds <= 12


@pytest.mark.gpu
def test_bound_only_saves_solves(gpu_engine, oracle):
    units = search_units()
    with_bound = order.infer_order(gpu_engine, units, mixtures=det_mixtures, use_bound=True)
    without = order.infer_order(gpu_engine, units, mixtures=det_mixtures, use_bound=False)
    for k, name in enumerate(SEARCH_IDS):
        assert np.array_equal(with_bound.dags[k], without.dags[k]), name
    par2 = SEARCH_IDS.index("par2-c2")
    solves = lambda r, k: sum(1 for x in r.logs[k] if x[2] == "solve")
    assert solves(with_bound, par2) < solves(without, par2)
    assert np.array_equal(without.dags[par2], oracle_loop(use_bound=False).dags[par2])


@pytest.mark.gpu
def test_batched_search_equals_unit_by_unit(gpu_engine):
    """The default refit, one seed per unit: the four units in one batch give the DAGs and logs each unit gives alone."""
    units, seeds = search_units(), [11, 12, 13, 14]
    together = order.infer_order(gpu_engine, units, seeds=seeds)
    for k, name in enumerate(SEARCH_IDS):
        alone = order.infer_order(gpu_engine, [units[k]], seeds=[seeds[k]])
        assert alone.logs[0] == together.logs[k], name
        assert np.array_equal(alone.dags[0], together.dags[k]), name
    assert together.rounds == max(sum(1 for x in log if x[2] == "solve") for log in together.logs)


@pytest.mark.gpu
def test_predictor_infers_the_graph_when_none_is_given():
    """TraceWeaverGPU.FindAssignments(..., invocation_graph=None) == the same call with the graph infer_order finds."""
    nx = pytest.importorskip("networkx")
    from traceweaver_amd.predictor import TraceWeaverGPU

    class Span(object):
        def __init__(self, sid, start, end):
            self.sid, self.start_mus, self.duration_mus = sid, int(start), int(end - start)

        def GetId(self):
            return ("t", self.sid)

    u, tp = synth.make_unit(1, 120, shape="chain3", concurrency=1.5)
    names = ["c", "b", "a"]   # key order = the reverse of the call order
    ins = {"in": [Span("i%d" % i, u.in_start[i], u.in_end[i]) for i in range(u.n_in)]}
    outs = {names[e]: [Span("%s%d" % (names[e], x), u.out_start[u.out_off[2 - e] + x], u.out_end[u.out_off[2 - e] + x]) for x in range(u.n_in)] for e in range(3)}
    truth = {names[e]: {("t", "i%d" % i): ("t", "%s%d" % (names[e], tp[2 - e, i])) for i in range(u.n_in)} for e in range(3)}
    pred = TraceWeaverGPU({}, {}, replay_true_fit=False)
    np.random.seed(3)
    inferred = pred.FindAssignments("m", "svc", ins, outs, False, False, truth)
    g = pred.last_order.graph(0, names)
    assert sorted(g.edges()) == [("a", "b"), ("a", "c"), ("b", "c")]
    np.random.seed(3)
    given = pred.FindAssignments("m", "svc", ins, outs, False, False, truth, g)
    pred._engine.close()
    assert inferred[0] == given[0] and inferred[2:4] == given[2:4] and inferred[5] == given[5]
    right = sum(inferred[0][ep][k] == v for ep in names for k, v in truth[ep].items())
    assert right >= 0.9 * 3 * u.n_in
