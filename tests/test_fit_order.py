"""The refit's order tables (fit_row in csrc/tw_fit.h; fit_order and fit_run in csrc/tw_engine.hip).

TW_FIT_ORDER=1 (the default): every launch of the refit hands its fits out longest first, through a permutation of its grid that
the host builds from the rows' distinct-value counts; TW_FIT_ORDER=0: in grid order.  A workgroup is one whole fit, a pure function
of (samples in request order, tape), so which workgroup makes it cannot show in the result: the tables are checked against their
definition, the mixtures and pass 2's parents bit for bit between the two orders.  The tables are built from the host's copy of the
rows' distinct-value counts, which the hash route and the sort route of fit_prepare each fetch in their own way: rows on either side of
the run cache (4 096 runs in LDS, the rest read from global memory) and of the hash table's limit (12 288 distinct values, beyond it the
batch takes the sort route) are fitted in both orders and against the restatement (oracle/tw_refit.py)."""
import numpy as np
import pytest

import parity
from test_fit import check_fit, close, degenerate
from test_fit_spec import FROZEN, ROW, STRESS, STRESS_GPU, _Env, assert_same, frozen_units, refit_rows, run_route
from traceweaver_amd.engine import Engine
from traceweaver_amd.predictor import reference_fit_order

K = 5   # kMaxComp


# ---- 1. the tables ---------------------------------------------------------------------------------------------------

def expected_tables(uniq, n):
    """The definition (include/traceweaver_amd.h, tw_get_fit_order), written out: block (5 - k) * S + q serves slot q at count k and
    is live if the row has samples and k <= #distinct; live blocks by #distinct x k descending, then k descending, then slot
    ascending; the others behind them in index order."""
    S = len(uniq)

    def table(blocks, key_of):
        keyed = [(key_of(b), b) for b in range(blocks)]
        live = sorted([(-key, b) for key, b in keyed if key >= 0])   # (b grows with falling k, then with q: the stated tie order)
        return np.array([b for _, b in live] + [b for key, b in keyed if key < 0], dtype=np.int32)

    def sel_key(b):
        q, k = b % S, K - b // S
        return int(uniq[q]) * k if n[q] > 0 and k <= uniq[q] else -1

    def row_key(q):
        k = min(int(uniq[q]), K) if n[q] > 0 else 0
        return int(uniq[q]) * k if k >= 1 else -1

    return table(4 * S, sel_key), table(5 * S, sel_key), table(S, row_key)


def fitted_tables(lib_path, units, order):
    with _Env(TW_FIT_ORDER=str(order)):
        eng = Engine(0, lib_path=lib_path)
    try:
        eng.load(units)
        eng.run_pass1()
        gaps = eng.gaps()
        eng.fit_mixtures(seed=5)
        tabs = eng.fit_order()
        mixes = eng.mixtures()
        eng.set_mixtures([m for m, _ in mixes], [p for _, p in mixes])
        assert eng.fit_order() is None   # (mixtures that were set come from no refit)
    finally:
        eng.close()
    uniq, n = [], []
    for u, g in zip(units, gaps):
        scored = set(int(q) for q in reference_fit_order(u, u.key_rank))
        for q in range(u.nslot):
            x = g[q][~np.isnan(g[q])] if q in scored else np.zeros(0)
            uniq.append(len(np.unique(x)))
            n.append(len(x))
    return tabs, np.array(uniq), np.array(n)


def check_tables(lib_path, units):
    tabs, uniq, n = fitted_tables(lib_path, units, 1)
    assert tabs is not None
    S = len(uniq)
    assert (n > 0).sum() >= 10 and len(set(uniq[n > 0])) >= 5 and (n == 0).any()   # rows of several lengths, and slots without a fit
    for got, want, blocks in zip(tabs, expected_tables(uniq, n), (4 * S, 5 * S, S)):
        assert np.array_equal(np.sort(got), np.arange(blocks))   # a permutation of the grid
        assert np.array_equal(got, want)
    # written out once more for the EM table: live blocks first with non-increasing keys, dead ones behind them in index order
    em = tabs[1].astype(np.int64)
    q, k = em % S, K - em // S
    live = (n[q] > 0) & (k <= uniq[q])
    first_dead = int(live.sum())
    assert live[:first_dead].all() and not live[first_dead:].any()
    keys = (uniq[q] * k)[:first_dead]
    assert (np.diff(keys) <= 0).all() and (np.diff(em[first_dead:]) > 0).all()
    again, _, _ = fitted_tables(lib_path, units, 1)
    for a, b in zip(tabs, again):
        assert np.array_equal(a, b)
    assert fitted_tables(lib_path, units, 0)[0] is None


def test_tables_are_the_stated_permutations(emu_lib):
    check_tables(emu_lib, parity.stress_units(STRESS)[0] + frozen_units(FROZEN))


@pytest.mark.gpu
def test_tables_are_the_stated_permutations_on_gpu():
    """The knob is honoured by the real library too: tables under 1 -- the bit-equality below compares an ordered run --, none under 0."""
    check_tables(None, parity.stress_units(STRESS_GPU)[0] + frozen_units(FROZEN))


# ---- 2. the same bits in either order --------------------------------------------------------------------------------

def check_orders(lib_path, units, spec, routes=("seed", "tape", "twice")):
    for route in routes:
        with _Env(TW_FIT_ORDER="0"):
            off = run_route(lib_path, units, spec, route)
        with _Env(TW_FIT_ORDER="1"):
            on = run_route(lib_path, units, spec, route)
        assert_same(off, on)
        assert off[0] and off[1] is not None
        assert off[2] == on[2], (route, off[2], on[2])   # hits and misses of the speculative fit
        assert (sum(on[2]) > 0) == (spec == 1), (route, on[2])


@pytest.mark.parametrize("spec", [1, 0])
def test_both_orders_give_the_same_bits(emu_lib, spec):
    check_orders(emu_lib, parity.stress_units(STRESS)[0] + frozen_units(FROZEN), spec)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [1, 0])
def test_both_orders_give_the_same_bits_on_gpu(spec):
    check_orders(None, parity.stress_units(STRESS_GPU)[0] + frozen_units(FROZEN), spec)


# ---- 3. rows around the run cache and the hash table's limit ---------------------------------------------------------

RUN_CACHE, HASH_MAX = 4096, 12288   # kRunCache, kHashMax of the production build (csrc/tw_fit.h)
ROW_POOLS = [("short", 1500, 1000, RUN_CACHE), ("beyond the run cache", 9000, RUN_CACHE + 1, HASH_MAX), ("beyond the hash table", 60000, HASH_MAX + 1, 20000)]


def cache_rows(n, pools):
    """One row of n integer samples per pool, drawn evenly from `values` distinct values: a dense lump and a sparse tail."""
    rng = np.random.RandomState(23)
    rows = []
    for name, values, lo, hi in pools:
        pool = np.cumsum(np.where(np.arange(values) < values * 6 // 10, 1, 1 + rng.randint(0, 40, values))).astype(np.float64)
        rows.append((name, pool[rng.randint(0, values, n)]))
    return rows


def check_cache_rows(lib_path, pools, seed=5):
    import tw_refit as R

    units, _ = parity.stress_units([(71, 20000, "chain3", 2, 1)])
    u = units[0]
    rows = cache_rows(u.n_in, pools)
    for (name, _, lo, hi), (_, x) in zip(pools, rows):
        assert lo <= len(np.unique(x)) <= hi, (name, len(np.unique(x)))
    with _Env(TW_FIT_ORDER="0"):
        off = refit_rows(lib_path, [(u, rows)], 1, seed)
    with _Env(TW_FIT_ORDER="1"):
        on = refit_rows(lib_path, [(u, rows)], 1, seed)
    assert_same(off, on)
    assert off[2] == on[2] and sum(on[2]) == len(rows)
    tape = np.random.RandomState(seed).random_sample(u.nslot * ROW[5])
    mn, mp = on[0][0]
    for q, (name, x) in zip(reference_fit_order(u, u.key_rank), rows):
        n, p = R.fit_edge(x, tape[q * ROW[5]:])
        print("%s: %d distinct values, %d components" % (name, len(np.unique(x)), n))
        assert not degenerate(p, n) and not degenerate(mp[q], int(mn[q])), name   # (thousands of distinct values a component)
        assert mn[q] == n, (name, int(mn[q]), n)
        assert close(mp[q], p, n, 1e-9), name   # check_fit's tolerance (tests/test_fit.py)


@pytest.fixture(scope="module")
def emu_prod_lib(emu_lib):
    """The host emulation with the table sizes of the HIP build (emu_lib: its environment)."""
    from tests.hostemu.build_emu import build

    return build(production=True)


def test_rows_around_the_limits_sort_route(emu_prod_lib):
    check_cache_rows(emu_prod_lib, ROW_POOLS)   # the third row refuses the hash table: the batch takes the sort route


def test_rows_around_the_limits_hash_route(emu_prod_lib):
    check_cache_rows(emu_prod_lib, ROW_POOLS[:2])


@pytest.mark.gpu
@pytest.mark.parametrize("pools", [ROW_POOLS, ROW_POOLS[:2]], ids=["sort route", "hash route"])
def test_rows_around_the_limits_on_gpu(pools):
    check_cache_rows(None, pools)


@pytest.mark.gpu
def test_rows_of_pass_1_beyond_the_run_cache_on_gpu():
    """40 000 requests of the par2 shape at concurrency 1.6 (the unit of test_fit_spec's test_rows_beyond_the_run_cache_on_gpu, which
    asserts its rows of ~6 200 distinct values): rows from pass 1 itself, against the restatement and in both orders."""
    units, _ = parity.stress_units([(64, 40000, "par2", 1.6, 1)])
    assert check_fit(None, units) >= 2
    check_orders(None, units, 1, routes=("seed",))
