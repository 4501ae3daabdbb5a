"""The speculative final fit of the refit (csrc/tw_fit.h, fit_run in csrc/tw_engine.hip): the final fit of the largest admissible
count min(5, #distinct) runs beside the model selection and is adopted by the rows that select that count (TW_FIT_SPEC=1, the
default); TW_FIT_SPEC=0 fits every row after the selection.  Every fit is one workgroup computing the same function of (samples in
request order, tape) either way, so the two routes must agree bit for bit: counts, every parameter double, pass 2's parents."""
import glob
import os

import numpy as np
import pytest

import parity
from conftest import REPO, unit_from_golden
from traceweaver_amd.engine import Engine
from traceweaver_amd.predictor import reference_fit_order

ROW = Engine.FIT_ROW_DRAWS
STRESS = [(31, 600, "chain3", 2, 1), (32, 500, "par2", 3, 1000), (33, 400, "single", 1.5, 1)]          # test_device_fit_matches_the_restatement
STRESS_GPU = [(31, 6000, "chain3", 2, 1), (32, 5000, "par2", 3, 1000), (33, 40000, "single", 1.5, 1), (34, 3000, "diamond", 2, 1)]   # test_device_fit_on_gpu
# frozen services (970-1 000 samples a row): on some rows BIC selects the largest count, on others a smaller one
FROZEN = ["hotel_load100__frontend", "media_load100__text-service", "nodeio_1__service1"]


class _Env(object):
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def frozen_units(names):
    paths = [p for p in sorted(glob.glob(os.path.join(REPO, "tests", "golden", "ref_*.npz"))) if any(k in p for k in names)]
    assert len(paths) == len(names)
    return [unit_from_golden(np.load(p))[1] for p in paths]


def run_route(lib_path, units, spec, route, pass2=True):
    """One engine under TW_FIT_SPEC=spec (the knob is read when the engine is created).  route: "seed" (the engine's own MT19937),
    "tape" (the caller's uniforms), "twice" (a refit, other gap rows, a second refit on the same engine: what is returned is the
    second), "second" (the second refit of "twice" alone, on a fresh engine).  Returns (mixtures, parents of pass 2, (hits, misses))."""
    with _Env(TW_FIT_SPEC=str(spec)):
        eng = Engine(0, lib_path=lib_path)
    try:
        eng.load(units)
        eng.run_pass1()
        assert eng.fit_spec() == (0, 0)
        if route == "tape":
            offs, pos = [], 0
            for u, m in zip(units, eng.fit_rows()):
                o = np.zeros(u.nslot, dtype=np.int64)
                for q in range(u.nslot):
                    o[q] = pos
                    pos += ROW[int(m[q])]
                offs.append(o)
            eng.fit_mixtures(tape=np.random.RandomState(11).random_sample(pos), slot_off=offs)
        else:
            if route in ("twice", "second"):
                # the second refit's rows: every unit's scored rows in reverse order, so that a row sits where a row of another
                # outcome sat in the first refit (a stale speculative result or failed flag would show)
                other = []
                for u, g in zip(units, eng.gaps()):
                    sc = reference_fit_order(u, u.key_rank)
                    h = g.copy()
                    h[sc] = g[sc[::-1]]
                    other.append(h)
                if route == "twice":
                    eng.fit_mixtures(seed=5)
                eng.set_gaps(other)
            eng.fit_mixtures(seed=5)
        counts = eng.fit_spec()
        mixes = [(n.copy(), p.copy()) for n, p in eng.mixtures()]
        parents = None
        if pass2:
            eng.run_pass2()
            parents = [r["parent"].copy() for r in eng.results(2, fields=("parent",))]
    finally:
        eng.close()
    return mixes, parents, counts


def assert_same(a, b):
    (ma, pa, _), (mb, pb, _) = a, b
    for (na, xa), (nb, xb) in zip(ma, mb):
        assert np.array_equal(na, nb)
        assert np.array_equal(xa, xb)   # every parameter double, no tolerance
    if pa is not None:
        for x, y in zip(pa, pb):
            assert np.array_equal(x, y)


def check_routes(lib_path, units, routes=("seed", "tape", "twice"), need_miss=True):
    """need_miss=False: a batch of long rows only, on which BIC selects the largest count everywhere."""
    for route in routes:
        off = run_route(lib_path, units, 0, route)
        on = run_route(lib_path, units, 1, route)
        assert_same(off, on)
        assert off[2] == (0, 0), route
        hits, misses = on[2]
        print("route %s: %d hits, %d misses" % (route, hits, misses))
        assert hits >= 1 and (misses >= 1 or not need_miss), (route, hits, misses)
        assert hits + misses == sum(int((n > 0).sum()) for n, _ in on[0]), route
        if route == "twice":
            assert_same(on, run_route(lib_path, units, 1, "second"))


def test_both_routes_give_the_same_bits(emu_lib):
    units, _ = parity.stress_units(STRESS)
    check_routes(emu_lib, units + frozen_units(FROZEN))


# ---- row shapes ------------------------------------------------------------------------------------------------------

def shaped_rows(n, rng):
    """Six rows of n entries (NaN = no sample), integer microseconds: (name, row)."""
    two = np.round(np.where(rng.random_sample(n) < 0.5, rng.normal(1000.0, 30.0, n), rng.normal(9000.0, 50.0, n)))   # two well-separated Gaussians: BIC selects 2
    dropped = np.round(rng.gamma(3.0, 400.0, n))
    dropped[rng.random_sample(n) < 0.3] = np.nan
    return [("one value", np.full(n, 700.0)),
            ("three values", rng.choice([100.0, 5000.0, 90000.0], n)),
            ("dropped samples", dropped),
            ("no samples", np.full(n, np.nan)),
            ("two components", two),
            ("many values", np.round(rng.lognormal(7.0, 0.8, n)))]


def refit_rows(lib_path, unit_rows, spec, seed=5):
    """Loads the units, replaces their scored gap rows by the given ones (set_gaps: no pass is needed for a refit) and fits."""
    units = [u for u, _ in unit_rows]
    with _Env(TW_FIT_SPEC=str(spec)):
        eng = Engine(0, lib_path=lib_path)
    try:
        eng.load(units)
        gaps = []
        for u, rows in unit_rows:
            g = np.full((u.nslot, u.n_in), np.nan)
            sc = reference_fit_order(u, u.key_rank)
            assert len(rows) <= len(sc)
            for q, (_, x) in zip(sc, rows):
                g[q] = x
            gaps.append(g)
        eng.set_gaps(gaps)
        eng.fit_mixtures(seed=seed)
        return [(n.copy(), p.copy()) for n, p in eng.mixtures()], None, eng.fit_spec()
    finally:
        eng.close()


def check_row_shapes(lib_path, seed=5):
    import tw_refit as R
    from test_fit import close, degenerate

    units, _ = parity.stress_units([(61, 1500, "chain3", 2, 1), (62, 20000, "single", 1.5, 1)])
    rng = np.random.RandomState(17)
    long_row = np.round(rng.lognormal(9.0, 1.0, units[1].n_in))   # 20 000 samples, more than 4 096 distinct values: past the run cache
    assert len(np.unique(long_row)) > 4096
    unit_rows = [(units[0], shaped_rows(units[0].n_in, rng)), (units[1], [("long row", long_row)])]
    off = refit_rows(lib_path, unit_rows, 0, seed)
    on = refit_rows(lib_path, unit_rows, 1, seed)
    assert_same(off, on)
    assert off[2] == (0, 0)
    tape = np.random.RandomState(seed).random_sample(sum(u.nslot for u in units) * ROW[5])
    base, hits, got = 0, 0, {}
    for (u, rows), (mn, mp) in zip(unit_rows, on[0]):
        sc = reference_fit_order(u, u.key_rank)
        for q in range(u.nslot):
            if q not in sc[:len(rows)]:
                assert mn[q] == 0
        for q, (name, row) in zip(sc, rows):
            x = row[~np.isnan(row)]
            n, p = R.fit_edge(x, tape[(base + q) * ROW[5]:])
            got[name] = int(mn[q])
            hits += mn[q] > 0 and mn[q] == min(len(np.unique(x)), 5)   # a hit: the row selected the count that was fitted ahead
            if len(x) == 0:
                assert mn[q] == 0
                continue
            if degenerate(p, n) or degenerate(mp[q], int(mn[q])):
                continue
            assert mn[q] == n, (name, int(mn[q]), n)
            assert close(mp[q], p, n, 1e-9), name
        base += u.nslot
    assert got["one value"] == 1 and got["no samples"] == 0 and got["two components"] == 2 and got["three values"] <= 3, got
    live = sum(v > 0 for v in got.values())
    assert on[2][0] + on[2][1] == live and on[2][1] >= 1, (on[2], got)   # ("two components" is a miss by construction)
    assert on[2][0] == hits, (on[2], hits)


def test_row_shapes(emu_lib):
    check_row_shapes(emu_lib)


# ---- a speculative fit that fails ------------------------------------------------------------------------------------

def find_failed_speculative_row(limit=200):
    """Seeded candidate rows -- few distinct values and one far outlier -- for which the full-covariance fit of the largest
    admissible count raises while the model selection picks a smaller count.  Returns (candidate, row) or None."""
    import tw_refit as R

    for c in range(limit):
        rng = np.random.RandomState(1000 + c)
        vals = np.sort(rng.choice(np.arange(1, 40), 2 + c % 4, replace=False)).astype(np.float64) * (10.0 ** (c % 3))
        x = rng.choice(vals, 300 + c)
        x[rng.randint(len(x))] = float(10 ** (6 + c % 4))
        k = min(len(np.unique(x)), 5)
        if R.gmm_fit(x, k, R.refit_tape(k), full=True) is not None:
            continue
        n, _ = R.fit_edge(x, np.random.RandomState(c).random_sample(ROW[5]))
        if n < k:
            return c, x
    return None


def test_failed_speculative_fit_is_no_error(emu_lib):
    """No candidate of the search fails: a full covariance is a sum of squares plus reg_covar in the restatement and cannot end at
    or below zero.  Should a change of the candidates find one, both routes must fit it to the same table without raising."""
    found = find_failed_speculative_row()
    if found is None:
        return
    units, _ = parity.stress_units([(63, 600, "single", 1.5, 1)])
    x = np.resize(found[1], units[0].n_in)
    rows = [(units[0], [("failed speculative fit", x)])]
    assert_same(refit_rows(emu_lib, rows, 0), refit_rows(emu_lib, rows, 1))


# ---- the real library ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_both_routes_give_the_same_bits_on_gpu():
    units, _ = parity.stress_units(STRESS_GPU)
    check_routes(None, units + frozen_units(FROZEN))


@pytest.mark.gpu
def test_rows_beyond_the_run_cache_on_gpu():
    """40 000 requests of the par2 shape at concurrency 1.6: the closing-gap rows hold more distinct values than the run cache."""
    units, _ = parity.stress_units([(64, 40000, "par2", 1.6, 1)])
    eng = Engine(0)
    try:
        eng.load(units)
        eng.run_pass1()
        g = eng.gaps()[0]
    finally:
        eng.close()
    distinct = [len(np.unique(g[q][~np.isnan(g[q])])) for q in reference_fit_order(units[0], units[0].key_rank)]
    print("distinct values of the scored rows:", distinct)
    assert max(distinct) > 4096, distinct   # (kRunCache, csrc/tw_fit.h: the speculative seed and EM kernels read the rest of such a row from global memory)
    check_routes(None, units, need_miss=False)


@pytest.mark.gpu
def test_row_shapes_on_gpu():
    check_row_shapes(None)
