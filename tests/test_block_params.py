"""Pass-1 block parameters by one wavefront per group of blocks of a unit (k_block_params_wave, traceweaver_amd/csrc/tw_kernels.h)
against the thread-per-slot kernel of the same build (TW_BLOCK_PARAMS=0) bit for bit, and against the oracle under the comparison of
tests/parity.py.  Block lengths around every edge of the ten sub-batches and of a lane's second span, every slot layout, load-scaled
units (binary64 sums in order), units of several groups with a short last one, and a batch whose classes alternate, joined and
staged.  CPU tier: the host-emulation build; the same cases on the HIP library under -m gpu."""
import numpy as np
import pytest

import parity
import tw_oracle as T
from traceweaver_amd import synth, transforms
from traceweaver_amd.engine import Engine, EngineError

# batch_size 100: blocks of 1, 7, 9, 10, 11, 50, 64, 99, 100 spans; 1300: 13 blocks, several groups of every group size, the last one short
N_IN = (1, 7, 9, 10, 11, 99, 100, 101, 164, 250, 1001, 1300)
SHAPES = ("single", "par2", "chain2", "chain3", "par4")
ALTERNATING = ("single", "par4", "par2", "single", "par2", "par4")
JOINED, STAGED, UNPIPELINED = {"TW_STAGE_MIN_TILES": "1000000"}, {"TW_STAGE_MIN_TILES": "1"}, {"TW_STAGE_MIN_TILES": "1", "TW_CLASS_PIPELINE": "0"}


def _unit(seed, n_in, shape):
    return synth.make_unit(seed, n_in, shape=shape, concurrency=2.0)


def _pass1(lib, monkeypatch, knob, units, env=None, scale=None, chain=False):
    """(error code, gauss_params() or None, parents after pass 2 or None) of one engine created under TW_BLOCK_PARAMS=knob."""
    monkeypatch.setenv("TW_BLOCK_PARAMS", knob)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    eng = Engine(0, lib_path=lib)
    try:
        try:
            eng.load([u for u, _ in units])
            if scale is not None:
                eng.set_truth([tp for _, tp in units])
                eng.scale_load([scale] * len(units))
            eng.run_pass1()
        except EngineError as ex:
            return ex.code, None, None
        g = eng.gauss_params()
        parents = None
        if chain:
            eng.fit_mixtures()
            eng.run_pass2()
            parents = [r["parent"] for r in eng.results(2, fields=("parent",))]
        return 0, g, parents
    finally:
        eng.close()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True)   # (NaNs in the same places)


def _against_oracle(g_eng, services):
    for k, svc in enumerate(services):   # tests/parity.py:79-83
        g = T.gauss_params(svc)
        m = ~np.isnan(g[..., 0])
        assert np.array_equal(g_eng[k][..., 0][m], g[..., 0][m]), "unit %d: gaussian means" % k
        assert np.array_equal(g_eng[k][..., 1][m], g[..., 1][m]), "unit %d: gaussian stds" % k
        assert np.isnan(g_eng[k][..., 0][~m]).all()


def _check(lib, monkeypatch, units, env=None, scale=None, chain=False, services=None):
    new = _pass1(lib, monkeypatch, "1", units, env, scale, chain)
    old = _pass1(lib, monkeypatch, "0", units, env, scale, chain)
    assert new[0] == old[0]
    if services is None:
        services = [parity.oracle_service(u) for u, _ in units]
    if new[0] != 0:
        # a unit of one request is refused at load; a last block of one request has no variance: the std is NaN and the pass ends with
        # that error, as the reference aborts there -- by both kernels, and where the oracle's std is NaN too
        n_in = {u.n_in for u, _ in units}
        assert (new[0] == -1 and n_in == {1}) or (new[0] == -7 and all(n % 100 == 1 for n in n_in)), new[0]
        if new[0] == -7:
            for svc in services:
                g = T.gauss_params(svc)
                assert np.isnan(g[-1][..., 1][~np.isnan(g[-1][..., 0])]).all() and not np.isnan(g[:-1][..., 1][~np.isnan(g[:-1][..., 0])]).any()
        return
    _same(new[1], old[1])
    _against_oracle(new[1], services)
    if chain:
        _same(new[2], old[2])


def _block_lengths(lib, monkeypatch, n_in):
    if n_in == 1:   # (the generator itself builds requests in flight: a unit of one request is the first of a unit of two)
        u, tp = _unit(31, 2, "par2")
        cut = type(u)(u.in_start[:1], u.in_end[:1], np.arange(u.E + 1, dtype=np.int64), u.out_start[[0, 2]], u.out_end[[0, 2]], u.dag, u.key_rank)
        return _check(lib, monkeypatch, [(cut, tp[:, :1])], services=[])
    more = [_unit(33 + n_in, n_in, "single"), _unit(34 + n_in, n_in, "par4")] if n_in == 1300 else []
    _check(lib, monkeypatch, [_unit(31 + n_in, n_in, "par2"), _unit(32 + n_in, n_in, "chain3")] + more)


def _slot_layouts(lib, monkeypatch):
    units = [_unit(50 + k, 164, s) for k, s in enumerate(SHAPES)]
    wl, truth, _ = synth.make_alibaba_workload(3, 1)   # its smallest size: two requests per service
    eight = [(u, tp) for u, tp in zip(wl, truth) if u.E == 8][:1]
    assert len(eight) == 1 and eight[0][0].n_in == 2
    _check(lib, monkeypatch, units + eight)


def _float_time(lib, monkeypatch):
    units = [_unit(61, 250, "par2"), _unit(62, 164, "chain3")]
    host = [transforms.compress_unit(u, tp, 3).arrays for u, tp in units]
    assert all(h.time_scale is not None for h in host)
    _check(lib, monkeypatch, units, scale=3, services=[parity.oracle_service(h) for h in host])


def _class_tables(lib, monkeypatch, env):
    _check(lib, monkeypatch, [_unit(70 + k, 300, s) for k, s in enumerate(ALTERNATING)], env=env, chain=True)


# ---- CPU tier: the host-emulation build ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in", N_IN)
def test_block_lengths_emulated(emu_lib, monkeypatch, n_in):
    _block_lengths(emu_lib, monkeypatch, n_in)


def test_slot_layouts_emulated(emu_lib, monkeypatch):
    _slot_layouts(emu_lib, monkeypatch)


def test_float_time_emulated(emu_lib, monkeypatch):
    _float_time(emu_lib, monkeypatch)


@pytest.mark.parametrize("env", [JOINED, STAGED, UNPIPELINED], ids=["joined", "staged", "unpipelined"])
def test_class_tables_emulated(emu_lib, monkeypatch, env):
    _class_tables(emu_lib, monkeypatch, env)


# ---- GPU tier --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_in", N_IN)
def test_block_lengths_on_the_gpu(monkeypatch, n_in):
    _block_lengths(None, monkeypatch, n_in)


@pytest.mark.gpu
def test_slot_layouts_on_the_gpu(monkeypatch):
    _slot_layouts(None, monkeypatch)


@pytest.mark.gpu
def test_float_time_on_the_gpu(monkeypatch):
    _float_time(None, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [JOINED, STAGED, UNPIPELINED], ids=["joined", "staged", "unpipelined"])
def test_class_tables_on_the_gpu(monkeypatch, env):
    _class_tables(None, monkeypatch, env)
