"""The C-ABI of the trace extraction (tw_extract_traces / tw_get_extracted): the symbols in both builds, the structs' layout as
include/traceweaver_amd.h declares it, the timing slots appended after the last one in use."""
import ctypes
import os
import re

import numpy as np
import pytest

from traceweaver_amd import _ffi, build

HEADER = os.path.join(build.REPO, "include", "traceweaver_amd.h")


def test_symbols_in_the_emulation_build(emu_lib):
    lib = ctypes.CDLL(emu_lib)
    for name in ("tw_extract_traces", "tw_get_extracted"):
        assert name in _ffi.EXPORTS and getattr(lib, name) is not None


def test_symbols_in_the_hip_library():
    lib = ctypes.CDLL(build.build())                              # (loading it needs no device)
    for name in ("tw_extract_traces", "tw_get_extracted"):
        assert getattr(lib, name) is not None


def test_struct_layout_follows_the_header():
    text = open(HEADER).read()
    query = re.search(r"typedef struct \{([^}]*)\} tw_extract_query;", text).group(1)
    out = re.search(r"typedef struct \{([^}]*)\} tw_extracted;", text).group(1)
    strip = lambda body: re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = lambda body: [n.strip(" *") for decl in strip(body).split(";") if decl.strip() for n in decl.strip().split(" ", 2 if decl.strip().startswith("const") else 1)[-1].split(",")]
    assert names(query) == [k for k, _ in _ffi.ExtractQuery._fields_]
    assert names(out) == [k for k, _ in _ffi.Extracted._fields_]
    # uint32 x 2, int32 x 2, int64, int32 x 2, two pointers: no padding on the LP64 targets the engine builds for
    assert ctypes.sizeof(_ffi.ExtractQuery) == 4 * 4 + 8 + 2 * 4 + 2 * ctypes.sizeof(ctypes.c_void_p) == 48
    assert _ffi.ExtractQuery.limit.offset == 16 and _ffi.ExtractQuery.probs.offset == 32 and _ffi.ExtractQuery.list.offset == 40
    assert ctypes.sizeof(_ffi.Extracted) == 16 * ctypes.sizeof(ctypes.c_void_p)
    assert _ffi.TW_EXTR_MAX_PROBS == int(re.search(r"#define TW_EXTR_MAX_PROBS (\d+)", text).group(1)) == 32
    assert "#define TW_EXTR_MAX_LIST (1 << 20)" in text and _ffi.TW_EXTR_MAX_LIST == 1 << 20


def run_timing_slots(lib):
    """The slots of the extraction follow the filter's 46 .. 48, which keep their meaning: an extraction leaves them as they were."""
    import test_profiles as tp
    from traceweaver_amd.traces import clause

    eng, st, link, rows, group, G = tp.table_engine(lib, tp.wide_table(16))
    ms = lambda: (lambda a: (eng._check(eng._lib.tw_get_timing(eng._h, a.ctypes.data_as(ctypes.c_void_p), 52)), a)[1])(np.full(52, -1.0))
    before = ms()
    assert (before[49:52] == 0).all()
    eng.filter_traces([clause("rows", 3, 3)])
    mid = ms()
    assert (mid[49:52] == 0).all()
    x = eng.extract_traces("top", "tree")
    after = ms()
    assert np.array_equal(after[:49], mid[:49]) and (after[49:52] >= 0).all() and x.n_trees == st.n_trees
    assert eng.filter_timing() == dict(zip(("trees", "list", "copies"), mid[46:49].tolist()))
    assert eng.extract_timing() == dict(zip(("select", "trees", "copies"), after[49:52].tolist()))
    short = np.full(50, -1.0)
    eng._check(eng._lib.tw_get_timing(eng._h, short.ctypes.data_as(ctypes.c_void_p), 50))
    assert np.array_equal(short, after[:50])
    eng.close()


def test_timing_slots_are_appended(emu_lib):
    run_timing_slots(emu_lib)


@pytest.mark.gpu
def test_timing_slots_are_appended_gpu():
    run_timing_slots(None)
