"""The stitch entry points cross the ABI as include/traceweaver_amd.h declares them: symbols in the HIP library and in the
host-emulation build, tw_stitched as a C compiler lays it out against the ctypes declaration."""
import ctypes
import os
import subprocess

from conftest import REPO

NAMES = ("tw_set_span_rows", "tw_set_parents", "tw_stitch_traces")


def test_symbols_in_the_hip_library():
    from traceweaver_amd import _ffi, build

    lib = ctypes.CDLL(build.build())
    for name in NAMES:
        assert hasattr(lib, name) and name in _ffi.EXPORTS


def test_symbols_in_the_emulation_build(emu_lib):
    lib = ctypes.CDLL(emu_lib)
    for name in NAMES:
        assert hasattr(lib, name)


def test_tw_stitched_layout(tmp_path):
    from traceweaver_amd import _ffi

    members = [f for f, _ in _ffi.Stitched._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "traceweaver_amd.h"', 'int main(void) {',
           'printf("%zu", sizeof(tw_stitched));']
    src += ['printf(" %%zu", offsetof(tw_stitched, %s));' % m for m in members]
    src += ['printf("\\n");', "return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(src))
    exe = str(tmp_path / "abi")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "abi.c"), "-o", exe])
    size, *offs = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert ctypes.sizeof(_ffi.Stitched) == size == 8 * len(members)
    assert [getattr(_ffi.Stitched, m).offset for m in members] == offs


def test_timing_slots_are_appended(emu_lib):
    """tw_get_timing keeps its first ten slots; the stitch figures follow them."""
    import numpy as np

    from traceweaver_amd.engine import Engine

    eng = Engine(0, lib_path=emu_lib)
    assert list(eng.timing()) == ["pass", "enumerate", "select", "windows", "repair", "params", "fit", "rounds", "host_enum_submit", "host_pass"]
    assert list(eng.stitch_timing()) == ["stitch", "links", "jump", "scatter", "group", "rounds"]
    ms = np.full(10, -1.0)
    eng._lib.tw_get_timing(eng._h, ctypes.c_void_p(ms.ctypes.data), 10)
    assert (ms >= 0).all()
    eng.close()
