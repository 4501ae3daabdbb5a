"""The two structures of tw_compare_cohorts as a C compiler sees include/traceweaver_amd.h against their ctypes twins, in the
manner of tests/test_cabi.py::test_ctypes_structures_match_the_header."""
import ctypes
import os
import subprocess

from conftest import REPO

FIELDS = {"tw_cmp_query": ("CmpQuery", ["n_pairs", "pairs", "n_q", "probs", "n_perm", "seed", "max_pool"]),
          "tw_cohort_comparison": ("CohortComparison", ["n_a", "n_b", "ks_gap", "ks_at", "u2", "quantile_shift", "perm_ge_ks", "perm_ge_u", "perm_ge_q"])}


def test_compare_structures_match_the_header(tmp_path):
    from traceweaver_amd import _ffi

    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "traceweaver_amd.h"', 'int main(void) {']
    for c_name, (_, names) in FIELDS.items():
        src.append('printf("%s %%zu", sizeof(%s));' % (c_name, c_name))
        for f in names:
            src.append('printf(" %%zu", offsetof(%s, %s));' % (c_name, f))
        src.append('printf("\\n");')
    src += ['printf("max_q %d\\n", TW_CMP_MAX_Q);', "return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(src))
    exe = str(tmp_path / "abi")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "abi.c"), "-o", exe])
    lines = subprocess.check_output([exe], text=True).splitlines()
    assert lines[-1] == "max_q %d" % _ffi.TW_CMP_MAX_Q and len(lines) == len(FIELDS) + 1
    for line in lines[:-1]:
        c_name, size, *offs = line.split()
        cls = getattr(_ffi, FIELDS[c_name][0])
        assert [name for name, _ in cls._fields_] == FIELDS[c_name][1], c_name
        assert ctypes.sizeof(cls) == int(size), c_name
        assert [getattr(cls, f).offset for f in FIELDS[c_name][1]] == [int(o) for o in offs], c_name


def test_compare_entry_point_is_listed():
    from traceweaver_amd import _ffi

    assert "tw_compare_cohorts" in _ffi.EXPORTS and _ffi.TW_CMP_MAX_Q == 8
    text = open(os.path.join(REPO, "include", "traceweaver_amd.h")).read()
    assert "int tw_compare_cohorts(tw_engine *e, const tw_cmp_query *q, const tw_cohort_comparison *out, int64_t *summary4);" in text
