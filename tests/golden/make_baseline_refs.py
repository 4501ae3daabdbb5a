"""Writes tests/golden/baseline_refs.npz: what the reference's own FCFS, ArrivalOrder, vPath and WAP5 classes return for every
input of tests/test_baselines.py (generated corpora, shipped corpora, load-scaled units), in the layout run_reference() describes.
The test then compares traceweaver_amd/baselines.py with these arrays and needs no reference tree.

    python tests/golden/make_baseline_refs.py <root of the reference's tree>
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main(ref_root):
    os.environ.setdefault("TW_TILE", "1")
    os.environ.setdefault("TW_COOP_THREADS", "1")
    import test_baselines as B
    from hostemu.build_emu import build

    lib = build()
    classes = B.reference_classes(os.path.join(ref_root, "src", "trace_reconstructor", "ports", "python"))
    out = {}

    def add(case, units, parents=True, wap5=True):
        for k, v in B.run_reference(units, classes, parents, wap5).items():
            out[case + "/" + k] = v

    with tempfile.TemporaryDirectory() as d:
        for case, app, seed, traces, conc in B.GENERATED:
            add(case, B.generated_units(lib, os.path.join(d, case), app, seed, traces, conc), case != "gen_wap5", case == "gen_wap5")
        for factor in B.SCALED:
            add("scaled_%d" % factor, B.scaled_units(lib, os.path.join(d, "scaled_%d" % factor), factor))
    for rel, fix in B.WAP5_CORPORA:
        add(rel, B.corpus_units(lib, ref_root, rel, fix), parents=False)
    for rel, fix in B.BASELINE_CORPORA:
        add(rel, B.corpus_units(lib, ref_root, rel, fix), wap5=False)
    np.savez_compressed(os.path.join(HERE, "baseline_refs.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
