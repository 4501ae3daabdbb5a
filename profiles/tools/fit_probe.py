"""What the refit's workgroups are on the headline workload, measured on the CPU with the restatement (oracle/tw_refit.py):
per scored row of the six media-shape services at --n requests, from the ground-truth gaps (they stand in for pass 1's): samples,
distinct values, the count BIC selects, Lloyd iterations and EM sweeps of the model-selection fits and of the final fit, and
whether the selected count is the largest admissible one, min(5, #distinct) -- the count the engine fits ahead (TW_FIT_SPEC).

    python profiles/tools/fit_probe.py [--n 100000] [--seed 1000]

The iteration counts come from counting calls inside the restatement (two np.bincount per Lloyd iteration, one _params per EM
sweep and one for the start); the restatement itself is not changed."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import tw_refit as R  # noqa: E402
from traceweaver_amd import synth  # noqa: E402
from traceweaver_amd.predictor import TraceWeaverGPU, reference_fit_order  # noqa: E402


class Calls(object):
    """Counts the calls of np.bincount and R._params while a fit of the restatement runs.  Tied to oracle/tw_refit.py as it stands:
    `lloyd` calls np.bincount exactly twice per iteration (the counts `w` and the sums `s`) and nowhere else, hence `bincount // 2`;
    `gmm_fit` calls `_params` once for the start from the k-means labels and once per EM sweep, hence `params - 1`.  Another
    bincount or _params call in the restatement changes these figures: main() checks the two relations on a row of two values first."""

    def __enter__(self):
        self.bincount = self.params = 0
        self._b, self._p = np.bincount, R._params

        def bincount(*a, **k):
            self.bincount += 1
            return self._b(*a, **k)

        def params(*a, **k):
            self.params += 1
            return self._p(*a, **k)

        np.bincount, R._params = bincount, params
        return self

    def __exit__(self, *a):
        np.bincount, R._params = self._b, self._p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    # two point masses, two clusters: k-means++ picks both values and Lloyd's first iteration moves no centre (one iteration, 2 bincount
    # calls), and a fit of one component is the start plus two sweeps (3 _params calls: the second sweep moves nothing)
    with Calls() as c:
        R.kmeans_labels(np.repeat([1.0, 9.0], 50), 2, np.array([0.1, 0.9, 0.9]))
    assert c.bincount == 2, "oracle/tw_refit.py changed: np.bincount calls per Lloyd iteration (%d for one iteration)" % c.bincount
    with Calls() as c:
        R.gmm_fit(np.repeat([1.0, 9.0], 50), 1, np.array([0.5]), full=False)
    assert c.params == 3, "oracle/tw_refit.py changed: _params calls per EM sweep (%d for a start and two sweeps)" % c.params
    units, truth = synth.make_workload(args.seed, args.n, services=synth.MEDIA_SERVICES, replicas=1, concurrency=1.6)
    rng = np.random.RandomState(0)
    print("unit E slot samples distinct selected largest lloyd_iterations(k=2..max) em_sweeps(k=1..max) final_lloyd final_em")
    for ui, (u, tp) in enumerate(zip(units, truth)):
        for q in reference_fit_order(u, u.key_rank):
            x = TraceWeaverGPU._gap_row(u, tp.astype(np.int64), q)
            if len(x) == 0:
                continue
            uniq = len(np.unique(x))
            max_n = min(uniq, R.MAX_COMP)
            tape = rng.random_sample(R.draws_per_row(max_n))
            t, bics, ll, em = 0, [], [], []
            for k in range(1, max_n + 1):
                with Calls() as c:
                    m = R.gmm_fit(x, k, tape[t:t + R.draws_per_fit(k)], full=False)
                t += R.draws_per_fit(k)
                if k > 1:
                    ll.append(c.bincount // 2)
                em.append(c.params - 1)
                bics.append(np.inf if m is None else R.bic(m[4], len(x), k))
            sel = int(np.argmin(bics)) + 1
            with Calls() as c:
                R.gmm_fit(x, sel, R.refit_tape(sel), full=True)
            print("%d %d %d %d %d %d %s %s %s %d %d" % (ui, u.E, q, len(x), uniq, sel, "yes" if sel == max_n else "no",
                                                     ",".join(map(str, ll)), ",".join(map(str, em)), c.bincount // 2, c.params - 1), flush=True)


if __name__ == "__main__":
    main()
