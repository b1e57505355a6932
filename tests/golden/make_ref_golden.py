"""Regenerates tests/golden/ref_<program>_<case>.npz: what the reference programs, executed
as host code by oracle/refdiff.py, left behind on the cases of oracle/ref_cases.py.  Needs a
reference checkout ($GF_REFERENCE) and the built package:

    python tests/golden/make_ref_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import refdiff as R, ref_cases as RC  # noqa: E402


def main():
    if R.reference_root() is None:
        sys.exit("no reference checkout: set $%s" % R.REF_ENV)
    R.build()
    for case in RC.CASES:
        sc = RC.scenario(case)
        for program in RC.PROGRAMS:
            d = R.fixture_arrays(sc, program, RC.nows(sc), RC.params(case))
            bad = sum(int(d[k][:, 12].sum()) for k in d if k.endswith("_obs"))
            path = os.path.join(HERE, "ref_%s_%s.npz" % (program, case))
            np.savez_compressed(path, **d)
            print("%s: %d bytes, unmodelled helper reached by %d packets" % (path, os.path.getsize(path), bad))
            assert bad == 0 and os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
