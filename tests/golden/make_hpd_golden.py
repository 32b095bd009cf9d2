#!/usr/bin/env python3
"""Generate tests/golden/hpd.npz from the REFERENCE's calcHPD (np_bnn 0.1.23, BNN_lib.py:286-302).  Runs only beside a checkout of
the upstream repository (imported unmodified; only its outputs on seeded synthetic inputs are stored).  Usage:
    NPBNN_UPSTREAM_DIR=<np_bnn checkout> python tests/golden/make_hpd_golden.py

The inputs are rebuilt from seeds by tests/hpd_cases.py; the fixture holds, per case, upstream's bounds of every column under
``<case>/lo`` and ``<case>/hi`` (float64; exact for float32 inputs)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UPSTREAM = os.environ.get("NPBNN_UPSTREAM_DIR")
if not UPSTREAM:
    sys.exit("NPBNN_UPSTREAM_DIR: set it to a checkout of the upstream np_bnn repository (0.1.23)")
sys.path.insert(0, UPSTREAM)
sys.path.insert(0, os.path.dirname(HERE))

import np_bnn as bn  # noqa: E402  (the reference)
import hpd_cases  # noqa: E402


def main():
    out = {}
    for name, s, level, dtype in hpd_cases.cases():
        x = hpd_cases.case_data(s, dtype, hpd_cases.case_seed(name))
        bounds = [bn.calcHPD(x[:, c], level) for c in range(x.shape[1])]
        out[name + "/lo"] = np.array([b[0] for b in bounds], dtype=np.float64)
        out[name + "/hi"] = np.array([b[1] for b in bounds], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "hpd.npz"), **out)
    print("wrote %d cases to %s" % (len(hpd_cases.cases()), os.path.join(HERE, "hpd.npz")))


if __name__ == "__main__":
    main()
