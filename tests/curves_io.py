"""Load the validation-metric golden fixtures (tests/golden/make_golden_curves.py)."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def curve_fixtures():
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "curves_*.npz"))):
        z = np.load(p)
        d = {k: z[k] for k in z.files}
        d["name"] = os.path.basename(p)[7:-4]
        out.append(d)
    return out
