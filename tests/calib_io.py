"""Load the calibration golden fixtures (tests/golden/make_golden_calib.py)."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def calib_fixtures():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "calib_*.npz"))):
        z = np.load(path)
        d = {k: z[k] for k in z.files}
        d["name"] = os.path.basename(path)[6:-4]
        d["dists"] = json.loads(str(d["dists"]))
        # the value types decide the reference's weights dtype: np.float64 ->
        # float64, Python float -> float32 (make_golden_calib.py)
        d["pyfloat"] = bool(int(d["pyfloat"]))
        if not d["pyfloat"]:
            d["dists"] = [{k: np.float64(v) for k, v in t.items()} for t in d["dists"]]
        d["learn_logit"] = bool(int(d["learn_logit"]))
        d["active"] = bool(int(d["active"]))
        d["fair_coeff"] = float(d["fair_coeff"])
        for k in ("labels", "sensitive", "centroids"):
            d[k] = d[k].astype(np.int64)
        out.append(d)
    return out


def gap(f, key):
    """max |fp32 record - fp64 record| of one recorded tensor: the reference's
    own fp32 error on this case."""
    return float(np.abs(np.asarray(f[key], np.float64) - f[key + "_64"]).max())
