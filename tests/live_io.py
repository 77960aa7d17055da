"""Load tests/golden/live_l20.npz (made by tests/golden/make_golden_live.py): the
reference's gradients, or None, of 13 objectives over the outputs of
compute_loss, and the checks every backend is held to against it."""
import argparse
import os

import numpy as np
import torch

import mpvae

from golden_io import GOLDEN, OUTS
from tolerances import FWD_RTOL, GRAD_RTOL, rel_err

GRADS = ["fe_out", "fe_mu", "fe_logvar", "fx_out", "fx_mu", "fx_logvar", "r_sqrt_sigma"]
# the 13 objectives, as tuples of output names (the fixture's, in its order)
SUBSETS = [(k,) for k in OUTS] + [("nll", "c_x"), ("nll_x", "c"), ("kl", "indiv_prob"),
                                  ("nll", "nll_x", "kl"), tuple(OUTS)]
SCALARS = OUTS[:6]
KEYS = ["y", "fe_out", "fe_mu", "fe_logvar", "fx_out", "fx_mu", "fx_logvar"]


class LiveFixture:
    def __init__(self, path=os.path.join(GOLDEN, "live_l20.npz")):
        z = np.load(path)
        self.data = {k: z[k] for k in z.files}
        self.L, self.z, self.B, self.S, self.d = (int(v) for v in self.data["meta"])
        self.nll_coeff, self.c_coeff = (float(v) for v in self.data["coeffs"])
        self.objectives = [tuple(str(o).split("+")) for o in self.data["objectives"]]
        assert self.objectives == SUBSETS

    def __getitem__(self, k):
        return self.data[k]

    def args(self, **extra):
        return argparse.Namespace(label_dim=self.L, z_dim=self.z, n_train_sample=self.S,
                                  n_test_sample=self.S, mode="train", nll_coeff=self.nll_coeff,
                                  c_coeff=self.c_coeff, **extra)

    def grads(self, i):
        """{input: the reference's gradient of objective i, or None}."""
        return {k: None if self.data["is_none"][i, j] else self.data[f"g{i}_{k}"]
                for j, k in enumerate(GRADS)}

    def weights(self, obj):
        """The scalar outputs' weights of one objective as elbo_backward keywords."""
        w = dict(zip(SCALARS, self.data["w"]))
        return {"g_" + k: float(w[k]) for k in obj if k in w}


def nan_rows(g):
    return np.isnan(g).all(1).nonzero()[0].tolist()


def check_live(fix, run):
    """run(obj) -> {input: gradient array or None} of the objective
    sum_{k in obj} w_k out_k (w_k the fixture's weight, g_I or g_IL) on the
    fixture's inputs and noise.  Against the reference's record: equal NaN
    patterns, None met by None or exact zeros, GRAD_RTOL elsewhere; and the
    per-branch fact stated outright."""
    bad, worst = [], 0.0
    for i, obj in enumerate(fix.objectives):
        got, ref = run(obj), fix.grads(i)
        tag = "+".join(obj) if len(obj) < 8 else "all"
        for k in GRADS:
            g = None if got[k] is None else np.asarray(got[k], np.float64)
            if ref[k] is None:
                if g is not None and (g != 0).any():   # NaN != 0 too
                    bad.append((tag, k, "the reference returns None"))
                continue
            if g is None:
                bad.append((tag, k, "None"))
            elif not np.array_equal(np.isnan(g), np.isnan(ref[k])):
                bad.append((tag, k, "NaN pattern"))
            else:
                e = rel_err(g, ref[k])
                worst = max(worst, e)
                if e > GRAD_RTOL:
                    bad.append((tag, k, e))
        if len(obj) > 1:
            continue
        # one output alone: which branch a degenerate row (1: no positive,
        # 4: no negative) poisons
        nan = {k: got[k] is not None and bool(np.isnan(got[k]).any()) for k in GRADS}
        hit = {"c": "fe_out", "c_x": "fx_out"}.get(obj[0])
        if obj[0] == "total":
            want = {"fe_out", "fx_out", "r_sqrt_sigma"}
        else:
            want = {hit, "r_sqrt_sigma"} if hit else set()
        if {k for k in GRADS if nan[k]} != want:
            bad.append((tag, "NaN in", sorted(k for k in GRADS if nan[k])))
        for k in want:
            if got[k] is None:
                continue  # already reported above
            rows = nan_rows(got[k])
            if rows != ([1, 4] if k != "r_sqrt_sigma" else list(range(fix.L))):
                bad.append((tag, k, "NaN rows", rows))
    assert not bad, bad
    return worst


def compute_loss_runner(f, device, **extra):
    """run(obj) of check_live through mpvae.compute_loss on `device`."""
    ups = [torch.tensor(float(w), dtype=torch.float32, device=device) for w in f["w"]] + \
        [torch.from_numpy(f["g_I"]).to(device), torch.from_numpy(f["g_IL"]).to(device)]

    def run(obj):
        t = {k: torch.from_numpy(f[k].copy()).to(device) for k in KEYS + ["r_sqrt_sigma"]}
        for k in GRADS:
            t[k].requires_grad_(True)
        out = mpvae.compute_loss(*[t[k] for k in KEYS], t["r_sqrt_sigma"],
                                 f.args(mpvae_noise=torch.from_numpy(f["noise"]), **extra))
        for k, o in zip(OUTS, out):
            e = rel_err(o.detach().cpu().double().numpy(), f["out_" + k])
            assert e <= FWD_RTOL, (k, e)
        sum((out[OUTS.index(k)] * ups[OUTS.index(k)]).sum() for k in obj).backward()
        for k in GRADS:
            assert t[k].grad is None or t[k].grad.dtype == t[k].dtype, k
        return {k: None if t[k].grad is None else t[k].grad.cpu().double().numpy()
                for k in GRADS}
    return run
