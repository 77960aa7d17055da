"""Golden vectors for the post-process threshold calibration.

Runs ONLY in the build container, where the reference is mounted at
/root/reference (it never travels to the GPU box).  The outputs come from the
reference's own source text, fairsoft_train_postprocess.py, executed in a
prepared namespace (the module cannot be imported here: it pulls in main ->
train -> tensorboard, absent, and both blocks are inline in long functions):

  * ``logit`` / ``sigmoid`` / ``calibrate_p`` (:39-49);
  * the training block, from ``sensitive_feat = torch.from_numpy(`` through
    ``smooth_fair_loss += fair_loss.item()`` (:112-165);
  * the evaluation's calibrate lines (:376-381) and its fairness block, from
    ``if eval_fairness:`` through ``mean_diffs = np.mean(mean_diffs)``
    (:413-446).

Each case records the fp32 run -- the reference as it is -- and the same
block on the same values as fp64 tensors (``*_64``; there ``torch.tensor`` of
the looked-up weights is made float64 as well, so that the record is fp64
throughout).  The reference's own fp32-vs-fp64 gap is what the tests measure
the fp32 record with: <= 4e-6 relative on gradients for the interior draws,
1e-3 to 1e-2 for the edge draw.  Recorded per run: bce, fair_loss (0 and
active = 0 when the reference leaves it a Python float), total, cal_prob, the
gradients of total w.r.t. threshold_ and indiv_prob (active cases), and the
gradients of bce_loss alone (every case).  Data only.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_calib.py [NAME ...]
Writes: tests/golden/calib_*.npz
"""
import argparse
import json
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/fairsoft_train_postprocess.py"


def _between(lines, first, last, start=0):
    a = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(first))
    b = next(i for i in range(a, len(lines)) if last in lines[i])
    return textwrap.dedent("\n".join(lines[a:b + 1])), (a + 1, b + 1)


def reference_blocks():
    lines = open(REF).read().split("\n")
    funcs, fl = _between(lines, "def logit(p):", "return sigmoid(cal_logit)")
    train, tl = _between(lines, "sensitive_feat = torch.from_numpy(",
                         "smooth_fair_loss += fair_loss.item()")
    ev0 = next(i for i, l in enumerate(lines) if "def evaluate_fair_through_postprocess" in l)
    cal, cl = _between(lines, "sen_belong = torch.all(", "cal_prob = cal_prob.transpose(1, 2)[sen_belong]",
                       ev0)
    ev, el = _between(lines, "if eval_fairness:", "mean_diffs = np.mean(mean_diffs)", cl[1])
    print("functions :%d-%d, training block :%d-%d, eval calibrate :%d-%d, eval block :%d-%d"
          % (fl + tl + cl + el))
    return funcs, train, cal, ev


class _Torch64:
    """``torch`` for the fp64 run: ``torch.tensor(weights)`` gives float64."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def tensor(x, *a, **k):
        k.setdefault("dtype", torch.float64)
        return torch.tensor(x, *a, **k)


class _Data:
    pass


def run_train(blocks, case, dt):
    funcs, train = blocks[0], blocks[1]
    p = torch.tensor(case["p"], dtype=dt, requires_grad=True)
    x = torch.tensor(case["threshold"], dtype=dt, requires_grad=True)
    base = torch.tensor(1.25, dtype=dt, requires_grad=True)
    data = _Data()
    data.labels, data.sensitive_feat = case["labels"], case["sensitive"]
    B = case["labels"].shape[0]
    ns = dict(torch=_Torch64() if dt == torch.float64 else torch, np=np, data=data,
              idx=np.arange(B),
              args=argparse.Namespace(device="cpu", learn_logit=case["learn_logit"],
                                      fair_coeff=case["fair_coeff"]),
              sen_centroids=torch.from_numpy(case["centroids"]), threshold_=x, indiv_prob=p,
              input_label=torch.tensor(case["labels"], dtype=dt),
              target_fair_labels=case["targets"], label_distances=case["dists"],
              contributed_reg_fair_sample=0, total_loss=base * 1.0, smooth_fair_loss=0.0)
    exec(funcs, ns)
    exec(train, ns)
    fl, bce, total = ns["fair_loss"], ns["bce_loss"], ns["total_loss"]
    g_bce = torch.autograd.grad(bce, [x, p], retain_graph=True)
    rec = dict(bce=bce.item(), total=total.item(), cal_prob=ns["cal_prob"].detach().numpy(),
               g_bce_threshold=g_bce[0].numpy(), g_bce_p=g_bce[1].numpy(),
               contributed=ns["contributed_reg_fair_sample"])
    if isinstance(fl, float):
        rec.update(active=0, fair=fl)
    else:
        total.backward()
        rec.update(active=1, fair=fl.item(), fair_dtype=str(fl.dtype).replace("torch.", ""),
                   g_threshold=x.grad.numpy(), g_p=p.grad.numpy())
    return rec


def run_eval(blocks, case, dt, thr=None):
    """``thr``: the evaluation's threshold as the fp32 run made it (the fp64 run
    calibrates with the same values)."""
    funcs, cal, ev = blocks[0], blocks[2], blocks[3]
    x = torch.tensor(case["threshold"], dtype=dt)
    data = _Data()
    data.labels, data.sensitive_feat = case["labels"], case["sensitive"]
    B = case["labels"].shape[0]
    ns = dict(torch=torch, np=np, data=data, indiv_prob=torch.tensor(case["p"], dtype=dt),
              sensitive_feat=torch.from_numpy(case["sensitive"]),
              sen_centroids=torch.from_numpy(case["centroids"]))
    exec(funcs, ns)
    # the caller's sigmoid (evaluate_over_labels, :541-543), then :376-381
    if thr is not None:
        ns["threshold_"] = torch.tensor(thr, dtype=dt)
    else:
        ns["threshold_"] = ns["sigmoid"](x) if case["learn_logit"] else x
    exec(cal, ns)
    cal_prob = ns["cal_prob"].numpy()
    ns.update(eval_fairness=True, calibrated_prob=[cal_prob], subset_idx=np.arange(B),
              train_sensitive=case["sensitive"], target_fair_labels=case["targets"],
              label_distances=case["dists"])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # np.mean([]) of a fully inactive split
        exec(ev, ns)
    return dict(eval_threshold=ns["threshold_"].numpy(), eval_cal_prob=cal_prob,
                eval_mean_diff=float(ns["mean_diffs"]))


def make_case(name, B, L, G, T, seed, learn_logit, pyfloat, coeff, kind=""):
    rng = np.random.default_rng(300 + seed)
    labels = (rng.random((B, L)) < 0.3).astype(np.int64)
    labels[B // 2:, :] = labels[:B - B // 2, :]  # repeated patterns
    # two sensitive columns; G distinct patterns, every one present
    pats = np.array([[g % 2, g // 2] for g in range(G)], np.int64)
    gsel = np.concatenate([np.arange(G), rng.integers(0, G, B - G)]) if B >= G else \
        np.arange(B) % G
    rng.shuffle(gsel)
    sens = pats[gsel]
    centroids = np.unique(sens, axis=0)
    assert len(centroids) == G, name
    miss = np.zeros(B, bool)
    if kind == "zero_weight_group":  # a group with rows, none of them in any dict
        miss = (sens == centroids[0]).all(1)
        miss |= np.array([any((labels[b] == labels[c]).all() for c in np.where(miss)[0])
                          for b in range(B)])
    if kind == "inactive":
        miss[:] = True
    keys = ["".join(r.astype(str)) for r in labels[~miss]]
    extra = ["".join(rng.integers(0, 2, L).astype(str)) for _ in range(4)]
    dists, targets = {}, []
    for t in range(T):
        tk = "".join(rng.integers(0, 2, L).astype(str))
        if pyfloat:  # Python floats: torch.tensor(weights) is float32
            d = {k: (1 + int(rng.integers(0, 3))) / 3 for k in keys + extra if rng.random() < 0.7}
        else:        # numpy float64, as label_distance.py's np.clip(np.exp(...))
            d = {k: np.float64(rng.uniform(0.05, 1.0)) for k in keys + extra
                 if rng.random() < 0.7}
        if kind == "dead_target" and t == 1:  # this target's dict misses the whole batch
            d = {k: np.float64(0.5) for k in extra}
        dists[tk] = d
        targets.append(tk)
    if kind == "edge":  # within 1e-4 of the ends of the probit's range
        lo = 5e-7 + rng.uniform(0, 1e-4, (B, L))
        hi = 1 - 5e-7 - rng.uniform(0, 1e-4, (B, L))
        p = np.where(rng.random((B, L)) < 0.5, lo, hi)
    else:
        p = rng.uniform(0.02, 0.98, (B, L))
    thr = rng.uniform(0.3, 0.7, (1, L, G))
    if learn_logit:
        thr = np.log(thr / (1 - thr))
    return dict(name=name, p=p.astype(np.float32), threshold=thr.astype(np.float32),
                labels=labels, sensitive=sens, centroids=centroids, dists=dists, targets=targets,
                learn_logit=bool(learn_logit), pyfloat=bool(pyfloat), fair_coeff=coeff)


CASES = [  # name, B, L, G, T, seed, learn_logit, pyfloat, fair_coeff, kind
    ("c1_logit", 24, 20, 3, 2, 1, True, False, 1.5, ""),
    ("c2_prob_pyfloat", 24, 20, 3, 2, 2, False, True, 0.7, ""),
    ("c3_zero_weight_group", 30, 12, 3, 2, 3, True, False, 2.0, "zero_weight_group"),
    ("c4_dead_target", 21, 16, 4, 3, 4, False, False, 1.0, "dead_target"),
    ("c5_inactive", 10, 9, 2, 2, 5, True, False, 1.0, "inactive"),
    ("c6_one_group", 12, 33, 1, 2, 6, True, True, 1.0, ""),
    ("c7_l257", 5, 257, 3, 2, 7, False, False, 0.9, ""),
    ("c8_edge", 24, 50, 3, 1, 8, True, False, 1.0, "edge"),
]


def main():
    only = set(sys.argv[1:])
    blocks = reference_blocks()
    for spec in CASES:
        if only and spec[0] not in only:
            continue
        case = make_case(*spec)
        r32, r64 = run_train(blocks, case, torch.float32), run_train(blocks, case, torch.float64)
        e32 = run_eval(blocks, case, torch.float32)
        e64 = run_eval(blocks, case, torch.float64, thr=e32["eval_threshold"])
        assert r32["active"] == r64["active"] and r32["contributed"] == r64["contributed"]
        rec = dict(p=case["p"], threshold=case["threshold"], labels=case["labels"].astype(np.int8),
                   sensitive=case["sensitive"].astype(np.int8),
                   centroids=case["centroids"].astype(np.int8),
                   dists=np.array(json.dumps([{k: float(v) for k, v in case["dists"][t].items()}
                                              for t in case["targets"]])),
                   learn_logit=np.array(int(case["learn_logit"])),
                   pyfloat=np.array(int(case["pyfloat"])), fair_coeff=np.array(case["fair_coeff"]))
        for k, v in r32.items():
            rec[k] = np.array(v)
        for k, v in r64.items():
            if k not in ("active", "contributed", "fair_dtype"):
                rec[k + "_64"] = np.array(v)
        for k, v in e32.items():
            rec[k] = np.array(v)
        rec["eval_cal_prob_64"] = e64["eval_cal_prob"]
        rec["eval_mean_diff_64"] = np.array(e64["eval_mean_diff"])
        path = os.path.join(HERE, f"calib_{case['name']}.npz")
        np.savez_compressed(path, **rec)
        gap = lambda k: float(np.abs(rec[k] - rec[k + "_64"]).max() /
                              max(np.abs(rec[k + "_64"]).max(), 1e-300))
        print(case["name"], "active", r32["active"], "bce", r32["bce"], "fair", r32["fair"],
              r32.get("fair_dtype", "-"), "mean_diff", e32["eval_mean_diff"],
              "fp32-fp64 gap: g_bce_threshold %.1e cal_prob %.1e" % (gap("g_bce_threshold"),
                                                                      gap("cal_prob")),
              "%d KB" % (os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
