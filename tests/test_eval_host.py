"""CPU: the evaluation restatement (tests/eval_ref.py) against the reference's
own records (tests/golden/make_golden_eval.py), ``mpvae_fair.split_scores`` on
CPU tensors against the restatement, ``mpvae_step.EvalPass`` on a small VAE
through libmpvae_host.so, and the host-side argument checks of mpv_split_eval.

Tolerances.  F1 against the records: relative 4 N 2^-24 -- the reference sums N
non-negative fp32 terms per label sequentially (relative error <= N 2^-24 per
count) and rounds each count to fp32 once more; F1 is a ratio of such counts.
fair_mean_diff is fp64 on both sides: 2^-52 plus four times the restatement's
own sensitivity to the order of the rows (eval_ref.tol), measured here with the
rows permuted.  Measured on the CPU: miF1 <= 1.1e-7, maF1 <= 1.6e-7 of the records
(bounds 9.5e-6 at N = 40 to 7.2e-5 at N = 300), fair_mean_diff equal bit for bit.
"""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import eval_ref as er
import mpvae
import mpvae_fair as mf
import mpvae_hip as H
import mpvae_step as ms

FIX = er.eval_fixtures()
IDS = [f["name"] for f in FIX]


def _restated(f, weight_labels=None):
    wl = f["weight_labels"] if weight_labels is None else weight_labels
    w = er.weights(wl, f["dists"])
    gid = er.group_of(f["sensitive"], f["centroids"])
    G = len(f["centroids"])
    return er.scores(f["pred"], f["labels"], w, gid, G), \
        er.order_sensitivity(f["pred"], f["labels"], w, gid, G)


def test_the_cases_the_issue_lists_are_recorded():
    by = {f["name"]: f for f in FIX}
    assert set(by) >= {"e1_l25", "e2_dead_zero_fn", "e3_inactive", "e4_first_rows", "e5_l257"}
    assert by["e1_l25"]["pred"].shape == (300, 25) and len(by["e1_l25"]["dists"]) == 2
    assert len(by["e1_l25"]["centroids"]) == 3
    f = by["e2_dead_zero_fn"]
    w, gid = er.weights(f["weight_labels"], f["dists"]), er.group_of(f["sensitive"], f["centroids"])
    assert (w.sum(1) == 0).tolist() == [False, True, False]        # a dead target
    assert (gid == 0).any() and (w[:, gid == 0] == 0).all()        # a zero-weight group
    assert er.counts(f["pred"], f["labels"])[2].sum() == 25        # fn > 0: p == 0 under y == 1
    assert np.signbit(f["pred"][(f["pred"] == 0) & (f["labels"] == 1)]).any()   # a -0.0 among them
    assert np.isnan(by["e3_inactive"]["fair_mean_diff"])
    f = by["e4_first_rows"]
    assert not np.array_equal(f["weight_labels"], f["labels"])
    assert all(np.array_equal(g["weight_labels"], g["labels"]) for g in FIX if g is not f)
    f = by["e5_l257"]
    assert f["pred"].shape == (40, 257) and len(f["dists"]) == 9 and len(f["centroids"]) == 2


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_restatement_matches_the_records(f):
    got, s = _restated(f)
    N = len(f["pred"])
    f1_tol = 4 * N * 2.0 ** -24
    for k in ("miF1", "maF1"):
        e = abs(got[k] - float(f[k])) / abs(float(f[k]))
        print(f"{f['name']} {k}: {e:.3g} (bound {f1_tol:.3g})")
        assert e <= f1_tol, (k, e)
    ref = float(f["fair_mean_diff"])
    e = er.err(got["fair_mean_diff"], ref)
    print(f"{f['name']} fair_mean_diff: {e:.3g} (bound {er.tol(s['fair']):.3g})")
    assert e <= er.tol(s["fair"])


def test_the_weights_come_from_the_first_rows_in_the_reference():
    """e4: the record follows ``data.labels[np.arange(N)]`` (weight_labels);
    with the split's own labels the restatement gives another result (here no
    row of the split is in a dict at all: NaN)."""
    f = next(f for f in FIX if f["name"] == "e4_first_rows")
    own, _ = _restated(f, f["labels"])
    ref = float(f["fair_mean_diff"])
    assert not abs(own["fair_mean_diff"] - ref) <= 1e-3 * abs(ref)


def _tables(f, dev="cpu"):
    L = f["labels"].shape[1]
    return [mf.LabelDistanceTable(d, L, dev) for d in f["dists"]]


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _assert_scores(sc, ref, s, what=""):
    L = ref["counts"].shape[1]
    for k in ("miF1", "maF1", "fair_mean_diff", "fair_mean_sq"):
        v = getattr(sc, k)
        assert v.dtype == torch.float64 and v.dim() == 0, k
        bound = er.f1_tol(s["counts"], L) if k in ("miF1", "maF1") else er.tol(s["fair"])
        assert er.err(float(v), ref[k]) <= bound, (what, k, float(v), ref[k])
    assert er.err(sc.counts.numpy(), ref["counts"]) <= er.tol(s["counts"]), what
    assert er.err(sc.fair_terms.numpy(), ref["terms"]) <= er.tol(s["fair"]), what


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_split_scores_on_cpu_tensors(f):
    ref, s = _restated(f)
    sc = mf.split_scores(_t(f["pred"]), _t(f["labels"], torch.float32), _t(f["sensitive"]),
                         _t(f["centroids"]), _tables(f), _t(f["weight_labels"], torch.float32))
    _assert_scores(sc, ref, s, f["name"])
    assert sc.gid.dtype == torch.int32
    assert np.array_equal(sc.gid.numpy(), er.group_of(f["sensitive"], f["centroids"]))
    # the table lookup on the host against the dicts
    w = mf._table_weights_host(_t(f["weight_labels"], torch.float32), _tables(f))
    assert np.array_equal(w.numpy(), er.weights(f["weight_labels"], f["dists"]))


def test_split_scores_without_fairness_and_edge_inputs():
    f = FIX[0]
    p, y = _t(f["pred"]), _t(f["labels"], torch.float32)
    sc = mf.split_scores(p, y)
    assert sc.fair_mean_diff is None and sc.fair_mean_sq is None and sc.fair_terms is None
    assert sc.gid is None
    ref = er.scores(f["pred"], f["labels"])
    s = er.order_sensitivity(f["pred"], f["labels"])
    assert er.err(float(sc.miF1), ref["miF1"]) <= er.f1_tol(s["counts"], p.shape[1])
    assert er.err(float(sc.maF1), ref["maF1"]) <= er.f1_tol(s["counts"], p.shape[1])
    # no target: NaN, as np.mean([])
    sens, cents = _t(f["sensitive"]), _t(f["centroids"])
    sc = mf.split_scores(p, y, sens, cents, [])
    assert torch.isnan(sc.fair_mean_diff) and sc.fair_terms.shape == (0, len(cents))
    # a row that matches no centroid: the fairness fields NaN, the F1 untouched
    bad = sens.clone()
    bad[5] = 9
    sc2 = mf.split_scores(p, y, bad, cents, _tables(f))
    assert torch.isnan(sc2.fair_mean_diff) and torch.isnan(sc2.fair_mean_sq)
    assert torch.isnan(sc2.fair_terms).all() and float(sc2.miF1) == float(sc.miF1)
    # N = 0
    sc0 = mf.split_scores(p[:0], y[:0], sens[:0], cents, _tables(f))
    assert torch.isnan(sc0.miF1) and torch.isnan(sc0.maF1) and torch.isnan(sc0.fair_mean_diff)
    assert sc0.counts.shape == (3, p.shape[1]) and sc0.gid.numel() == 0
    assert mf.split_scores(p[:0], y[:0]).fair_mean_diff is None
    # all-zero predictions and labels: 0 / 0 is NaN for miF1, maF1 is 0 (1e-6 keeps it finite)
    z = mf.split_scores(torch.zeros(4, 3), torch.zeros(4, 3))
    assert torch.isnan(z.miF1) and float(z.maF1) == 0.0
    with pytest.raises(ValueError):
        mf.split_scores(p, y, tables=_tables(f))
    with pytest.raises(ValueError):
        mf.split_scores(p, y[:, :3])


def test_eval_lanes_and_slices_rule():
    assert [mf.eval_lanes(L) for L in (1, 2, 3, 25, 32, 33, 64, 257)] == [1, 2, 4, 32, 32, 64, 64, 64]


def test_split_eval_host_checks():
    """mpv_split_eval's workspace sizing and argument checks run on the host and
    reject bad calls before any launch (csrc/evalsplit.hip)."""
    lib = H.load_library()
    wsb = lib.mpv_split_eval_workspace_bytes
    assert wsb(0, 25, 1, 2, 1) == 0 and wsb(1 << 31, 25, 1, 2, 1) == 0
    assert wsb(10, 0, 1, 2, 1) == 0 and wsb(10, 4097, 1, 2, 1) == 0
    assert wsb(10, 25, -1, 2, 1) == 0 and wsb(10, 25, 1, 0, 1) == 0 and wsb(10, 25, 1, 65536, 1) == 0
    assert wsb(10, 25, 1, 2, 0) == 0 and wsb(10, 25, 1, 2, 65536) == 0
    need = wsb(10, 25, 2, 3, 4)
    assert need > wsb(10, 25, 0, 3, 4) > 0 and wsb(10, 4096, 0, 1, 1) > 0
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks

    def args(**kw):
        base = dict(pred=fake, target=fake, w=fake, order=fake, goff=fake, N=10, L=25, T=2, G=3,
                    R=4, counts=fake, terms=fake, out=fake)
        base.update(kw)
        return H.SplitEvalArgs(**base)

    def run(a, ws=fake, n=need):
        return lib.mpv_split_eval(ctypes.byref(a), ws, n, None)

    assert run(args(N=0)) == H.EINVAL and b"shape" in lib.mpv_last_error()
    assert run(args(L=4097)) == H.EINVAL and b"shape" in lib.mpv_last_error()
    assert run(args(L=0)) == H.EINVAL and run(args(T=-1)) == H.EINVAL
    assert run(args(G=0)) == H.EINVAL and run(args(G=65536)) == H.EINVAL
    assert run(args(R=0)) == H.EINVAL and b"R must be" in lib.mpv_last_error()
    assert run(args(R=65536)) == H.EINVAL
    assert run(args(pred=None)) == H.EINVAL and run(args(target=None)) == H.EINVAL
    assert run(args(goff=None)) == H.EINVAL and b"goff" in lib.mpv_last_error()
    assert run(args(w=None)) == H.EINVAL and b"NULL w" in lib.mpv_last_error()
    assert run(args(terms=None)) == H.EINVAL
    assert run(args(counts=None)) == H.EINVAL and run(args(out=None)) == H.EINVAL
    assert run(args(), n=need - 1) == H.EINVAL and b"workspace" in lib.mpv_last_error()
    assert run(args(), ws=None) == H.EINVAL
    assert lib.mpv_split_eval(None, fake, need, None) == H.EINVAL


# ------------------------------------------------------------------ EvalPass
L_, Z_, D_, F_, S_ = 25, 10, 8, 20, 16


def _vae_args(**kw):
    a = argparse.Namespace(feature_dim=F_, latent_dim=D_, label_dim=L_, z_dim=Z_, keep_prob=0.5,
                           scale_coeff=1.0, residue_sigma="", mode="test", n_train_sample=4,
                           n_test_sample=S_, nll_coeff=0.1, c_coeff=200.0)
    a.__dict__.update(kw)
    return a


@pytest.fixture(scope="module")
def split():
    """A 300-row split with three sensitive groups and two target tables."""
    rng = np.random.default_rng(17)
    y = (rng.random((300, L_)) < 0.3).astype(np.float32)
    y[150:] = y[:150]
    x = rng.standard_normal((300, F_)).astype(np.float32)
    sens = np.stack([rng.integers(0, 3, 300), np.ones(300, np.int64)], 1)
    keys = sorted({"".join(r.astype(int).astype(str)) for r in y})
    dists = [{k: np.float64(rng.uniform(0.05, 1.0)) for k in keys if rng.random() < 0.7}
             for _ in range(2)]
    torch.manual_seed(3)
    np.random.seed(3)
    args = _vae_args()
    model = mpvae.VAE(args)
    return dict(y=torch.from_numpy(y), x=torch.from_numpy(x), sens=torch.from_numpy(sens),
                cents=torch.from_numpy(np.unique(sens, axis=0)), dists=dists, model=model,
                args=args)


def _hand_loop(model, args, y, x, B):
    """The reference's loop (fairsoft_evaluate.py:55-81) written by hand."""
    rows = []
    with torch.no_grad():
        for i in range(len(y) // B + 1):
            yb, xb = y[i * B:min((i + 1) * B, len(y))], x[i * B:min((i + 1) * B, len(y))]
            if len(yb) == 0:
                continue
            out = model(yb, xb)
            rows.append(mpvae.compute_loss(yb, *out, model.r_sqrt_sigma, args)[6])
    return torch.cat(rows)


@pytest.mark.parametrize("N", [300, 256, 5])
@pytest.mark.parametrize("was_training", [True, False])
def test_eval_pass_on_the_cpu(split, N, was_training):
    """Two full batches plus a tail, an exact multiple, a tail only."""
    d = split
    model, args = d["model"], d["args"]
    y, x, sens = d["y"][:N], d["x"][:N], d["sens"][:N]
    tables = [mf.LabelDistanceTable(t, L_, "cpu") for t in d["dists"]]
    model.eval()
    torch.manual_seed(11)
    want = _hand_loop(model, args, y, x, 128)
    model.train(was_training)
    ev = ms.EvalPass(model, args, 128, tables=tables, centroids=d["cents"])
    torch.manual_seed(11)
    out = ev.run(y, x, sens)
    assert model.training == was_training
    assert out.indiv_prob.shape == (N, L_) and out.indiv_prob.dtype == torch.float32
    assert torch.equal(out.indiv_prob, want)
    sc = mf.split_scores(out.indiv_prob, y, sens, d["cents"], tables)
    for k in ("miF1", "maF1", "fair_mean_diff", "fair_mean_sq", "fair_terms", "counts", "gid"):
        a, b = getattr(out.scores, k), getattr(sc, k)
        assert torch.equal(a, b) or (torch.isnan(a) & torch.isnan(b)).all(), k
    res = ev.read(out)
    assert set(res) == {"fair_mean_diff", "miF1", "maF1"}
    assert all(type(v) is float for v in res.values())
    assert res["miF1"] == float(sc.miF1) and res["fair_mean_diff"] == float(sc.fair_mean_diff)
    # against the restatement, from the same buffer
    w = er.weights(y.numpy().astype(np.int64), d["dists"])
    gid = er.group_of(sens.numpy(), d["cents"].numpy())
    ref = er.scores(want.numpy(), y.numpy(), w, gid, 3)
    s = er.order_sensitivity(want.numpy(), y.numpy(), w, gid, 3)
    assert er.err(res["fair_mean_diff"], ref["fair_mean_diff"]) <= er.tol(s["fair"])
    assert er.err(res["miF1"], ref["miF1"]) <= er.f1_tol(s["counts"], L_)


def test_eval_pass_without_tables_and_label_free(split):
    d = split
    model, args = d["model"], d["args"]
    y, x = d["y"][:140], d["x"][:140]
    model.train()
    ev = ms.EvalPass(model, args, 128)
    torch.manual_seed(2)
    out = ev.run(y, x)
    res = ev.read(out)
    assert res["fair_mean_diff"] is None and type(res["miF1"]) is float and type(res["maF1"]) is float
    assert out.scores.fair_terms is None and model.training
    # label_free: the feature branch alone, batch by batch
    ev2 = ms.EvalPass(model, args, 128, label_free=True)
    torch.manual_seed(2)
    out2 = ev2.run(y, x)
    model.eval()
    torch.manual_seed(2)
    with torch.no_grad():
        want = torch.cat([model.predict_proba(x[:128], args), model.predict_proba(x[128:], args)])
    assert torch.equal(out2.indiv_prob, want)
    # the weights' rows: weight_labels reaches split_scores
    tables = [mf.LabelDistanceTable(t, L_, "cpu") for t in d["dists"]]
    ev3 = ms.EvalPass(model, args, 128, tables=tables, centroids=d["cents"])
    torch.manual_seed(2)
    o3 = ev3.run(y, x, d["sens"][:140], weight_labels=d["y"][100:240])
    sc = mf.split_scores(o3.indiv_prob, y, d["sens"][:140], d["cents"], tables, d["y"][100:240])
    assert torch.equal(o3.scores.fair_mean_diff, sc.fair_mean_diff)
    own = mf.split_scores(o3.indiv_prob, y, d["sens"][:140], d["cents"], tables)
    assert not torch.equal(own.fair_mean_diff, sc.fair_mean_diff)
    with pytest.raises(ValueError):
        ms.EvalPass(model, args, 128, tables=tables)
    with pytest.raises(ValueError):
        ev3.run(y, x)
    with pytest.raises(ValueError):
        ev.capture(y, x)   # torch_cpu noise is drawn on the host
