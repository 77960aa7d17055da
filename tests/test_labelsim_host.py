"""CPU: the closed-form label similarities.  The numpy restatement
(tests/labelsim_ref.py) against the reference's own stored values
(tests/golden/make_golden_labelsim.py), ``mpvae_fair.similarity_weights`` on CPU
tensors against both, ``LabelSimilarity`` beside ``LabelDistanceTable`` and
``split_scores_defs`` against one ``split_scores`` per definition.

Tolerances.  Without gamma every value is 0, 1 or the IEEE fp64 quotient of two
small integers on both sides: exact equality.  With gamma the restatement runs
numpy's own ``np.clip(np.exp(gamma * (sim - 1)))`` on a bit-equal argument:
exact again.  The torch path evaluates the same expression with torch's ``exp``:
two libraries that each claim about 1 ulp, so at most 4 ulp (measured here: 0).
"""
import os

import numpy as np
import pytest
import torch

import labelsim_ref as lr
import mpvae_fair as mf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ["labelsim_s1_l25.npz", "labelsim_s2_l130.npz"]
EXP_ULPS = 4


def load(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: z[k] for k in z.files}


FIX = {n: load(n) for n in FILES}


def gamma_of(g):
    return None if g != g else float(g)


def cases(f):
    for ki, kind in enumerate(f["kinds"]):
        for gi, g in enumerate(f["gammas"]):
            for ti, tgt in enumerate(f["targets"]):
                yield str(kind), gamma_of(g), tgt, f["values"][ki, gi, ti], bool(f["np64"][ki, gi])


def key_of(row):
    return "".join(str(int(v)) for v in row)


def test_the_goldens_hold_what_the_issue_lists():
    assert sum(os.path.getsize(os.path.join(GOLDEN, n)) for n in FILES) < 100_000
    s1, s2 = FIX[FILES[0]], FIX[FILES[1]]
    assert s1["patterns"].shape == (40, 25) and s1["targets"].shape == (3, 25)
    assert s2["patterns"].shape[1] == 130 and s2["targets"].shape == (3, 130)
    # s2: beside all-zero, all-one and a complement, the patterns differ in word 2 only
    assert (s2["patterns"][:4, :128] == s2["patterns"][0, :128]).all()
    assert len({key_of(r[128:]) for r in s2["patterns"][:4]}) == 4
    for f in (s1, s2):
        L = f["patterns"].shape[1]
        assert list(f["kinds"]) == lr.KINDS
        g = f["gammas"]
        assert np.isnan(g[0]) and set(g[1:4]) == {0.01, 1.0, 10.0} and (g[1:] < 0).sum() == 1
        assert not f["targets"][1].any()                       # the all-zero target
        assert (f["patterns"].sum(1) == 0).any() and (f["patterns"].sum(1) == L).any()
        assert ((f["patterns"] & f["targets"][0]).sum(1) == 0).any()   # disjoint from target 0
        # Python floats without gamma, numpy float64 with
        assert (f["np64"][:, 0] == 0).all() and (f["np64"][:, 1:] == 1).all()
        # the negative gamma makes the clip act: nothing above 1
        assert f["values"].max() == 1.0 and (f["values"][2:, 4] == 1.0).any()


@pytest.mark.parametrize("name", FILES)
def test_restatement_equals_the_reference_values(name):
    f = FIX[name]
    for kind, gamma, tgt, want, _ in cases(f):
        got = lr.weights(kind, tgt, f["patterns"], gamma)
        assert np.array_equal(got, want), (kind, gamma)


@pytest.mark.parametrize("name", FILES)
def test_similarity_weights_on_cpu_tensors(name):
    f = FIX[name]
    L = f["patterns"].shape[1]
    y = torch.from_numpy(f["patterns"].astype(np.float32))
    worst = 0
    for kind, gamma, tgt, want, np64 in cases(f):
        sim = mf.LabelSimilarity(kind, tgt, L, "cpu", gamma=gamma)
        assert sim.ref_dtype == (torch.float64 if np64 else torch.float32), (kind, gamma)
        w, count = mf.similarity_weights(y, [sim])
        assert w.dtype == torch.float64 and w.shape == (1, len(y)) and count.dtype == torch.int32
        assert int(count) == int((want > 0).sum())
        got = w[0].numpy()
        if gamma is None:
            assert np.array_equal(got, want), (kind,)
        else:
            d = lr.ulp_distance(got, want)
            worst = max(worst, d)
            assert d <= EXP_ULPS, (kind, gamma, d)
            assert np.array_equal(got[(want == 0) | (want == 1)], want[(want == 0) | (want == 1)])
        assert lr.ulp_distance(got, lr.weights(kind, tgt, f["patterns"], gamma)) <= EXP_ULPS
    print(f"{name}: torch exp against the reference's values, max {worst} ulp")


def test_targets_as_strings_vectors_and_tensors_agree():
    f = FIX[FILES[0]]
    tgt = f["targets"][0]
    y = torch.from_numpy(f["patterns"].astype(np.float32))
    a = mf.LabelSimilarity("jaccard", key_of(tgt), 25, "cpu")
    b = mf.LabelSimilarity("jaccard", tgt.tolist(), 25, "cpu")
    c = mf.LabelSimilarity("jaccard", torch.from_numpy(tgt).float(), 25, "cpu")
    assert a.key == b.key == c.key and torch.equal(a.target, b.target)
    ws = mf.similarity_weights(y, [a, b, c])[0]
    assert torch.equal(ws[0], ws[1]) and torch.equal(ws[0], ws[2])
    assert a.target.dtype == torch.int64 and a.target.numel() == 1 and a.W == 1
    assert mf.LabelSimilarity("hamming", np.zeros(130), 130, "cpu").target.numel() == 3


@pytest.mark.parametrize("name", FILES)
def test_equal_to_tables_built_from_the_reference_dicts(name):
    """A LabelDistanceTable from the golden dict (the reference's stored
    values, Python floats or numpy float64 as recorded) looks up what the
    closed form computes, for rows taken from the dict's patterns."""
    f = FIX[name]
    L = f["patterns"].shape[1]
    keys = [key_of(r) for r in f["patterns"]]
    y = torch.from_numpy(f["patterns"].astype(np.float32))
    for kind, gamma, tgt, want, np64 in cases(f):
        conv = np.float64 if np64 else float
        tab = mf.LabelDistanceTable({k: conv(v) for k, v in zip(keys, want)}, L, "cpu")
        sim = mf.LabelSimilarity(kind, tgt, L, "cpu", gamma=gamma)
        assert tab.ref_dtype == sim.ref_dtype
        wt = mf._table_weights_host(y, [tab])[0].numpy()
        ws = mf.similarity_weights(y, [sim])[0][0].numpy()
        assert np.array_equal(wt, want)
        if gamma is None:
            assert np.array_equal(ws, wt), (kind,)
        else:
            assert lr.ulp_distance(ws, wt) <= EXP_ULPS, (kind, gamma)
        # a mixed list on the host: each source fills its own rows
        mixed = mf._weights_host(y, [sim, tab, sim])
        assert np.array_equal(mixed[1].numpy(), wt) and np.array_equal(mixed[0].numpy(), ws)
        assert torch.equal(mixed[0], mixed[2])


def test_rows_without_a_binary_key_and_truncation():
    L = 25
    f = FIX[FILES[0]]
    y = f["patterns"][:6].astype(np.float32)
    y[1, 3] = 2.0            # not binary
    y[2, 0] = np.nan         # NaN
    y[3, 24] = -1.0          # int() is -1
    y[4] = np.where(y[4] == 1, 1.75, 0.5)     # trunc: 1.75 counts as 1, 0.5 as 0
    y[5] = np.where(y[5] == 1, 1.0, -0.25)    # -0.25 truncates to -0: a 0
    sims = [mf.LabelSimilarity(k, f["targets"][0], L, "cpu", gamma=g)
            for k in lr.KINDS for g in (None, 1.0)]
    w, count = mf.similarity_weights(torch.from_numpy(y), sims)
    assert (w[:, 1:4] == 0).all()
    clean = torch.from_numpy(f["patterns"][:6].astype(np.float32))
    w0, _ = mf.similarity_weights(clean, sims)
    assert torch.equal(w[:, [0, 4, 5]], w0[:, [0, 4, 5]])
    assert int(count) == int((w > 0).sum())
    for i, s in enumerate(sims):
        ref = lr.label_weights(s.kind, f["targets"][0], y, s.gamma)
        assert lr.ulp_distance(w[i].numpy(), ref) <= (0 if s.gamma is None else EXP_ULPS)
    # the constant kind still gives 0 for such a row, as the dict miss does
    assert w[2, 1] == 0 and w[2, 0] == 1


def _same(a, b):
    """Equal, with NaN at the same places."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _split(N=60, L=25, seed=5):
    rng = np.random.default_rng(seed)
    f = FIX[FILES[0]]
    y = f["patterns"][rng.integers(0, len(f["patterns"]), N)].astype(np.float32)
    p = rng.uniform(0.01, 0.99, (N, L)).astype(np.float32)
    sens = rng.integers(0, 3, (N, 1))
    return (torch.from_numpy(p), torch.from_numpy(y), torch.from_numpy(sens),
            torch.from_numpy(np.unique(sens, axis=0)), f)


def _definitions(f, L, dev="cpu"):
    """Four definitions of two targets each; the last has no active term (an
    indication of patterns no row holds is 0 everywhere)."""
    t0, t2 = f["targets"][0], f["targets"][2]
    absent = np.ones(L, np.uint8)
    absent[::2] = 0
    mk = lambda kind, t, g=None: mf.LabelSimilarity(kind, t, L, dev, gamma=g)
    return [[mk("jaccard", t0), mk("jaccard", t2)],
            [mk("hamming", t0, 10.0), mk("hamming", t2, 10.0)],
            [mk("constant", t0), mk("indication", t0)],
            [mk("indication", absent), mk("indication", absent)]]


def test_split_scores_defs_on_cpu_tensors():
    p, y, sens, cents, f = _split()
    defs = _definitions(f, 25)
    assert not (y.numpy() == _definitions(f, 25)[3][0].target.numpy()).all(1).any()
    sc = mf.split_scores_defs(p, y, sens, cents, defs)
    D, T, G = 4, 2, len(cents)
    assert sc.fair_mean_diff.shape == (D,) and sc.fair_mean_sq.shape == (D,)
    assert sc.fair_terms.shape == (D, T, G) and sc.miF1.dim() == 0
    for d, one in enumerate(defs):
        ref = mf.split_scores(p, y, sens, cents, one)
        for k in ("fair_mean_diff", "fair_mean_sq", "fair_terms"):
            a, b = getattr(sc, k)[d], getattr(ref, k)
            assert _same(a, b), (d, k)
        for k in ("miF1", "maF1", "counts", "gid"):
            assert torch.equal(getattr(sc, k), getattr(ref, k)), k
    assert torch.isnan(sc.fair_mean_diff[3]) and not torch.isnan(sc.fair_mean_diff[:3]).any()
    # tables and similarities in one definition; weight_labels reaches the weights
    keys = [key_of(r) for r in f["patterns"]]
    tab = mf.LabelDistanceTable({k: float(v) for k, v in zip(keys, f["values"][2, 0, 0])}, 25, "cpu")
    a = mf.split_scores_defs(p, y, sens, cents, [[tab, defs[0][1]]])
    assert _same(a.fair_terms[0], sc.fair_terms[0])
    b = mf.split_scores_defs(p, y, sens, cents, defs[:1], weight_labels=y.flip(0))
    want = mf.split_scores(p, y, sens, cents, defs[0], weight_labels=y.flip(0))
    assert torch.equal(b.fair_mean_diff[0], want.fair_mean_diff)
    assert not torch.equal(b.fair_mean_diff[0], sc.fair_mean_diff[0])
    # N = 0: NaN of the right shapes, no launch
    z = mf.split_scores_defs(p[:0], y[:0], sens[:0], cents, defs)
    assert z.fair_mean_diff.shape == (D,) and torch.isnan(z.fair_mean_diff).all()
    assert z.fair_terms.shape == (D, T, G)


def test_eval_pass_with_definitions_on_the_cpu():
    import argparse
    import mpvae
    import mpvae_step as ms
    p, y, sens, cents, f = _split(N=70)
    args = argparse.Namespace(feature_dim=12, latent_dim=8, label_dim=25, z_dim=10, keep_prob=0.5,
                              scale_coeff=1.0, residue_sigma="", mode="test", n_train_sample=4,
                              n_test_sample=8, nll_coeff=0.1, c_coeff=200.0)
    torch.manual_seed(3)
    np.random.seed(3)
    model = mpvae.VAE(args)
    x = torch.randn(70, 12)
    defs = _definitions(f, 25)
    ev = ms.EvalPass(model, args, 32, definitions=defs, centroids=cents)
    torch.manual_seed(9)
    out = ev.run(y, x, sens)
    res = ev.read(out)
    assert isinstance(res["fair_mean_diff"], list) and len(res["fair_mean_diff"]) == 4
    assert all(type(v) is float for v in res["fair_mean_diff"]) and type(res["miF1"]) is float
    for d, one in enumerate(defs[:3]):
        one_pass = ms.EvalPass(model, args, 32, tables=one, centroids=cents)
        torch.manual_seed(9)
        o = one_pass.run(y, x, sens)
        assert torch.equal(o.indiv_prob, out.indiv_prob)
        assert one_pass.read(o)["fair_mean_diff"] == res["fair_mean_diff"][d]
    assert np.isnan(res["fair_mean_diff"][3])
    with pytest.raises(ValueError):
        ms.EvalPass(model, args, 32, tables=defs[0], definitions=defs, centroids=cents)
    with pytest.raises(ValueError):
        ms.EvalPass(model, args, 32, definitions=defs)
    with pytest.raises(ValueError):
        ev.run(y, x)


def test_bad_arguments():
    f = FIX[FILES[0]]
    t = f["targets"][0]
    with pytest.raises(ValueError, match="unknown similarity kind"):
        mf.LabelSimilarity("cosine", t, 25, "cpu")
    with pytest.raises(ValueError, match="length 24"):
        mf.LabelSimilarity("jaccard", t, 24, "cpu")
    with pytest.raises(ValueError):
        mf.LabelSimilarity("jaccard", key_of(t) + "1", 25, "cpu")
    with pytest.raises(ValueError):
        mf.LabelSimilarity("jaccard", "2" * 25, 25, "cpu")
    with pytest.raises(ValueError, match="0/1"):
        mf.LabelSimilarity("jaccard", np.full(25, 0.5), 25, "cpu")
    sim = mf.LabelSimilarity("jaccard", t, 25, "cpu")
    with pytest.raises(ValueError, match="label_dim 25, labels have 24"):
        mf.similarity_weights(torch.zeros(3, 24), [sim])
    with pytest.raises(TypeError):
        mf.similarity_weights(torch.zeros(3, 25), [mf.LabelDistanceTable({}, 25, "cpu")])
    p, y, sens, cents, _ = _split()
    with pytest.raises(ValueError, match="same number of targets"):
        mf.split_scores_defs(p, y, sens, cents, [[sim, sim], [sim]])
    with pytest.raises(ValueError, match="label_dim"):
        mf.split_scores_defs(p, y, sens, cents, [[mf.LabelSimilarity("jaccard", [1, 0], 2, "cpu")]])
    with pytest.raises(ValueError):
        mf.split_scores_defs(p, y, None, None, [[sim]])
    with pytest.raises(ValueError):
        mf.split_scores_defs(p, y, sens, cents, [])
