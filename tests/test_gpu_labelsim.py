"""GPU: label_sim_kernel (mpv_label_sim_weights) and mpv_split_eval_defs at
their edges, and ``LabelSimilarity`` through every consumer of the row weights.

Shapes sit at the kernel's edges: L around the 64-label words (1, 2, 31 .. 65,
128, 129) and at the 4096 limit of the LDS row, B around the four rows of a
workgroup (1, 3, 4, 5, 257), T around the eight definitions of a launch (1, 8,
9).  Every (L, B), (L, T) and (B, T) pair occurs (55 cases, not the 165 of the
full product).

Tolerances.  Without gamma both sides form 0, 1 or the IEEE fp64 quotient of
two small integers: bit-equal.  With gamma the argument of ``exp`` is bit-equal
by construction (subtract, then multiply: nothing to contract), so the two
``exp`` implementations are the only difference.  Measured on the MI355X over
the 55 cases and both golden files (profiles/labelsim_errs.jsonl, recorded with
MPVAE_RECORD_ERRS set): at most EXP_ULPS_MEASURED ulp from the restatement and
from the reference's stored values; the bound is that plus 1 ulp, and may not
pass 4 ulp (two libraries that each claim about 1 ulp, doubled).  Everything
downstream of the weights is compared bit for bit.
"""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

import labelsim_ref as lr
import mpvae
import mpvae_fair as mf
import mpvae_hip as H
import mpvae_step as ms
from guarded_alloc import guard, same_bits
from tolerances import record_json

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXP_ULPS_MEASURED = 1
EXP_ULPS = EXP_ULPS_MEASURED + 1
assert EXP_ULPS <= 4

LS = [1, 2, 31, 32, 33, 63, 64, 65, 128, 129, 4096]
BS = [1, 3, 4, 5, 257]
TS = [1, 8, 9]
WEIGHT_CASES = [(L, B, TS[(i + j) % 3]) for i, L in enumerate(LS) for j, B in enumerate(BS)]
COMBOS = [(k, g) for k in lr.KINDS for g in (None, 0.01, 1.0, 10.0, -0.5)]


def test_the_weight_cases_cross_every_pair():
    assert {(L, B) for L, B, _ in WEIGHT_CASES} == {(L, B) for L in LS for B in BS}
    assert {(L, T) for L, _, T in WEIGHT_CASES} == {(L, T) for L in LS for T in TS}
    assert {(B, T) for _, B, T in WEIGHT_CASES} == {(B, T) for B in BS for T in TS}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _weight_case(L, B, T):
    """Labels (B, L) fp32 whose first rows are, rotated by the case so that
    B = 1 meets each of them at some L: target 0 itself, all-zero, all-one,
    target 0 with its last label flipped (a one-bit difference in the last
    word), a non-binary row and a NaN row; then random rows.  T targets and T
    (kind, gamma) pairs, rotated likewise so that all 20 occur."""
    n = LS.index(L) * len(BS) + BS.index(B)
    rng = np.random.default_rng([L, B, T])
    targets = (rng.random((T, L)) < 0.4).astype(np.uint8)
    t0 = targets[0].astype(np.float32)
    flip = t0.copy()
    flip[L - 1] = 1 - flip[L - 1]
    nonbin = t0.copy()
    nonbin[L // 2] = 2.0
    nan = t0.copy()
    nan[L - 1] = np.nan
    special = [t0, np.zeros(L, np.float32), np.ones(L, np.float32), flip, nonbin, nan]
    special = special[n % 6:] + special[:n % 6]
    rows = special + [(rng.random(L) < 0.4).astype(np.float32) for _ in range(max(0, B - 6))]
    y = np.stack(rows[:B])
    combos = [COMBOS[(n + t) % len(COMBOS)] for t in range(T)]
    return y, targets, combos


@pytest.mark.parametrize("L,B,T", WEIGHT_CASES)
def test_weights_at_the_kernel_edges(L, B, T):
    y, targets, combos = _weight_case(L, B, T)
    sims = [mf.LabelSimilarity(k, targets[t], L, DEV, gamma=g) for t, (k, g) in enumerate(combos)]
    w, count = mf.similarity_weights(_dev(y), sims)
    torch.cuda.synchronize()
    assert w.shape == (T, B) and w.dtype == torch.float64 and count.dtype == torch.int32
    got = w.cpu().numpy()
    worst = 0
    for t, (k, g) in enumerate(combos):
        want = lr.label_weights(k, targets[t], y, g)
        if g is None:
            assert np.array_equal(got[t], want), (k, t)
        else:
            d = lr.ulp_distance(got[t], want)
            worst = max(worst, d)
            print(f"L{L} B{B} T{T} t{t} {k} gamma {g}: {d} ulp")
            assert d <= EXP_ULPS, (k, g, d)
            clipped = (want == 0) | (want == 1)
            assert np.array_equal(got[t][clipped], want[clipped]), (k, g)
    assert int(count) == int((got > 0).sum())
    record_json(f"labelsim_weights_L{L}_B{B}_T{T}", {"max_ulp": worst})


@pytest.mark.parametrize("name", ["labelsim_s1_l25.npz", "labelsim_s2_l130.npz"])
def test_weights_against_the_reference_values(name):
    """Every (kind, gamma, target) of the golden files: 60 definitions, eight
    launches of the chunk loop."""
    z = np.load(os.path.join(GOLDEN, name))
    pats, targets = z["patterns"], z["targets"]
    L = pats.shape[1]
    defs = [(ki, gi, ti) for ki in range(4) for gi in range(len(z["gammas"]))
            for ti in range(len(targets))]
    gam = [None if g != g else float(g) for g in z["gammas"]]
    sims = [mf.LabelSimilarity(str(z["kinds"][ki]), targets[ti], L, DEV, gamma=gam[gi])
            for ki, gi, ti in defs]
    w, count = mf.similarity_weights(_dev(pats, torch.float32), sims)
    got = w.cpu().numpy()
    worst = 0
    for i, (ki, gi, ti) in enumerate(defs):
        want = z["values"][ki, gi, ti]
        if gam[gi] is None:
            assert np.array_equal(got[i], want), defs[i]
        else:
            d = lr.ulp_distance(got[i], want)
            worst = max(worst, d)
            assert d <= EXP_ULPS, (defs[i], d)
            clipped = (want == 0) | (want == 1)
            assert np.array_equal(got[i][clipped], want[clipped]), defs[i]
        assert sims[i].ref_dtype == (torch.float64 if z["np64"][ki, gi] else torch.float32)
    assert int(count) == int((got > 0).sum())
    print(f"{name}: max {worst} ulp from the reference's values")
    record_json(f"labelsim_golden_{name}", {"max_ulp": worst})


# ------------------------------------------------ downstream bit-equality
def _batch(B=33, L=25, seed=3):
    """A batch of 0/1 label rows with repeats, T = 3 similarity targets and,
    after a device round trip, tables that hold the very weights the kernel
    gave, keyed by the batch's patterns."""
    rng = np.random.default_rng(seed)
    pool = (rng.random((9, L)) < 0.35).astype(np.float32)
    y = pool[rng.integers(0, 9, B)]
    combos = [("jaccard", None), ("hamming", 10.0), ("jaccard", 1.0)]
    sims = [mf.LabelSimilarity(k, pool[t], L, DEV, gamma=g) for t, (k, g) in enumerate(combos)]
    w, _ = mf.similarity_weights(_dev(y), sims)
    wn = w.cpu().numpy()
    keys = ["".join(str(int(v)) for v in r) for r in y]
    tables = []
    for t, (k, g) in enumerate(combos):
        conv = float if g is None else np.float64      # the reference's value types
        tables.append(mf.LabelDistanceTable({key: conv(v) for key, v in zip(keys, wn[t])}, L, DEV))
    sens = np.stack([rng.integers(0, 3, B), np.ones(B, np.int64)], 1)     # three groups
    return dict(y=_dev(y), sims=sims, tables=tables, sens=_dev(sens),
                cents=_dev(np.unique(sens, axis=0)), rng=rng, B=B, L=L)


@pytest.fixture(scope="module")
def batch():
    return _batch()


def _source_lists(b):
    s, t = b["sims"], b["tables"]
    return {"similarities": s, "tables": t, "mixed": [s[0], t[1], s[2]],
            "mixed2": [t[0], s[1], s[2]]}


def test_label_weights_equal_the_tables(batch):
    ref_w, ref_c = mf.label_weights_batch(batch["y"], batch["tables"])
    assert int(ref_c) > 0
    for name, srcs in _source_lists(batch).items():
        for fn in (mf.label_weights, mf.label_weights_batch):
            w, c = fn(batch["y"], srcs)
            assert torch.equal(w, ref_w) and torch.equal(c, ref_c), (name, fn.__name__)
    for a, b in zip(batch["sims"], batch["tables"]):
        assert a.ref_dtype == b.ref_dtype


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("norm", ["l1", "l2"])
def test_fairness_penalty_equals_the_tables(batch, norm, fused):
    g = torch.Generator().manual_seed(5)
    lz0 = torch.rand(batch["B"], batch["L"], generator=g).to(DEV)
    fz0 = torch.rand(batch["B"], batch["L"], generator=g).to(DEV)

    def run(srcs):
        lz, fz = lz0.clone().requires_grad_(True), fz0.clone().requires_grad_(True)
        loss, count = mf.fairness_penalty(lz, fz, batch["y"], batch["sens"], srcs, norm, 1.5,
                                          max_groups=4, fused=fused)
        loss.backward()
        return loss.detach(), count, lz.grad, fz.grad

    lists = _source_lists(batch)
    want = run(lists["tables"])
    assert float(want[0]) > 0 and want[2].abs().sum() > 0
    for name in ("similarities", "mixed", "mixed2"):
        got = run(lists[name])
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a, b), name
    # the loss dtype rule: every source without gamma -> fp32
    s32 = [batch["sims"][0]]
    assert mf.fairness_penalty(lz0, fz0, batch["y"], batch["sens"], s32, norm, 1.5,
                               fused=fused)[0].dtype == torch.float32
    assert want[0].dtype == torch.float64


def test_calibration_loss_equals_the_tables(batch):
    g = torch.Generator().manual_seed(6)
    B, L, G = batch["B"], batch["L"], batch["cents"].shape[0]
    p = (torch.rand(B, L, generator=g) * 0.9 + 0.05).to(DEV)
    x0 = (torch.rand(1, L, G, generator=g) * 0.6 + 0.2).to(DEV)

    def run(srcs):
        x = x0.clone().requires_grad_(True)
        bce, fair, cal, active, count = mf.calibration_loss(p, x, batch["y"], batch["sens"],
                                                            batch["cents"], srcs, False, slices=2)
        (bce + 2.0 * fair).backward()
        return bce.detach(), fair.detach(), cal, active, count, x.grad

    lists = _source_lists(batch)
    want = run(lists["tables"])
    assert bool(want[3]) and float(want[1]) > 0
    for name in ("similarities", "mixed"):
        for a, b in zip(run(lists[name]), want):
            assert a.dtype == b.dtype and torch.equal(a, b), name
    a = mf.fair_mean_diff(p, batch["y"], batch["sens"], batch["cents"], lists["similarities"], 2)
    b = mf.fair_mean_diff(p, batch["y"], batch["sens"], batch["cents"], lists["tables"], 2)
    assert torch.equal(a, b) and float(a) > 0


# ----------------------------------------------------------- FairTrainStep
def _train_args(**kw):
    a = argparse.Namespace(feature_dim=40, latent_dim=8, label_dim=25, z_dim=10, keep_prob=0.0,
                           scale_coeff=1.0, residue_sigma="", n_train_sample=16, n_test_sample=16,
                           mode="train", nll_coeff=0.5, c_coeff=10.0, fair_coeff=2.0,
                           fairness_loss_norm="l2")
    a.__dict__.update(kw)
    return a


@pytest.mark.parametrize("T", [1, 3])
def test_fair_train_step_captured_replay_equals_eager(T):
    """C1-like shapes (B 32, L 25, z 10) with LabelSimilarity targets: replays
    of the captured step against eager steps from the same state, bit for bit,
    and the running sums."""
    B, L, F_ = 32, 25, 40
    g = torch.Generator().manual_seed(2)
    rng = np.random.default_rng(2)
    cents = np.array([[0, 0], [0, 1], [1, 0]], np.int64)
    batches = []
    for _ in range(3):
        y = (torch.rand(B, L, generator=g) < 0.3).float()
        y[:, 0], y[:, 1] = 1, 0
        batches.append((y.to(DEV), torch.randn(B, F_, generator=g).to(DEV),
                        torch.from_numpy(cents[rng.integers(0, 3, B)]).to(DEV)))
    combos = [("jaccard", 1.0), ("hamming", None), ("jaccard", None)][:T]
    targets = [batches[0][0][t].cpu() for t in range(T)]

    def make():
        a = _train_args(mpvae_noise="philox",
                        mpvae_seed=torch.tensor([99], dtype=torch.int64, device=DEV))
        torch.manual_seed(3)
        np.random.seed(3)
        m = mpvae.VAE(a).to(DEV).train()
        m.reparam_noise = torch.zeros_like
        o = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5, fused=True,
                             capturable=True)
        sims = [mf.LabelSimilarity(k, tg, L, DEV, gamma=gm) for (k, gm), tg in zip(combos, targets)]
        return m, ms.FairTrainStep(m, o, a, sims, max_groups=4)

    mg, tg = make()
    me, te = make()
    tg.capture(*batches[0], warmup=1)
    te(*batches[0])
    for batch in batches[1:]:
        og = [o.clone() for o in tg(*batch)]
        oe = te(*batch)
        torch.cuda.synchronize()
        assert float(oe.fairloss) > 0 and int(oe.contributed) > 0
        for name, a, b in zip(oe._fields, og, oe):
            assert same_bits(a, b.detach()), name
    for (k, a), b in zip(mg.state_dict().items(), me.state_dict().values()):
        assert same_bits(a, b), k
    tot_g, tot_e = tg.read_totals(), te.read_totals()
    assert tot_g["steps"] == tot_e["steps"] == 3 and tot_g["updates"] == tot_e["updates"] == 3
    assert tot_g == tot_e


# -------------------------------------------------------- split_scores_defs
DEF_CASES = [(1, 1, 1, 1, 1), (257, 25, 4, 11, 1), (300, 33, 3, 2, 3), (1030, 130, 2, 3, 5)]


def _defs_case(N, L, G, D, T):
    rng = np.random.default_rng([N, L, G, D, T])
    pool = (rng.random((12, L)) < 0.4).astype(np.float32)
    y = pool[rng.integers(0, 12, N)]
    p = rng.uniform(0.0, 1.0, (N, L)).astype(np.float32)
    sens = rng.integers(0, G, (N, 1))
    sens[:G, 0] = np.arange(G)[:N]
    defs = []
    for d in range(D):
        combos = [COMBOS[(3 * d + t) % len(COMBOS)] for t in range(T)]
        defs.append([mf.LabelSimilarity(k, pool[(d + t) % 12], L, DEV, gamma=g)
                     for t, (k, g) in enumerate(combos)])
    return _dev(p), _dev(y), _dev(sens), _dev(np.arange(G).reshape(G, 1)), defs, pool


def _absent(L, pool):
    """A pattern no row holds: its indication is 0 for every row."""
    for seed in range(100):
        r = (np.random.default_rng(seed).random(L) < 0.5).astype(np.float32)
        if not (pool == r).all(1).any():
            return r
    raise AssertionError("no absent pattern")


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("N,L,G,D,T", DEF_CASES)
def test_split_scores_defs_equal_one_call_per_definition(N, L, G, D, T, slices):
    p, y, sens, cents, defs, pool = _defs_case(N, L, G, D, T)
    dead = None
    if D >= 3 and L > 1:  # a definition with no active term, between live neighbours
        dead = 1
        defs[1] = [mf.LabelSimilarity("indication", _absent(L, pool), L, DEV) for _ in range(T)]
    sc = mf.split_scores_defs(p, y, sens, cents, defs, slices=slices)
    torch.cuda.synchronize()
    assert sc.fair_mean_diff.shape == (D,) and sc.fair_mean_sq.shape == (D,)
    assert sc.fair_terms.shape == (D, T, G)
    for d, one in enumerate(defs):
        ref = mf.split_scores(p, y, sens, cents, one, slices=slices)
        for k in ("fair_mean_diff", "fair_mean_sq", "fair_terms"):
            assert same_bits(getattr(sc, k)[d], getattr(ref, k)), (d, k)
        for k in ("miF1", "maF1", "counts", "gid"):
            assert same_bits(getattr(sc, k), getattr(ref, k)), (d, k)
        if d == dead:
            assert torch.isnan(sc.fair_mean_diff[d]) and torch.isnan(sc.fair_terms[d]).all()
    live = [d for d in range(D) if d != dead]
    if N > 1:
        assert not torch.isnan(sc.fair_mean_diff[live]).any()


# ----------------------------------------------------------------- EvalPass
def test_eval_pass_with_definitions():
    L, Z, F_, S, B = 25, 10, 20, 16, 128
    rng = np.random.default_rng(17)
    y = (rng.random((300, L)) < 0.3).astype(np.float32)
    y[150:] = y[:150]
    x = rng.standard_normal((300, F_)).astype(np.float32)
    sens = np.stack([rng.integers(0, 3, 300), np.ones(300, np.int64)], 1)
    yd, xd, sd, cents = _dev(y), _dev(x), _dev(sens), _dev(np.unique(sens, axis=0))

    def args(seed):
        return argparse.Namespace(feature_dim=F_, latent_dim=8, label_dim=L, z_dim=Z, keep_prob=0.5,
                                  scale_coeff=1.0, residue_sigma="", mode="test", n_train_sample=4,
                                  n_test_sample=S, nll_coeff=0.1, c_coeff=200.0,
                                  mpvae_noise="philox", mpvae_seed=seed)

    torch.manual_seed(3)
    np.random.seed(3)
    model = mpvae.VAE(args(None)).to(DEV).eval()
    model.reparam_noise = torch.zeros_like
    # the sweep of evaluate_models_over_label_distances: nine gammas, indication, constant
    sweep = [("jaccard", g) for g in (0.01, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0)] + \
        [("indication", None), ("constant", None)]
    defs = [[mf.LabelSimilarity(k, y[t], L, DEV, gamma=g) for t in (0, 7)] for k, g in sweep]
    key = 4242
    seed = torch.tensor([key], dtype=torch.int64, device=DEV)
    ev = ms.EvalPass(model, args(seed), B, definitions=defs, centroids=cents)
    out = ev.run(yd, xd, sd)
    res = ev.read(out)
    assert isinstance(res["fair_mean_diff"], list) and len(res["fair_mean_diff"]) == 11
    assert all(type(v) is float and v == v for v in res["fair_mean_diff"])
    assert type(res["miF1"]) is float and type(res["maF1"]) is float
    for d in (0, 6, 9, 10):  # the tables pass under the same seed, definition by definition
        seed1 = torch.tensor([key], dtype=torch.int64, device=DEV)
        one = ms.EvalPass(model, args(seed1), B, tables=defs[d], centroids=cents)
        o = one.run(yd, xd, sd)
        assert torch.equal(o.indiv_prob, out.indiv_prob)
        assert same_bits(o.scores.fair_mean_diff, out.scores.fair_mean_diff[d])
        assert same_bits(o.scores.fair_terms, out.scores.fair_terms[d])
        assert one.read(o)["fair_mean_diff"] == res["fair_mean_diff"][d]
        assert one.read(o)["miF1"] == res["miF1"]
    # captured: two full batches replayed, the tail and the scoring eager
    seed_g = torch.tensor([7], dtype=torch.int64, device=DEV)
    cap = ms.EvalPass(model, args(seed_g), B, definitions=defs, centroids=cents)
    cap.capture(yd, xd, warmup=1)
    seed_g.fill_(key)
    got = cap.run(yd, xd, sd)
    torch.cuda.synchronize()
    assert cap.graph is not None and int(seed_g) == key + 3
    assert torch.equal(got.indiv_prob, out.indiv_prob)
    for k in ("miF1", "maF1", "fair_mean_diff", "fair_mean_sq", "fair_terms", "counts", "gid"):
        assert same_bits(getattr(got.scores, k), getattr(out.scores, k)), k
    with pytest.raises(ValueError):
        ms.EvalPass(model, args(seed), B, tables=defs[0], definitions=defs, centroids=cents)


# -------------------------------------------------------------- guard bands
def _guarded_sims(alloc, sims):
    for s in sims:
        s.target = alloc(s.target)
    return sims


def _both(monkeypatch, run, min_buffers, what):
    plain = run(lambda t, role="input": t.detach().clone())
    torch.cuda.synchronize()
    g = guard(monkeypatch, mf, device=DEV)
    got = run(g.alloc_like)
    rep = g.check()
    n_product = sum(1 for r in g.records if not r.own)
    print(f"{what}: {rep.n_buffers} arenas ({n_product} the wrapper's), {rep.n_bad_bytes} bad bytes")
    assert rep.n_bad_bytes == 0, (what, rep)
    assert n_product >= min_buffers, (what, n_product)
    assert set(got) == set(plain)
    assert not [k for k in got if not same_bits(got[k], plain[k])], what


@pytest.mark.parametrize("L,B,T", [(1, 1, 1), (65, 5, 9), (129, 257, 8), (4096, 3, 9)])
def test_similarity_weights_under_guard_bands(L, B, T, monkeypatch):
    y, targets, combos = _weight_case(L, B, T)

    def run(alloc):
        sims = _guarded_sims(alloc, [mf.LabelSimilarity(k, targets[t], L, DEV, gamma=g)
                                     for t, (k, g) in enumerate(combos)])
        w, count = mf.similarity_weights(alloc(_dev(y)), sims)
        return {"w": w, "count": count}

    _both(monkeypatch, run, 2, f"similarity_weights L{L} B{B} T{T}")     # w, count


@pytest.mark.parametrize("N,L,G,D,T", DEF_CASES[1:])
def test_split_scores_defs_under_guard_bands(N, L, G, D, T, monkeypatch):
    p, y, sens, cents, defs, _ = _defs_case(N, L, G, D, T)

    def run(alloc):
        for d in defs:
            _guarded_sims(alloc, d)
        sc = mf.split_scores_defs(alloc(p), alloc(y), alloc(sens), alloc(cents), defs, slices=3)
        return {k: getattr(sc, k) for k in sc._fields}

    # w, count; the layout's counts, goff; ws, counts, out, out_defs, terms
    _both(monkeypatch, run, 9, f"split_scores_defs N{N} L{L} G{G} D{D} T{T}")


# ------------------------------------------------------------ bad arguments
def test_bad_arguments_surface_as_mpv_errors():
    lib = H.load_library()
    sim0 = mf.LabelSimilarity("jaccard", [], 0, DEV)
    with pytest.raises(H.MPVError, match="label_dim"):
        mf.similarity_weights(torch.zeros((3, 0), device=DEV), [sim0])                    # L = 0
    big = mf.LabelSimilarity("hamming", np.zeros(4097), 4097, DEV)
    with pytest.raises(H.MPVError, match="4096"):
        mf.similarity_weights(torch.zeros((3, 4097), device=DEV), [big])                  # L > 4096
    with pytest.raises(H.MPVError):
        mf.similarity_weights(torch.zeros((3, 25), device=DEV), [])                       # T = 0
    p, y, sens, cents, defs, _ = _defs_case(*DEF_CASES[2])
    with pytest.raises(H.MPVError, match="definitions"):
        mf.split_scores_defs(p, y, sens, cents, [])                                       # D = 0
    # an unknown kind and a NULL target stop in the host checks too
    w = torch.full((1, 3), -7.0, dtype=torch.float64, device=DEV)
    count = torch.zeros((), dtype=torch.int32, device=DEV)
    yy = torch.zeros((3, 25), device=DEV)
    ok = mf.LabelSimilarity("jaccard", np.zeros(25), 25, DEV)
    for s in (H.LabelSim(H.ptr(ok.target), 7, 0, 0.0, 0.0, 1.0), H.LabelSim(None, 0, 0, 0.0, 0.0, 1.0)):
        arr = (H.LabelSim * 1)(s)
        assert lib.mpv_label_sim_weights(H.ptr(yy), 3, 25, arr, 1, H.ptr(w), H.ptr(count),
                                         None) == H.EINVAL
    torch.cuda.synchronize()
    assert (w == -7.0).all() and int(count) == 0      # nothing was launched
