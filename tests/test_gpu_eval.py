"""GPU: the evaluation pass (csrc/evalsplit.hip through mpvae_fair.split_scores
and mpvae_step.EvalPass) against the numpy fp64 restatement tests/eval_ref.py,
the reference's records (tests/golden/eval_*.npz), the calibration kernels as
an independent device peer, and the per-batch calls made by hand.

Tolerances.  The kernel and the restatement both sum in fp64 from the same
fp32 inputs, in different orders: a count, a term or a fairness mean may differ
from the restatement by 2^-52 plus four times s, the restatement's own
sensitivity to the order of the rows (eval_ref.tol, eval_ref.order_sensitivity:
the restatement on permuted rows against itself, no kernel involved); miF1 and
maF1, ratios of counts summed over the labels, by eval_ref.f1_tol.  Errors are
relative to the largest entry of the tensor.  Against the reference's records
the F1 bound is 4 N 2^-24 (its fp32 sums, tests/test_eval_host.py).  The
measured figures of every edge case go to $MPVAE_RECORD_ERRS
(profiles/split_eval_errs.jsonl).

Measured on the MI355X over the 40 edge cases: counts and miF1 equal the
restatement exactly (sums of fp32 values, which fp64 holds without rounding),
maF1 <= 2.5e-16, terms <= 2.2e-14 (the restatement's own s up to 5.1e-14),
fair_mean_diff <= 1.2e-15, fair_mean_sq <= 2.3e-15, and <= 1.6e-15 from the
calibration kernels' value.
"""
import argparse
import ctypes
import itertools

import numpy as np
import pytest
import torch

import eval_ref as er
import mpvae
import mpvae_fair as mf
import mpvae_hip as H
import mpvae_step as ms
from guarded_alloc import guard, same_bits
from tolerances import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------- 1. the kernel's edges
AXES = dict(L=[1, 25, 32, 33, 63, 64, 65, 257], N=[1, 7, 300, 4097], G=[1, 3, 17],
            T=[0, 1, 4, 5, 9], R=[1, 3, 64])


def pairwise_cover(axes):
    """A greedy pairwise-covering selection: every pair of values of two axes
    occurs in some case.  Deterministic."""
    names = list(axes)
    todo = {(a, va, b, vb) for a, b in itertools.combinations(names, 2)
            for va in axes[a] for vb in axes[b]}
    full = [dict(zip(names, v)) for v in itertools.product(*axes.values())]
    picked = []
    while todo:
        def gain(c):
            return sum((a, c[a], b, c[b]) in todo for a, b in itertools.combinations(names, 2))
        best = max(full, key=gain)
        picked.append(best)
        todo -= {(a, best[a], b, best[b]) for a, b in itertools.combinations(names, 2)}
    return picked


CASES = pairwise_cover(AXES)
CASE_IDS = ["L{L}_N{N}_G{G}_T{T}_R{R}".format(**c) for c in CASES]


def test_the_selection_covers_every_pair():
    assert 35 <= len(CASES) <= 60, len(CASES)
    for a, b in itertools.combinations(AXES, 2):
        assert {(c[a], c[b]) for c in CASES} == set(itertools.product(AXES[a], AXES[b]))
    # R larger than a group's rows, N past MPV_GROUP_MAX_B, T past a register
    # tile and past label_weights_batch's 8 tables, a NULL layout
    assert any(c["R"] == 64 and c["N"] <= 7 for c in CASES)
    assert any(c["N"] > H.GROUP_MAX_B for c in CASES) and any(c["T"] > 8 for c in CASES)
    assert any(c["G"] == 1 for c in CASES)


def make_case(L, N, G, T, R, seed=0):
    """Inputs of one edge case.  With G > 1 group 1 has no row; some
    probabilities are exactly 0, a few of them under a positive label (fn > 0);
    target 1 (when there are more than three) has no weight at all, and target
    0 has none in group 0 (when there is another group with rows)."""
    rng = np.random.default_rng([seed, L, N, G, T, R])
    pred = rng.random((N, L)).astype(np.float32)
    y = (rng.random((N, L)) < 0.3).astype(np.float32)
    pred[rng.random((N, L)) < 0.05] = 0.0
    groups = [k for k in range(G) if k != 1 or G == 1]
    gid = np.asarray(groups)[rng.integers(0, len(groups), N)]
    w = rng.uniform(0.05, 1.0, (T, N)) * (rng.random((T, N)) < 0.7)
    if T > 3:
        w[1] = 0.0
    if T and len(groups) > 1:
        w[0, gid == 0] = 0.0
    return dict(pred=pred, y=y, gid=gid, w=w, G=G, R=R)


def run_kernel(c, null_layout=False, R=None):
    """mpv_split_eval on the case: (counts, out, terms) device tensors."""
    p, y = _dev(c["pred"]), _dev(c["y"])
    w = _dev(c["w"]) if len(c["w"]) else None
    if null_layout:
        order = goff = None
    else:
        order, goff = mf._group_layout(_dev(c["gid"].astype(np.int32)), c["G"])
    return mf._split_eval(p, y, w, order, goff, c["G"], c["R"] if R is None else R)


def check_against_restatement(c, counts, out, terms, what):
    T, L = len(c["w"]), c["pred"].shape[1]
    ref = er.scores(c["pred"], c["y"], c["w"] if T else None, c["gid"], c["G"])
    s = er.order_sensitivity(c["pred"], c["y"], c["w"] if T else None, c["gid"], c["G"])
    out = out.cpu().numpy()
    errs = dict(counts=er.err(counts.cpu().numpy(), ref["counts"]), s_counts=s["counts"],
                miF1=er.err(out[0], ref["miF1"]), maF1=er.err(out[1], ref["maF1"]))
    bounds = dict(counts=er.tol(s["counts"]), miF1=er.f1_tol(s["counts"], L),
                  maF1=er.f1_tol(s["counts"], L))
    if T:
        errs.update(terms=er.err(terms.cpu().numpy(), ref["terms"]),
                    fair_mean_diff=er.err(out[2], ref["fair_mean_diff"]),
                    fair_mean_sq=er.err(out[3], ref["fair_mean_sq"]), s_fair=s["fair"])
        bounds.update({k: er.tol(s["fair"]) for k in ("terms", "fair_mean_diff", "fair_mean_sq")})
        assert out[4] == ref["nterms"], what
    else:
        assert terms is None and np.isnan(out[2]) and np.isnan(out[3]) and out[4] == 0, what
    print(what, {k: f"{v:.3g}" for k, v in errs.items()})
    record("split_eval_" + what, errs)
    for k, b in bounds.items():
        assert errs[k] <= b, (what, k, errs[k], b)
    return ref, s


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_split_eval_at_its_loop_edges(case):
    c = make_case(**case)
    what = "L{L}_N{N}_G{G}_T{T}_R{R}".format(**case)
    null = case["G"] == 1 and case["N"] % 2 == 1   # a NULL layout in half of the G = 1 cases
    counts, out, terms = run_kernel(c, null_layout=null)
    ref, s = check_against_restatement(c, counts, out, terms, what)
    # the same call again: the same bits
    c2, o2, t2 = run_kernel(c, null_layout=null)
    assert same_bits(counts, c2) and same_bits(out, o2) and same_bits(terms, t2)
    if case["G"] == 1:   # NULL order / goff against the explicit identity
        c3, o3, t3 = run_kernel(c, null_layout=not null)
        assert same_bits(counts, c3) and same_bits(out, o3) and same_bits(terms, t3)
    if case["T"]:
        # the mean of the squared distances against the calibration kernels,
        # an independent device peer (mf.fair_mean_diff's path)
        order, goff = mf._group_layout(_dev(c["gid"].astype(np.int32)), c["G"])
        peer, _, _ = mf._calib_fwd(_dev(c["pred"]), None, None, _dev(c["w"]), order, goff, c["G"],
                                   case["R"], False, False)
        peer = peer.cpu().numpy()
        assert peer[2] == out[4].item()
        if peer[2]:
            e = er.err(out[3].item(), peer[1] / peer[2])
            record("split_eval_peer_" + what, dict(fair_mean_sq=e))
            assert e <= er.tol(s["fair"]), (what, e)


def test_slices_agree_to_rounding_and_order_entries_out_of_range_are_skipped():
    c = make_case(25, 300, 3, 4, 1, seed=1)
    runs = [run_kernel(c, R=R) for R in (1, 2, 7, 64, 300)]
    s = er.order_sensitivity(c["pred"], c["y"], c["w"], c["gid"], c["G"])
    for counts, out, terms in runs[1:]:
        assert er.err(counts.cpu().numpy(), runs[0][0].cpu().numpy()) <= er.tol(s["counts"])
        assert er.err(terms.cpu().numpy(), runs[0][2].cpu().numpy()) <= er.tol(s["fair"])
    # rows 3 and 10 knocked out of `order`: the scores of the split without them
    order, goff = mf._group_layout(_dev(c["gid"].astype(np.int32)), c["G"])
    order = order.clone()
    drop = torch.isin(order, torch.tensor([3, 10], dtype=torch.int32, device=DEV))
    order[drop] = torch.tensor([-1, 300], dtype=torch.int32, device=DEV)
    counts, out, terms = mf._split_eval(_dev(c["pred"]), _dev(c["y"]), _dev(c["w"]), order, goff,
                                        c["G"], 3)
    keep = np.setdiff1d(np.arange(300), [3, 10])
    ref = er.scores(c["pred"][keep], c["y"][keep], c["w"][:, keep], c["gid"][keep], c["G"])
    assert er.err(counts.cpu().numpy(), ref["counts"]) <= er.tol(s["counts"])
    assert er.err(terms.cpu().numpy(), ref["terms"]) <= er.tol(s["fair"])


# ----------------------------------------------------------------- 2. NaN cases
def test_nan_cases():
    c = make_case(25, 64, 3, 2, 2, seed=2)
    c["w"][:] = 0.0   # no active term
    counts, out, terms = run_kernel(c)
    out = out.cpu().numpy()
    assert np.isnan(out[2]) and np.isnan(out[3]) and out[4] == 0 and np.isfinite(out[:2]).all()
    assert torch.isnan(terms).all()
    # a row with no centroid, through split_scores
    f = next(f for f in FIX if f["name"] == "e1_l25")
    sens = f["sensitive"].copy()
    sens[7] = 9
    sc = mf.split_scores(_dev(f["pred"]), _dev(f["labels"], torch.float32), _dev(sens),
                         _dev(f["centroids"]), _tables(f))
    assert torch.isnan(sc.fair_mean_diff) and torch.isnan(sc.fair_mean_sq)
    assert torch.isnan(sc.fair_terms).all() and torch.isfinite(sc.miF1) and torch.isfinite(sc.maF1)
    # N = 0: NaN without a launch
    H.load_library().mpv_timing_enable(1)
    H.load_library().mpv_timing_reset()
    try:
        s0 = mf.split_scores(_dev(f["pred"])[:0], _dev(f["labels"], torch.float32)[:0],
                             _dev(sens)[:0], _dev(f["centroids"]), _tables(f))
        assert not H.kernel_times()
    finally:
        H.load_library().mpv_timing_enable(0)
    assert torch.isnan(s0.miF1) and torch.isnan(s0.fair_mean_diff) and s0.miF1.is_cuda


# ------------------------------------------------------------ 3. bad arguments
def test_bad_arguments_launch_nothing():
    lib = H.load_library()
    c = make_case(25, 16, 2, 1, 2, seed=3)
    p, y, w = _dev(c["pred"]), _dev(c["y"]), _dev(c["w"])
    order, goff = mf._group_layout(_dev(c["gid"].astype(np.int32)), 2)
    need = lib.mpv_split_eval_workspace_bytes(16, 25, 1, 2, 2)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    counts = torch.full((3, 25), -7.0, dtype=torch.float64, device=DEV)
    terms = torch.full((1, 2), -7.0, dtype=torch.float64, device=DEV)
    out = torch.full((5,), -7.0, dtype=torch.float64, device=DEV)

    def call(nbytes=need, **kw):
        base = dict(pred=H.ptr(p), target=H.ptr(y), w=H.ptr(w), order=H.ptr(order),
                    goff=H.ptr(goff), N=16, L=25, T=1, G=2, R=2, counts=H.ptr(counts),
                    terms=H.ptr(terms), out=H.ptr(out))
        base.update(kw)
        a = H.SplitEvalArgs(**base)
        return lib.mpv_split_eval(ctypes.byref(a), H.ptr(ws), nbytes, H.stream_of(DEV))

    lib.mpv_timing_enable(1)
    lib.mpv_timing_reset()
    try:
        assert call(N=0) == H.EINVAL and b"shape" in lib.mpv_last_error()
        assert call(L=4097) == H.EINVAL and b"shape" in lib.mpv_last_error()
        assert call(R=0) == H.EINVAL and b"R must be" in lib.mpv_last_error()
        assert call(nbytes=need - 1) == H.EINVAL and b"workspace" in lib.mpv_last_error()
        assert not H.kernel_times()
    finally:
        lib.mpv_timing_enable(0)
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((terms == -7).all()) and bool((out == -7).all())
    assert not bool(ws.any())
    assert call() == 0   # and the good call runs
    torch.cuda.synchronize()
    assert not bool((out == -7).any())


# ---------------------------------------------------------------- 4. guard bands
@pytest.mark.parametrize("shape", [dict(L=25, N=300, G=3, T=5, R=3), dict(L=65, N=7, G=17, T=1, R=64),
                                   dict(L=257, N=4097, G=1, T=0, R=3)],
                         ids=["L25", "L65", "L257"])
def test_guard_bands(shape, monkeypatch):
    """counts, terms, out and the workspace between guard bands, the inputs
    registered: nothing stored past a buffer, no input changed, the same bits."""
    c = make_case(**shape)
    plain = run_kernel(c)
    torch.cuda.synchronize()
    g = guard(monkeypatch, mf, device=DEV)
    p, y = g.alloc_like(_dev(c["pred"])), g.alloc_like(_dev(c["y"]))
    w = g.alloc_like(_dev(c["w"])) if shape["T"] else None
    order, goff = mf._group_layout(_dev(c["gid"].astype(np.int32)), c["G"])
    order, goff = g.alloc_like(order), g.alloc_like(goff)
    got = mf._split_eval(p, y, w, order, goff, c["G"], c["R"])
    rep = g.assert_clean(min_buffers=4 if shape["T"] else 3, what=str(shape))
    print(shape, rep)
    for a, b in zip(got, plain):
        assert same_bits(a, b)


# ----------------------------------------------- 5. the records, through tables
FIX = er.eval_fixtures()


def _tables(f):
    return [mf.LabelDistanceTable(d, f["labels"].shape[1], DEV) for d in f["dists"]]


@pytest.mark.parametrize("f", FIX, ids=[f["name"] for f in FIX])
def test_split_scores_match_the_records(f):
    N, L = f["pred"].shape
    sc = mf.split_scores(_dev(f["pred"]), _dev(f["labels"], torch.float32), _dev(f["sensitive"]),
                         _dev(f["centroids"]), _tables(f), _dev(f["weight_labels"], torch.float32))
    w = er.weights(f["weight_labels"], f["dists"])
    gid = er.group_of(f["sensitive"], f["centroids"])
    s = er.order_sensitivity(f["pred"], f["labels"], w, gid, len(f["centroids"]))
    for k in ("miF1", "maF1"):
        v = getattr(sc, k)
        assert v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda
        assert abs(float(v) - float(f[k])) <= 4 * N * 2.0 ** -24 * abs(float(f[k])), k
    assert er.err(float(sc.fair_mean_diff), float(f["fair_mean_diff"])) <= er.tol(s["fair"])
    assert np.array_equal(sc.gid.cpu().numpy(), gid)
    assert sc.counts.shape == (3, L) and sc.fair_terms.shape == (len(f["dists"]), len(f["centroids"]))
    # the post-process variant from the existing entry point, on the same inputs
    peer = mf.fair_mean_diff(_dev(f["pred"]), _dev(f["weight_labels"], torch.float32),
                             _dev(f["sensitive"]), _dev(f["centroids"]), _tables(f))
    assert er.err(float(sc.fair_mean_sq), float(peer)) <= er.tol(s["fair"])
    # without tables: the reference's eval_fairness=False
    plain = mf.split_scores(_dev(f["pred"]), _dev(f["labels"], torch.float32))
    assert plain.fair_mean_diff is None and plain.fair_terms is None and plain.gid is None
    assert er.err(float(plain.miF1), float(sc.miF1)) <= er.f1_tol(s["counts"], L)


def test_split_scores_are_capturable():
    """No host sync: the whole call records into a HIP graph and replays."""
    f = next(f for f in FIX if f["name"] == "e1_l25")
    p, y = _dev(f["pred"]), _dev(f["labels"], torch.float32)
    sens, cents, tables = _dev(f["sensitive"]), _dev(f["centroids"]), _tables(f)
    eager = mf.split_scores(p, y, sens, cents, tables)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mf.split_scores(p, y, sens, cents, tables)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sc = mf.split_scores(p, y, sens, cents, tables)
    p.copy_(_dev(f["pred"]).flip(0))
    graph.replay()
    p.copy_(_dev(f["pred"]))
    graph.replay()
    torch.cuda.synchronize()
    for k in ("miF1", "maF1", "fair_mean_diff", "fair_mean_sq", "fair_terms", "counts"):
        assert same_bits(getattr(sc, k), getattr(eager, k)), k


# ------------------------------------------------------------------ 6. EvalPass
L_, Z_, D_, F_, S_, B_ = 25, 10, 8, 20, 16, 128
KEY = 4242


def _vae_args(**kw):
    a = argparse.Namespace(feature_dim=F_, latent_dim=D_, label_dim=L_, z_dim=Z_, keep_prob=0.5,
                           scale_coeff=1.0, residue_sigma="", mode="test", n_train_sample=4,
                           n_test_sample=S_, nll_coeff=0.1, c_coeff=200.0)
    a.__dict__.update(kw)
    return a


@pytest.fixture(scope="module")
def split():
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
    model = mpvae.VAE(_vae_args()).to(DEV)
    return dict(y=_dev(y), x=_dev(x), sens=_dev(sens), cents=_dev(np.unique(sens, axis=0)),
                tables=[mf.LabelDistanceTable(t, L_, DEV) for t in dists], model=model)


def _philox_args(seed):
    return _vae_args(mpvae_noise="philox", mpvae_seed=seed)


def _assert_scores_equal(a, b):
    for k in ("miF1", "maF1", "fair_mean_diff", "fair_mean_sq", "fair_terms", "counts", "gid"):
        assert same_bits(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("N", [300, 256, 5])
@pytest.mark.parametrize("label_free", [False, True])
def test_eval_pass_equals_the_batches_made_by_hand(split, N, label_free):
    """Philox noise from a device key: batch i draws with key KEY + i.  The
    hand loop passes that key as an int, batch by batch."""
    d = split
    model = d["model"].train()
    y, x, sens = d["y"][:N], d["x"][:N], d["sens"][:N]
    seed = torch.tensor([KEY], dtype=torch.int64, device=DEV)
    ev = ms.EvalPass(model, _philox_args(seed), B_, tables=d["tables"], centroids=d["cents"],
                     label_free=label_free)
    torch.cuda.manual_seed(5)
    out = ev.run(y, x, sens)
    assert model.training
    n_batches = -(-N // B_)
    assert int(seed) == KEY + n_batches   # every non-empty batch advanced the key once
    model.eval()
    torch.cuda.manual_seed(5)
    rows = []
    with torch.no_grad():
        for i in range(n_batches):
            yb, xb = y[i * B_:(i + 1) * B_], x[i * B_:(i + 1) * B_]
            a = _philox_args(KEY + i)
            rows.append(model.predict_proba(xb, a) if label_free
                        else mpvae.predict_proba(model(yb, xb)[3], model.r_sqrt_sigma, a))
    want = torch.cat(rows)
    assert out.indiv_prob.shape == (N, L_) and torch.equal(out.indiv_prob, want)
    _assert_scores_equal(out.scores, mf.split_scores(out.indiv_prob, y, sens, d["cents"],
                                                     d["tables"]))
    res = ev.read(out)
    assert all(type(v) is float for v in res.values()) and set(res) == {"fair_mean_diff", "miF1",
                                                                          "maF1"}
    assert res["fair_mean_diff"] == float(out.scores.fair_mean_diff)


@pytest.mark.parametrize("label_free", [False, True])
def test_captured_pass_returns_the_bits_of_the_eager_pass(split, label_free):
    """Two full batches replayed from the graph and an eager tail against the
    eager pass from the same key (the reparameterisation noise switched off, as
    in test_train_step_graph_replays_match_eager: torch's generator inside a
    graph is torch's business)."""
    d = split
    model = d["model"].eval()
    y, x, sens = d["y"], d["x"], d["sens"]
    noise, model.reparam_noise = model.reparam_noise, torch.zeros_like
    try:
        seed = torch.tensor([KEY], dtype=torch.int64, device=DEV)
        eager = ms.EvalPass(model, _philox_args(seed), B_, tables=d["tables"], centroids=d["cents"],
                            label_free=label_free)
        want = eager.run(y, x, sens)
        assert eager.graph is None
        seed_g = torch.tensor([7], dtype=torch.int64, device=DEV)
        ev = ms.EvalPass(model, _philox_args(seed_g), B_, tables=d["tables"], centroids=d["cents"],
                         label_free=label_free)
        ev.capture(y, x, warmup=1)
        assert ev.graph is not None and not model.training
        seed_g.fill_(KEY)
        got = ev.run(y, x, sens)
        torch.cuda.synchronize()
        assert int(seed_g) == KEY + 3
        assert torch.equal(got.indiv_prob, want.indiv_prob)
        _assert_scores_equal(got.scores, want.scores)
        with pytest.raises(ValueError):
            ms.EvalPass(model, _vae_args(), B_).capture(y, x)
        with pytest.raises(ValueError):
            ms.EvalPass(model, _philox_args(seed_g), B_).capture(y[:5], x[:5])
    finally:
        model.reparam_noise = noise


@pytest.mark.parametrize("N", [300, 5])
def test_torch_cpu_noise_equals_the_compute_loss_loop(split, N):
    """label_free=False with the default noise: the reference's RNG stream and
    the bits of its compute_loss(...)[6], batch by batch."""
    d = split
    model = d["model"].eval()
    y, x = d["y"][:N], d["x"][:N]
    args = _vae_args()
    torch.manual_seed(21)
    torch.cuda.manual_seed(21)
    rows = []
    with torch.no_grad():
        for i in range(N // B_ + 1):
            yb, xb = y[i * B_:min((i + 1) * B_, N)], x[i * B_:min((i + 1) * B_, N)]
            if len(yb):
                rows.append(mpvae.compute_loss(yb, *model(yb, xb), model.r_sqrt_sigma, args)[6])
    state = torch.get_rng_state()
    ev = ms.EvalPass(model, args, B_)
    torch.manual_seed(21)
    torch.cuda.manual_seed(21)
    out = ev.run(y, x)
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(out.indiv_prob, torch.cat(rows))
    assert ev.read(out)["fair_mean_diff"] is None
    _assert_scores_equal(out.scores, mf.split_scores(out.indiv_prob, y))
