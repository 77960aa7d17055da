"""GPU: the fused fairness path (mpv_group_rows, mpv_label_weights_batch,
``fairness_penalty(fused=True)``) against the unfused one, bit for bit, and
``mpvae_step.FairTrainStep`` against the reference loop restated op for op
(oracle/torch_ref, tests/fair_step_ref.penalty_ref), against TrainStep, and
captured in a HIP graph."""
import argparse
import warnings

import numpy as np
import pytest
import torch

import mpvae
import mpvae_fair as mf
import mpvae_hip as H
import mpvae_step
from fair_io import fair_fixtures
from fair_step_ref import penalty_ref
from oracle import fairness as of
from oracle import torch_ref
from tolerances import params_track

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAIR = fair_fixtures()
NP_DTYPES = {"int64": np.int64, "int32": np.int32, "float32": np.float32, "float64": np.float64}


# ------------------------------------------------------------ 1. group_rows
def _group_patterns(B, n, dtype, rng):
    """name -> (B, n) rows of ``dtype``: the edge patterns of the grouping."""
    is_float = np.issubdtype(dtype, np.floating)
    unit = 0.5 if is_float else 1
    same = np.full((B, n), 3 * unit)
    distinct = np.zeros((B, n))
    distinct[:, 0] = (np.arange(B) // 3 - B // 6) * unit if n > 1 else (np.arange(B) - B // 2) * unit
    distinct[:, -1] = distinct[:, -1] if n == 1 else (np.arange(B) % 3) * unit
    last = np.zeros((B, n))
    last[:, -1] = rng.integers(-2, 3, B) * unit
    negative = rng.integers(-3, 3, (B, n)) * unit
    zeros = rng.integers(0, 2, (B, n)).astype(np.float64)
    if is_float:
        zeros[rng.random((B, n)) < 0.5] *= -1.0  # -0.0 beside +0.0 (and -1 beside 1)
    pats = dict(same=same, distinct=distinct, last_column=last, negative=negative,
                signed_zero=zeros)
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in pats.items()}


@pytest.mark.parametrize("dtype", list(NP_DTYPES))
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 1025])
def test_group_rows_equals_sensitive_groups(B, n, dtype):
    rng = np.random.default_rng(1000 * B + 10 * n + len(dtype))
    for name, rows in _group_patterns(B, n, NP_DTYPES[dtype], rng).items():
        uniq, inv = torch.unique(torch.from_numpy(rows), dim=0, return_inverse=True)
        k = uniq.shape[0]
        if name == "distinct":
            assert k == B
        if name == "signed_zero" and rows.dtype.kind == "f" and B > 1:
            assert np.signbit(rows[rows == 0]).any() and not np.signbit(rows[rows == 0]).all()
        x = torch.from_numpy(rows).to(DEV)
        for mg in (k, k - 1, None):
            if mg == 0:
                continue
            got, ref = mf.group_rows(x, mg), mf.sensitive_groups(x, mg)
            what = (name, mg)
            assert got[3] == ref[3], what
            for a, b, field in zip(got[:3], ref[:3], ("gid", "order", "goff")):
                assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b), what + (field,)
            assert got[4].dtype == torch.bool and torch.equal(got[4], ref[4]), what
            assert bool(got[4]) == (mg is not None and mg < k), what
            if not bool(got[4]):
                assert torch.equal(got[0].cpu().long(), inv.reshape(B)), what


def test_group_rows_casts_other_dtypes_and_falls_back_out_of_range():
    rng = np.random.default_rng(4)
    rows = rng.integers(0, 2, (40, 3))
    ref = mf.sensitive_groups(torch.from_numpy(rows).to(DEV), 8)
    for dt in (torch.bool, torch.uint8, torch.int16, torch.float16, torch.bfloat16):
        got = mf.group_rows(torch.from_numpy(rows).to(DEV).to(dt), 8)
        assert all(torch.equal(a, b) for a, b in zip(got[:3] + got[4:], ref[:3] + ref[4:])), dt
    # an (8, 3, 2) batch is grouped by its flattened rows
    x3 = torch.from_numpy(rng.integers(0, 2, (8, 3, 2))).to(DEV)
    got, ref3 = mf.group_rows(x3), mf.sensitive_groups(x3)
    assert all(torch.equal(a, b) for a, b in zip(got[:3] + got[4:], ref3[:3] + ref3[4:]))
    # past the documented range (n > 64 columns): the library launches nothing
    # and says so; the wrapper answers through sensitive_groups
    wide = torch.from_numpy(rng.integers(0, 2, (8, H.GROUP_MAX_N + 1))).to(DEV)
    out = torch.empty(8, dtype=torch.int32, device=DEV)
    flag = torch.empty((), dtype=torch.bool, device=DEV)
    rc = H.load_library().mpv_group_rows(H.ptr(wide), H.EL_I64, 8, H.GROUP_MAX_N + 1, 8, H.ptr(out),
                                         H.ptr(out), H.ptr(out), H.ptr(flag), H.stream_of(DEV))
    assert rc == H.EINVAL
    got, refw = mf.group_rows(wide), mf.sensitive_groups(wide)
    assert all(torch.equal(a, b) for a, b in zip(got[:3] + got[4:], refw[:3] + refw[4:]))
    # an empty batch launches nothing
    e = mf.group_rows(torch.zeros((0, 2), dtype=torch.int64, device=DEV))
    r = mf.sensitive_groups(torch.zeros((0, 2), dtype=torch.int64, device=DEV))
    assert e[3] == r[3] and all(torch.equal(a, b) for a, b in zip(e[:3] + e[4:], r[:3] + r[4:]))


# ---------------------------------------------------- 2. label_weights_batch
def _tables_for(labels, T, rng, L):
    """T dicts over the batch's own rows: table t holds rows t, t + T + 1, ...
    (so rows T, 2T + 1, ... are in no table); with T >= 3 table 1 is empty."""
    dists = []
    for t in range(T):
        rows = labels[t::T + 1]
        dists.append({} if (T >= 3 and t == 1) else
                     {"".join(r.astype(int).astype(str)): np.float64(rng.uniform(0.1, 1))
                      for r in rows})
    return dists, [mf.LabelDistanceTable(d, L, DEV) for d in dists]


@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("T", [1, 3, H.LABEL_TABLES_PER_LAUNCH + 1])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 200, 1030])
def test_label_weights_batch_equals_label_weights(L, T, B):
    rng = np.random.default_rng(100 * L + 10 * T + B)
    labels = (rng.random((B, L)) < 0.3).astype(np.float32)
    dists, tables = _tables_for(labels, T, rng, L)
    if B > 1:
        labels[1, L // 2] = 2.0  # int() neither 0 nor 1: a miss in every table
    y = torch.from_numpy(labels).to(DEV)
    w, count = mf.label_weights_batch(y, tables)
    w_ref, count_ref = mf.label_weights(y, tables)
    assert w.shape == (T, B) and w.dtype == torch.float64 and count.dtype == torch.int32
    assert np.array_equal(w.cpu().numpy(), w_ref.cpu().numpy())
    assert int(count) == int(count_ref)
    # and both are what the reference's dict lookup gives
    for t, d in enumerate(dists):
        assert np.array_equal(w[t].cpu().numpy(), of.row_weights(labels, d))
    if B > 1:
        assert float(w[:, 1].abs().max()) == 0.0 and float(w[0, 0]) > 0.0
        if L > 1:  # L = 1 has two patterns only: no row is absent from every table
            assert float(w[:, T].abs().max()) == 0.0
    # the single row poisoned, and an empty table alone
    bad = y.clone()
    bad[0, 0] = 2.0
    for yy, tt in ((bad, tables), (y, [mf.LabelDistanceTable({}, L, DEV)])):
        a, b = mf.label_weights_batch(yy, tt), mf.label_weights(yy, tt)
        assert torch.equal(a[0], b[0]) and int(a[1]) == int(b[1])


@pytest.mark.parametrize("T", [1, H.LABEL_TABLES_PER_LAUNCH, H.LABEL_TABLES_PER_LAUNCH + 1])
def test_fused_groups_and_weights_take_one_plus_ceil_t_over_k_launches(T):
    rng = np.random.default_rng(T)
    B, L = 40, 70
    labels = (rng.random((B, L)) < 0.3).astype(np.float32)
    _, tables = _tables_for(labels, T, rng, L)
    y = torch.from_numpy(labels).to(DEV)
    sens = torch.from_numpy(rng.integers(0, 2, (B, 2))).to(DEV)
    lib = H.load_library()
    lib.mpv_timing_reset()
    lib.mpv_timing_enable(1)
    try:
        mf.label_weights_batch(y, tables)
        mf.group_rows(sens, 4)
        torch.cuda.synchronize()
        launched = H.kernel_times()
    finally:
        lib.mpv_timing_enable(0)
    chunks = -(-T // H.LABEL_TABLES_PER_LAUNCH)
    assert {k: v[0] for k, v in launched.items()} == {"label_weights": chunks, "group_rows": 1}


# --------------------------------------------------------- 3. fused penalty
def _penalty(f, fused, max_groups=None):
    L = f["labels"].shape[1]
    tables = [mf.LabelDistanceTable(d, L, DEV) for d in f["dists"]]
    lz = torch.from_numpy(f["label_z"]).to(DEV).requires_grad_(True)
    fz = torch.from_numpy(f["feat_z"]).to(DEV).requires_grad_(True)
    loss, count = mf.fairness_penalty(lz, fz, torch.from_numpy(f["labels"]).to(DEV),
                                      torch.from_numpy(f["sensitive"]).to(DEV), tables, f["norm"],
                                      f["coeff"], max_groups=max_groups, fused=fused)
    loss.backward()
    return loss.detach(), count, lz.grad, fz.grad


def _assert_same_penalty(a, b):
    assert a[0].dtype == b[0].dtype
    assert torch.equal(a[0], b[0]) or (torch.isnan(a[0]) and torch.isnan(b[0]))
    assert int(a[1]) == int(b[1])
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


@pytest.mark.parametrize("f", FAIR, ids=[f["name"] for f in FAIR])
def test_fused_penalty_equals_unfused_on_fixtures(f):
    _assert_same_penalty(_penalty(f, True), _penalty(f, False))
    for mg in (1, 64):  # an overflowing bound and a roomy one
        _assert_same_penalty(_penalty(f, True, mg), _penalty(f, False, mg))


@pytest.mark.parametrize("norm", ["l1", "l2"])
def test_fused_penalty_equals_unfused_at_training_size(norm):
    """The inputs of test_gpu_fair.test_fair_penalty_training_size_against_oracle."""
    rng = np.random.default_rng(7)
    B, L = 512, 1024
    labels = (rng.random((B, L)) < 0.02).astype(np.int64)
    labels[256:] = labels[:256]
    sens = rng.integers(0, 3, (B, 2)).astype(np.int64)
    dists = [{"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1)) for r in labels[i::7]}
             for i in range(3)]
    f = dict(labels=labels, sensitive=sens, dists=dists, norm=norm, coeff=0.5,
             label_z=rng.uniform(0.01, 0.99, (B, L)).astype(np.float32),
             feat_z=rng.uniform(0.01, 0.99, (B, L)).astype(np.float32))
    fused, unfused = _penalty(f, True), _penalty(f, False)
    _assert_same_penalty(fused, unfused)
    assert float(fused[0]) > 0 and int(fused[1]) > 0


def test_fused_penalty_is_graph_capturable():
    """test_gpu_fair.test_fair_penalty_is_graph_capturable with ``fused=True``:
    replays on new batch contents equal eager calls, and the capture raises no
    stream-mismatch warning."""
    rng = np.random.default_rng(5)
    B, L = 256, 300
    lab = torch.from_numpy((rng.random((B, L)) < 0.05).astype(np.float32)).to(DEV)
    dists = [{"".join(r.astype(int).astype(str)): float(rng.uniform(0.1, 1))
              for r in lab.cpu().numpy()[i::3]} for i in range(2)]
    tables = [mf.LabelDistanceTable(d, L, DEV) for d in dists]
    sens = torch.from_numpy(rng.integers(0, 3, (B, 2))).to(DEV)
    lz = torch.from_numpy(rng.uniform(0.01, 0.99, (B, L)).astype(np.float32)).to(DEV)
    fz = torch.from_numpy(rng.uniform(0.01, 0.99, (B, L)).astype(np.float32)).to(DEV)

    def eager(lz_v, fz_v, sens_v, fused):
        a, b = lz_v.clone().requires_grad_(True), fz_v.clone().requires_grad_(True)
        loss, cnt = mf.fairness_penalty(a, b, lab, sens_v, tables, "l2", 0.7, max_groups=16,
                                        fused=fused)
        loss.backward()
        return loss.detach(), cnt, a.grad, b.grad

    a = lz.clone().requires_grad_(True)
    b = fz.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            a.grad = b.grad = None
            loss, cnt = mf.fairness_penalty(a, b, lab, sens, tables, "l2", 0.7, max_groups=16,
                                            fused=True)
            loss.backward()
    torch.cuda.current_stream().wait_stream(side)
    a.grad = b.grad = None
    del loss, cnt  # the warm-up's graph holds AccumulateGrad nodes made on `side`
    graph = torch.cuda.CUDAGraph()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.cuda.graph(graph):
            loss, cnt = mf.fairness_penalty(a, b, lab, sens, tables, "l2", 0.7, max_groups=16,
                                            fused=True)
            loss.backward()
    bad = [str(w.message)[:80] for w in caught if "AccumulateGrad" in str(w.message)]
    assert not bad, bad
    for it in range(3):
        new_l = torch.from_numpy(rng.uniform(0.01, 0.99, (B, L)).astype(np.float32)).to(DEV)
        new_s = torch.from_numpy(rng.integers(0, 2 + it, (B, 2))).to(DEV)
        with torch.no_grad():
            a.copy_(new_l)
            sens.copy_(new_s)
        graph.replay()
        torch.cuda.synchronize()
        for fused in (True, False):
            ref = eager(new_l, fz, new_s, fused)
            assert torch.equal(loss, ref[0]) and int(cnt) == int(ref[1])
            assert torch.equal(a.grad, ref[2]) and torch.equal(b.grad, ref[3])


# ---------------------------------------------------------- FairTrainStep
def _args(**kw):
    a = argparse.Namespace(feature_dim=20, latent_dim=8, label_dim=6, z_dim=4, keep_prob=0.5,
                           scale_coeff=1.0, residue_sigma="", n_train_sample=16,
                           n_test_sample=16, mode="train", nll_coeff=0.5, c_coeff=10.0,
                           fair_coeff=2.0, fairness_loss_norm="l2")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _seeded_model(args, seed=0):
    torch.manual_seed(seed)
    np.random.seed(seed)
    return mpvae.VAE(args)


C1 = dict(feature_dim=1000, label_dim=38, z_dim=38, latent_dim=50, n_train_sample=10)
C1_B, C1_LR, C1_STEPS = 32, 7.5e-4, 4
CENTROIDS = np.array([[0, 0], [0, 1], [1, 0]], np.int64)


def _c1_data(steps=C1_STEPS, batch=C1_B):
    """Features, labels, sensitive rows (3 groups) of every step, and 2 target
    tables with numpy-float64 distances over the labels that occur."""
    g = torch.Generator().manual_seed(11)
    X = torch.randn(steps * batch, C1["feature_dim"], generator=g)
    Y = (torch.rand(steps * batch, C1["label_dim"], generator=g) < 0.3).float()
    Y[:, 0], Y[:, 1] = 1, 0
    rng = np.random.default_rng(13)
    sens = CENTROIDS[rng.integers(0, 3, steps * batch)]
    ynp = Y.numpy()
    dists = [{"".join(r.astype(int).astype(str)): np.float64(rng.uniform(0.1, 1))
              for r in ynp[i::3]} for i in range(2)]
    return X, Y, sens, dists


def _fair_loop(kind, norm, dists_on=True):
    """C1, 4 steps, torch-CPU probit noise, Adam + StepLR(2, 0.5).
    kind "fair": FairTrainStep; "plain": TrainStep (no penalty); "ref": the
    reference loop (fairsoft_train.py:47-162) restated op for op.
    -> per-step records and the final state_dict."""
    args = _args(mpvae_linear="torch", fairness_loss_norm=norm, **C1)
    model = _seeded_model(args, seed=7).to(DEV).train()
    ours = kind != "ref"
    opt = torch.optim.Adam(model.parameters(), lr=C1_LR, weight_decay=1e-5, fused=ours)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    X, Y, sens, dists = _c1_data()
    if not dists_on:
        dists = []
    if kind == "fair":
        tables = [mf.LabelDistanceTable(d, C1["label_dim"], DEV) for d in dists]
        step = mpvae_step.FairTrainStep(model, opt, args, tables, scheduler=sched)
    elif kind == "plain":
        step = mpvae_step.TrainStep(model, opt, args, scheduler=sched)
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    recs = []
    for i in range(C1_STEPS):
        sl = slice(C1_B * i, C1_B * (i + 1))
        feat, label, s = X[sl].to(DEV), Y[sl].to(DEV), torch.from_numpy(sens[sl]).to(DEV)
        if kind == "fair":
            out = step(label, feat, s)
            recs.append(dict(out=out, label=Y[sl].numpy(),
                             losses=[float(t.detach()) for t in out[:6]] + [float(out.fairloss)]))
            continue
        if kind == "plain":
            res = step(label, feat)
            recs.append(dict(losses=[float(r.detach()) for r in res[:6]] + [0.0]))
            continue
        opt.zero_grad()
        out = torch_ref.vae_forward_reference_order(model, label, feat)
        noise = torch.normal(0, 1, size=(C1["n_train_sample"], C1_B, C1["z_dim"])).to(DEV)
        res = torch_ref.elbo_naive(label, *out, model.r_sqrt_sigma, noise, args.nll_coeff,
                                   args.c_coeff)
        total_loss = res[0]
        fairloss, contributed = penalty_ref(res[7], res[6], Y[sl].numpy(), s, dists, norm,
                                            args.fair_coeff)
        if not isinstance(fairloss, float):
            total_loss += fairloss                                       # :137, in place, fp32
        total_loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
        if all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None):
            opt.step()
            sched.step()
        recs.append(dict(contributed=contributed,
                         losses=[float(total_loss.detach())] + [float(r.detach()) for r in res[1:6]]
                         + [float(fairloss.detach())]))
    if ours:
        step.sync_scheduler()
    lr = opt.param_groups[0]["lr"]
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return recs, state, lr, (step if ours else None)


@pytest.mark.parametrize("norm", ["l1", "l2"])
def test_fair_train_step_tracks_reference_loop(norm):
    """The tolerances of test_gpu_vae.test_train_step_device_gate_tracks_reference_loop
    for the losses (the penalty among them) and the parameters; ``contributed``
    exact and the metrics as test_gpu_fair's (rtol 1e-6, atol 1e-7) against
    oracle.fairness on the step's own indiv_prob; read_totals against the sums
    of the per-step values (fp64 sums of 4 terms in another order: 1e-12)."""
    ours, p1, lr1, step = _fair_loop("fair", norm)
    ref, p2, lr2, _ = _fair_loop("ref", norm)
    l1, l2 = [r["losses"] for r in ours], [r["losses"] for r in ref]
    print("losses ours", l1, "\nlosses ref ", l2)
    assert all(r["losses"][6] > 0 for r in ref)  # the penalty is active in every step
    np.testing.assert_allclose(l1, l2, rtol=1e-4)
    assert lr1 == lr2 == C1_LR * 0.25
    params_track("fair_step_vs_reference_loop_" + norm, p1, p2, C1_LR, C1_STEPS)
    sums = np.zeros(len(mpvae_step.SUM_KEYS))
    n_contrib = 0
    for o, r in zip(ours, ref):
        out = o["out"]
        assert out.total.dtype == torch.float32 and out.contributed.dtype == torch.int32
        assert out.metrics.dtype == torch.float64 and out.metrics.shape == (8,)
        assert int(out.contributed) == r["contributed"]
        want = of.train_metrics(out.indiv_prob.detach().cpu().numpy(), o["label"], 0.5)
        got = out.metrics.cpu().numpy()
        assert np.allclose(got, want, rtol=1e-6, atol=1e-7), (got, want)
        sums += np.array(o["losses"] + [got[mf.METRIC_KEYS.index("maF1")],
                                        got[mf.METRIC_KEYS.index("miF1")]])
        n_contrib += r["contributed"]
    tot = step.read_totals()
    assert tot["steps"] == C1_STEPS and tot["updates"] == C1_STEPS
    assert tot["contributed"] == n_contrib and tot["valid"]["steps"] == 0
    np.testing.assert_allclose([tot[k] for k in mpvae_step.SUM_KEYS], sums, rtol=1e-12)
    again = step.read_totals()  # reset
    assert again["steps"] == 0 and again["total"] == 0.0 and again["updates"] == C1_STEPS


def test_fair_train_step_returns_the_rounded_sum():
    """total = float32(float64(compute_loss's total) + fairloss) (:137): the
    first step of a FairTrainStep and of a TrainStep on the same model, the
    same Philox key and the same dropout / reparameterisation draws."""
    args = _args(n_train_sample=8, mpvae_noise="philox", mpvae_seed=3)
    label, feat, sens, tables = _small_batch()

    def first_step(fair):
        model = _seeded_model(args).to(DEV).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
        torch.cuda.manual_seed(1)
        if fair:
            return mpvae_step.FairTrainStep(model, opt, args, tables)(label, feat, sens)
        return mpvae_step.TrainStep(model, opt, args)(label, feat)

    out, res = first_step(True), first_step(False)
    assert torch.equal(out.nll, res[1]) and torch.equal(out.indiv_prob, res[6])
    assert float(out.fairloss) > 0 and out.fairloss.dtype == torch.float64
    want = (res[0].detach().double() + out.fairloss).float()
    assert out.total.dtype == torch.float32 and torch.equal(out.total, want)


def test_fair_train_step_without_tables_tracks_train_step():
    fair, p1, lr1, step = _fair_loop("fair", "l2", dists_on=False)
    plain, p2, lr2, _ = _fair_loop("plain", "l2")
    np.testing.assert_allclose([r["losses"] for r in fair], [r["losses"] for r in plain],
                               rtol=1e-4)
    assert lr1 == lr2
    params_track("fair_step_no_tables_vs_train_step", p1, p2, C1_LR, C1_STEPS)
    for r in fair:
        assert float(r["out"].fairloss) == 0.0 and int(r["out"].contributed) == 0
    tot = step.read_totals()
    assert tot["fairloss"] == 0.0 and tot["contributed"] == 0 and tot["steps"] == C1_STEPS


def _small_batch(B=12, seed=0):
    """A batch at _args()'s shapes with 3 sensitive patterns and one table over
    half of its label rows."""
    g = torch.Generator().manual_seed(seed)
    label = (torch.rand(B, 6, generator=g) < 0.5).float()
    label[:, 0], label[:, 1] = 1, 0
    feat = torch.randn(B, 20, generator=g)
    sens = torch.from_numpy(CENTROIDS[np.arange(B) % 3])
    rng = np.random.default_rng(seed)
    dist = {"".join(r.astype(int).astype(str)): np.float64(rng.uniform(0.1, 1))
            for r in label.numpy()[::2]}
    return label.to(DEV), feat.to(DEV), sens.to(DEV), [mf.LabelDistanceTable(dist, 6, DEV)]


@pytest.mark.parametrize("case", ["degenerate_label_row", "more_patterns_than_max_groups"])
def test_fair_train_step_gate_skips_the_update(case):
    """A NaN ranking gradient (a label row with no positive label), or a batch
    with more sensitive patterns than ``max_groups`` (the penalty is NaN), must
    leave every parameter and the Adam step count untouched and set found_inf;
    the running sums still advance."""
    args = _args(n_train_sample=8)
    model = _seeded_model(args).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    label, feat, sens, tables = _small_batch()
    ts = mpvae_step.FairTrainStep(model, opt, args, tables, max_groups=3)
    out = ts(label, feat, sens)
    assert int(ts.updates) == 1 and float(ts.found_inf) == 0.0 and float(out.fairloss) > 0
    contributed = int(out.contributed)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    if case == "degenerate_label_row":
        label = label.clone()
        label[2] = 0.0
    else:
        sens = sens.clone()
        sens[5] = 7  # a fourth pattern
    out = ts(label, feat, sens)
    assert int(ts.updates) == 1 and float(ts.found_inf) == 1.0
    if case == "more_patterns_than_max_groups":
        assert torch.isnan(out.fairloss) and torch.isnan(out.total)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(int(s["step"]) == 1 for s in opt.state.values())
    tot = ts.read_totals()
    assert tot["steps"] == 2 and tot["updates"] == 1
    assert tot["contributed"] == contributed + int(out.contributed)


def test_fair_train_step_graph_replays_match_eager():
    """The pattern and the numbers of test_gpu_vae.test_train_step_graph_replays_match_eager."""
    B, F_, L = 24, 40, 10
    g = torch.Generator().manual_seed(2)
    rng = np.random.default_rng(2)
    batches = []
    for _ in range(4):
        y = (torch.rand(B, L, generator=g) < 0.3).float()
        y[:, 0], y[:, 1] = 1, 0
        batches.append((y.to(DEV), torch.randn(B, F_, generator=g).to(DEV),
                        torch.from_numpy(CENTROIDS[rng.integers(0, 3, B)]).to(DEV)))
    rows = torch.cat([b[0] for b in batches]).cpu().numpy()
    dists = [{"".join(r.astype(int).astype(str)): np.float64(rng.uniform(0.1, 1))
              for r in rows[i::3]} for i in range(2)]

    def make():
        a = _args(feature_dim=F_, label_dim=L, z_dim=L, latent_dim=8, keep_prob=0.0,
                  n_train_sample=64, mpvae_noise="philox",
                  mpvae_seed=torch.tensor([99], dtype=torch.int64, device=DEV))
        m = _seeded_model(a, seed=3).to(DEV).train()
        m.reparam_noise = torch.zeros_like
        o = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5, fused=True,
                             capturable=True)
        sch = torch.optim.lr_scheduler.StepLR(o, 2, 0.5)
        tables = [mf.LabelDistanceTable(d, L, DEV) for d in dists]
        return m, mpvae_step.FairTrainStep(m, o, a, tables, max_groups=4, scheduler=sch)

    mg, tg = make()
    me, te = make()
    tg.capture(*batches[0], warmup=1)
    te(*batches[0])
    for batch in batches[1:]:
        og = [o.clone() for o in tg(*batch)]
        oe = te(*batch)
        torch.cuda.synchronize()
        assert float(oe.fairloss) > 0
        for name, a, b in zip(oe._fields, og, oe):
            if name == "contributed":
                assert torch.equal(a, b) and int(a) > 0
            else:
                torch.testing.assert_close(a, b.detach(), rtol=1e-6, atol=0, msg=name)
    for (k, a), b in zip(mg.state_dict().items(), me.state_dict().values()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-9, msg=k)
    assert int(tg.updates) == int(te.updates) == 4
    assert tg.sync_scheduler() == te.sync_scheduler() == [1e-3 * 0.5 * 0.5]
    tot_g, tot_e = tg.read_totals(), te.read_totals()
    assert tot_g["steps"] == tot_e["steps"] == 4
    assert tot_g["contributed"] == tot_e["contributed"] > 0
    # the addends of one key agree to rtol 1e-6 (above) and share a sign
    for k in mpvae_step.SUM_KEYS:
        assert abs(tot_g[k] - tot_e[k]) <= 1e-6 * abs(tot_e[k]), k


def test_fair_train_step_validate():
    """validate() equals the eager composition under no_grad (model.eval(),
    compute_loss, fairness_penalty with "l2" whatever args say, compute_metrics)
    bit for bit on the same Philox seed, changes no parameter and no optimizer
    state, and restores the model's mode."""
    args = _args(n_train_sample=8, mpvae_noise="philox", mpvae_seed=17, fairness_loss_norm="l1",
                 fair_coeff=2.5)
    model = _seeded_model(args).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    label, feat, sens, tables = _small_batch()
    ts = mpvae_step.FairTrainStep(model, opt, args, tables, max_groups=3)
    ts(label, feat, sens)  # one update, so that the optimizer has state
    ts.read_totals()
    params = {k: v.clone() for k, v in model.state_dict().items()}
    state = [{k: v.clone() for k, v in s.items()} for s in opt.state.values()]
    torch.cuda.manual_seed(21)
    out = ts.validate(label, feat, sens)
    assert model.training
    torch.cuda.manual_seed(21)
    model.eval()
    with torch.no_grad():
        res = mpvae.compute_loss(label, *model(label, feat), model.r_sqrt_sigma, args)
        fair, count = mf.fairness_penalty(res[7], res[6], label, sens, tables, "l2",
                                          args.fair_coeff, max_groups=3)
        metrics = mf.compute_metrics(res[6], label, 0.5)
    for a, b in zip(out[1:8], res[1:]):
        assert torch.equal(a, b)
    assert float(fair) > 0 and torch.equal(out.fairloss, fair) and int(out.contributed) == int(count)
    assert torch.equal(out.total, (res[0].double() + fair.double()).float())
    assert torch.equal(out.metrics, torch.stack([metrics[k] for k in mf.METRIC_KEYS]))
    torch.cuda.manual_seed(21)
    ts.validate(label, feat, sens)
    assert not model.training  # eval stays eval
    model.train()
    for k, v in model.state_dict().items():
        assert torch.equal(v, params[k]), k
    for s, old in zip(opt.state.values(), state):
        assert all(torch.equal(s[k], old[k]) for k in old)
    tot = ts.read_totals()
    assert tot["steps"] == 0 and tot["valid"]["steps"] == 2 and int(ts.updates) == 1
    assert tot["valid"]["contributed"] == 2 * int(count)
    assert abs(tot["valid"]["fairloss"] - 2 * float(fair)) <= 1e-12 * float(fair)
