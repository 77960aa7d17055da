"""GPU: whole epochs fed on the device -- ``TrainStep.run_epoch`` /
``capture_epoch`` (and FairTrainStep, CalibrationStep with their third input),
``FairTrainStep.validate_epoch`` and ``EvalPass.run_split`` over a
``mpvae_step.DeviceSplit`` -- against the same loops fed by hand, the way the
reference feeds them: ``torch.from_numpy(data[idx]).float().to(device)``."""
import argparse

import numpy as np
import pytest
import torch

import mpvae
import mpvae_fair as mf
import mpvae_step
from fair_step_ref import penalty_ref
from guarded_alloc import same_bits
from oracle import torch_ref
from tolerances import params_track

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F_, L_, Z_, B_, S_ = 12, 6, 4, 8, 10
CENTROIDS = np.array([[0, 0], [0, 1], [1, 0]], np.int64)


def _args(seed=5, **kw):
    a = argparse.Namespace(feature_dim=F_, latent_dim=8, label_dim=L_, z_dim=Z_, keep_prob=0.5,
                           scale_coeff=1.0, residue_sigma="", n_train_sample=S_,
                           n_test_sample=S_, mode="train", nll_coeff=0.5, c_coeff=10.0,
                           mpvae_noise="philox",
                           mpvae_seed=torch.tensor([seed], dtype=torch.int64, device=DEV),
                           fair_coeff=2.0, fairness_loss_norm="l2", learn_logit=True)
    a.__dict__.update(kw)
    return a


def _data(n, seed=0):
    """uint8 labels, fp64 features, int64 sensitive rows (3 patterns), and two
    distance dicts over the labels that occur (T = 2)."""
    rng = np.random.default_rng(seed)
    labels = (rng.random((n, L_)) < 0.4).astype(np.uint8)
    labels[:, 0], labels[:, 1] = 1, 0
    feats = rng.standard_normal((n, F_))
    sens = CENTROIDS[rng.integers(0, 3, n)]
    dists = [{"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1)) for r in labels[i::3]}
             for i in range(2)]
    return dict(labels=labels, feats=feats, sens=sens, dists=dists, n=n)


def _make(kind, d, capturable=True, **argkw):
    """-> (step, the tensors that make up its state)."""
    args = _args(**argkw)
    torch.manual_seed(3)
    np.random.seed(3)
    model = mpvae.VAE(args).to(DEV).train()
    tables = [mf.LabelDistanceTable(t, L_, DEV) for t in d["dists"]]
    if kind == "calib":
        g = torch.Generator().manual_seed(1)
        thr = torch.rand(1, L_, 3, generator=g) * .1 + .45
        x = torch.log(thr / (1 - thr)).to(DEV).requires_grad_(True)
        opt = torch.optim.Adam([x], lr=2e-2, weight_decay=1e-5, fused=True, capturable=capturable)
        sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
        step = mpvae_step.CalibrationStep(model, x, opt, args, tables,
                                          torch.from_numpy(CENTROIDS).to(DEV), scheduler=sched)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5, fused=True,
                               capturable=capturable)
        sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
        if kind == "fair":
            step = mpvae_step.FairTrainStep(model, opt, args, tables, max_groups=3,
                                            scheduler=sched)
        else:
            step = mpvae_step.TrainStep(model, opt, args, scheduler=sched)
    return step


def _state(step):
    """Parameters, Adam state, the update count, the Philox key, the device
    StepLR: everything a step changes."""
    out = [p.detach() for p in step.params] + list(step.model.state_dict().values())
    for p in step.params:
        out += [v for _, v in sorted(step.opt.state[p].items())]
    return out + [step.updates, step.args.mpvae_seed, step.sched.lr, step.sched.last_epoch]


def _hand_batches(d, order, B):
    """The reference's feed (fairsoft_train.py:48-56): per batch, a numpy gather,
    .float() and a host-to-device copy."""
    n = len(order)
    for i in range(n // B + 1):
        idx = order[i * B:min((i + 1) * B, n)]
        if len(idx) == 0:
            continue
        yield (torch.from_numpy(d["labels"][idx]).float().to(DEV),
               torch.from_numpy(d["feats"][idx]).float().to(DEV),
               torch.from_numpy(d["sens"][idx]).to(DEV))


def _hand_epoch(step, kind, d, order, B):
    n = 0
    for y, x, s in _hand_batches(d, order, B):
        step(y, x) if kind == "train" else step(y, x, s)
        n += 1
    return n


def _split(d, sens=True):
    return mpvae_step.DeviceSplit(d["labels"], d["feats"], d["sens"] if sens else None,
                                  device=DEV)


# --------------------------------------------- 1. eager against the hand-fed loop
@pytest.mark.parametrize("n,steps", [(8 * 5 + 3, 6), (8 * 5, 5), (3, 1)])
@pytest.mark.parametrize("kind", ["train", "fair", "calib"])
def test_run_epoch_eager_equals_the_hand_fed_loop(kind, n, steps):
    """Two epochs with different orders.  N = 8*5: the empty last batch is
    skipped (5 steps, not 6); N = 3 < B: one ragged step."""
    d = _data(n, seed=n)
    rng = np.random.default_rng(1)
    orders = [rng.permutation(n), rng.permutation(n)[::-1].copy()]
    fed, hand = _make(kind, d), _make(kind, d)
    split = _split(d, sens=kind != "train")
    torch.cuda.manual_seed(9)
    got = [fed.run_epoch(split, o, B_) for o in orders]
    assert int(split.cursor) == n - n % B_
    torch.cuda.manual_seed(9)
    want = [_hand_epoch(hand, kind, d, o, B_) for o in orders]
    assert got == want == [steps, steps]
    split.check()
    assert int(fed.updates) == 2 * steps
    a, b = _state(fed), _state(hand)
    assert len(a) == len(b) and all(same_bits(u, v) for u, v in zip(a, b))
    if kind == "fair":
        assert fed.read_totals() == hand.read_totals()


# ----------------------------------------------------- 2. the captured epoch
def _graph_pair(d, order0, **argkw):
    """A FairTrainStep with a captured epoch and its eager twin, both one
    step (the capture's warm-up) into order0; no torch RNG in the step, as in
    test_fair_train_step_graph_replays_match_eager."""
    out = []
    for captured in (True, False):
        step = _make("fair", d, keep_prob=0.0, n_train_sample=64, seed=99, **argkw)
        step.model.reparam_noise = torch.zeros_like
        split = _split(d)
        split.set_order(order0)
        if captured:
            step.capture_epoch(split, B_, warmup=1)
            assert int(split.cursor) == 0
        else:
            step.step(*split.gather(order0, 0, B_))
        out.append((step, split))
    return out


def test_capture_epoch_replays_match_the_eager_epochs():
    """The criterion of test_fair_train_step_graph_replays_match_eager: state to
    rtol 1e-6 (atol 1e-9), the counts exact, the sums to 1e-6 of their value."""
    n = 8 * 5 + 3
    d = _data(n, seed=4)
    rng = np.random.default_rng(2)
    order0 = rng.permutation(n)
    (tg, sg), (te, se) = _graph_pair(d, order0)
    for epoch in range(2):
        order = rng.permutation(n)
        assert tg.run_epoch(sg, order, B_) == te.run_epoch(se, order, B_) == 6
        assert int(sg.cursor) == int(se.cursor) == n - n % B_
        assert sg.order.tolist() == list(order)  # uploaded again for this epoch
        tot_g, tot_e = tg.read_totals(), te.read_totals()
        first = 1 if epoch == 0 else 0  # the warm-up step
        assert tot_g["steps"] == tot_e["steps"] == 6 + first
        assert tot_g["updates"] == tot_e["updates"] == 6 * (epoch + 1) + 1
        assert tot_g["contributed"] == tot_e["contributed"] > 0
        for k in mpvae_step.SUM_KEYS:
            assert abs(tot_g[k] - tot_e[k]) <= 1e-6 * abs(tot_e[k]), k
        assert tot_e["fairloss"] > 0
    for (k, a), b in zip(tg.model.state_dict().items(), te.model.state_dict().values()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-9, msg=k)
    assert int(tg.args.mpvae_seed) == int(te.args.mpvae_seed) == 99 + 13
    assert tg.sync_scheduler() == te.sync_scheduler()
    sg.check()
    se.check()
    # a shorter order next: the graph runs its full batches, the rest is -1 and unread
    short = rng.permutation(n)[:19]
    assert tg.run_epoch(sg, short, B_) == te.run_epoch(se, short, B_) == 3
    assert int(sg.cursor) == 16 and sg.order.tolist() == list(short) + [-1] * (n - 19)
    sg.check()
    for (k, a), b in zip(tg.model.state_dict().items(), te.model.state_dict().values()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-9, msg=k)


def test_capture_epoch_conditions():
    d = _data(20)
    split = _split(d)
    with pytest.raises(ValueError, match="capturable"):
        _make("fair", d, capturable=False).capture_epoch(split, B_)
    with pytest.raises(ValueError, match="philox"):
        _make("fair", d, mpvae_seed=3).capture_epoch(split, B_)
    with pytest.raises(ValueError, match="full batch"):
        _make("fair", d).capture_epoch(split, 21)
    cpu = mpvae_step.DeviceSplit(d["labels"], d["feats"], d["sens"])
    with pytest.raises(ValueError, match="GPU"):
        _make("fair", d).capture_epoch(cpu, B_)


def _device_events(fn):
    """{name: count} of the device activities (kernels, copies) of one call."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key: e.count for e in prof.key_averages()
            if (getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0))}


def test_replayed_epoch_step_has_no_batch_copy():
    """One replay of the epoch graph against one hand-fed captured step (three
    ``copy_`` into the static buffers, then the replay of the same body): the
    epoch step is that body plus at most two launches of the gather entry and
    nothing else -- no copy for the batch -- so it has fewer device activities."""
    n = 8 * 5
    d = _data(n, seed=6)
    order = np.random.default_rng(3).permutation(n)
    (tg, sg), _ = _graph_pair(d, order)
    hand = _make("fair", d, keep_prob=0.0, n_train_sample=64, seed=99)
    hand.model.reparam_noise = torch.zeros_like
    batch = next(_hand_batches(d, order, B_))
    hand.capture(*batch, warmup=1)
    sg.set_order(order)
    tg._epoch.graph.replay()
    hand(*batch)
    torch.cuda.synchronize()
    ours = _device_events(tg._epoch.graph.replay)
    theirs = _device_events(lambda: hand(*batch))
    feed = _device_events(lambda: [buf.copy_(x) for buf, x in zip(hand._captured.bufs, batch)])
    gathers = sum(c for k, c in ours.items() if "gather_" in k)
    print("epoch step:", sum(ours.values()), "device activities,", gathers, "of the gather entry;",
          "hand-fed step:", sum(theirs.values()), "; its three copy_:", feed)
    assert sum(feed.values()) == 3
    assert 1 <= gathers <= 2, ours
    assert not any("gather_" in k for k in theirs)
    body = {k: c - feed.get(k, 0) for k, c in theirs.items() if c - feed.get(k, 0)}
    assert {k: c for k, c in ours.items() if "gather_" not in k} == body
    assert sum(ours.values()) < sum(theirs.values())
    sg.check()


# ------------------------------------------ 3. against the reference's loop
def _c1_epoch(kind, norm):
    """One epoch (5 full batches of 24 and a ragged one of 8) over the inputs of
    test_gpu_fair_step.test_fair_train_step_tracks_reference_loop: C1, its
    features, labels, sensitive rows and tables, torch-CPU probit noise, Adam +
    StepLR(2, 0.5).  kind "epoch": FairTrainStep.run_epoch from a DeviceSplit;
    "ref": the reference's loop (fairsoft_train.py:47-162) restated op for op and
    fed the reference's way, ``data[idx]`` on the host."""
    from test_gpu_fair_step import C1, C1_LR, _args as c1_args, _c1_data, _seeded_model
    B = 24
    args = c1_args(mpvae_linear="torch", fairness_loss_norm=norm, **C1)
    model = _seeded_model(args, seed=7).to(DEV).train()
    ours = kind == "epoch"
    opt = torch.optim.Adam(model.parameters(), lr=C1_LR, weight_decay=1e-5, fused=ours)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    X, Y, sens, dists = _c1_data()
    X, Y = X.numpy(), Y.numpy()
    n = X.shape[0]
    order = np.random.default_rng(17).permutation(n)
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    if ours:
        tables = [mf.LabelDistanceTable(t, C1["label_dim"], DEV) for t in dists]
        step = mpvae_step.FairTrainStep(model, opt, args, tables, scheduler=sched)
        split = mpvae_step.DeviceSplit(Y, X, sens, device=DEV)
        steps = step.run_epoch(split, order, B)
        split.check()
        tot = step.read_totals()
        step.sync_scheduler()
        sums = [tot[k] for k in ("total", "nll", "nll_x", "c", "c_x", "kl", "fairloss")]
        contributed = tot["contributed"]
        assert tot["steps"] == tot["updates"] == steps
    else:
        sums, contributed, steps = np.zeros(7), 0, 0
        for i in range(n // B + 1):
            idx = order[i * B:min((i + 1) * B, n)]
            if len(idx) == 0:
                continue
            feat = torch.from_numpy(X[idx]).float().to(DEV)
            label = torch.from_numpy(Y[idx]).float().to(DEV)
            s = torch.from_numpy(sens[idx]).to(DEV)
            opt.zero_grad()
            out = torch_ref.vae_forward_reference_order(model, label, feat)
            noise = torch.normal(0, 1, size=(C1["n_train_sample"], len(idx),
                                             C1["z_dim"])).to(DEV)
            res = torch_ref.elbo_naive(label, *out, model.r_sqrt_sigma, noise, args.nll_coeff,
                                       args.c_coeff)
            total_loss = res[0]
            fairloss, c = penalty_ref(res[7], res[6], Y[idx], s, dists, norm, args.fair_coeff)
            assert not isinstance(fairloss, float)  # the penalty is active in every step
            total_loss += fairloss
            total_loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
            assert all(torch.isfinite(p.grad).all() for p in model.parameters()
                       if p.grad is not None)
            opt.step()
            sched.step()
            sums += np.array([float(total_loss.detach())] + [float(r.detach()) for r in res[1:6]]
                             + [float(fairloss.detach())])
            contributed += c
            steps += 1
        sums = list(sums)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return steps, sums, contributed, state, opt.param_groups[0]["lr"]


@pytest.mark.parametrize("norm", ["l1", "l2"])
def test_fair_run_epoch_tracks_reference_loop(norm):
    """The tolerances of test_fair_train_step_tracks_reference_loop, unwidened:
    rtol 1e-4 on the losses (here on the epoch's sum of each loss, six addends
    of one sign each within that bound), ``contributed`` exact, the learning rate
    equal, and params_track's Adam-flip bounds, which already scale with the
    number of steps (6)."""
    from test_gpu_fair_step import C1_LR
    n1, sums1, c1, p1, lr1 = _c1_epoch("epoch", norm)
    n2, sums2, c2, p2, lr2 = _c1_epoch("ref", norm)
    print("sums ours", sums1, "\nsums ref ", sums2)
    assert n1 == n2 == 6 and c1 == c2 > 0
    assert sums2[6] > 0
    np.testing.assert_allclose(sums1, sums2, rtol=1e-4)
    assert lr1 == lr2 == C1_LR * 0.125
    params_track("fair_epoch_vs_reference_loop_" + norm, p1, p2, C1_LR, n1)


# ------------------------------------------------------------ 4. validation
@pytest.mark.parametrize("n,steps", [(8 * 2 + 3, 3), (8 * 2, 2)])
def test_validate_epoch_equals_validate_over_the_same_batches(n, steps):
    d = _data(n, seed=8)
    order = np.random.default_rng(4).permutation(n)
    fed, hand = _make("fair", d), _make("fair", d)
    split = _split(d)
    torch.cuda.manual_seed(2)
    assert fed.validate_epoch(split, order, B_) == steps
    assert fed.model.training
    torch.cuda.manual_seed(2)
    for batch in _hand_batches(d, order, B_):
        hand.validate(*batch)
    split.check()
    got, want = fed.read_totals(), hand.read_totals()
    assert got == want and got["valid"]["steps"] == steps and got["steps"] == 0
    assert got["valid"]["contributed"] > 0 and int(fed.updates) == 0
    assert all(same_bits(a, b) for a, b in zip(_state(fed)[:-2], _state(hand)[:-2]))
    fed.model.eval()
    fed.validate_epoch(split, order, B_)
    assert not fed.model.training  # eval stays eval


# ------------------------------------------------------------ 5. evaluation
@pytest.mark.parametrize("subset", [True, False])
def test_eval_pass_run_split_equals_run_on_gathered_tensors(subset):
    n = 43
    d = _data(n, seed=12)
    args = _args(mode="test", mpvae_seed=11)
    torch.manual_seed(3)
    model = mpvae.VAE(args).to(DEV)
    tables = [mf.LabelDistanceTable(t, L_, DEV) for t in d["dists"]]
    ev = mpvae_step.EvalPass(model, args, B_, tables=tables,
                             centroids=torch.from_numpy(CENTROIDS).to(DEV))
    order = np.random.default_rng(5).permutation(n)[:29] if subset else None
    idx = order if subset else np.arange(n)
    torch.cuda.manual_seed(7)
    got = ev.run_split(_split(d), order)
    torch.cuda.manual_seed(7)
    want = ev.run(torch.from_numpy(d["labels"][idx]).float().to(DEV),
                  torch.from_numpy(d["feats"][idx]).float().to(DEV),
                  torch.from_numpy(d["sens"][idx]).to(DEV))
    assert same_bits(got.indiv_prob, want.indiv_prob)
    for k in ("miF1", "maF1", "fair_mean_diff", "fair_mean_sq", "fair_terms", "counts", "gid"):
        assert same_bits(getattr(got.scores, k), getattr(want.scores, k)), k
    assert ev.read(got) == ev.read(want)


# --------------------------------------------------- 6. an order out of range
@pytest.mark.parametrize("kind", ["train", "fair"])
def test_out_of_range_device_order_is_gated_and_reported(kind):
    """A device-tensor order is not checked on the host: the bad row is NaN, the
    step's gradients are not finite, the gate skips the update, check() raises."""
    n = 8
    d = _data(n, seed=2)
    step = _make(kind, d)
    split = _split(d, sens=kind != "train")
    good = torch.arange(n, device=DEV)
    assert step.run_epoch(split, good, B_) == 1
    assert int(step.updates) == 1 and float(step.found_inf) == 0.0
    split.check()
    before = [t.clone() for t in _state(step)[:-4]]
    bad = good.clone()
    bad[5] = n
    assert step.run_epoch(split, bad, B_) == 1
    assert float(step.found_inf) == 1.0 and int(step.updates) == 1
    assert any(not bool(torch.isfinite(p.grad).all()) for p in step.params if p.grad is not None)
    assert all(same_bits(a, b) for a, b in zip(before, _state(step)[:-4]))
    with pytest.raises(IndexError, match="out-of-range"):
        split.check()
    split.check()
    with pytest.raises(IndexError, match=r"outside \[0, 8\)"):  # a numpy order: on the host
        step.run_epoch(split, bad.cpu().numpy(), B_)
