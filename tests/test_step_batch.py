"""The batch is a step's argument list (``TrainStep.inputs``), and a captured
graph is one record per capture: a captured ``step``, a captured epoch and
eager calls interleaved keep to their own buffers; ``release_scheduler`` drops
every record; the wrong number of tensors is a ``TypeError`` before anything
runs; a ``validate`` that raises leaves nothing behind.

Shapes: N = 20 rows, B = 8 (two full batches and a ragged tail of 4), L = 5,
6 features, 2 sensitive columns with 3 patterns, 4 noise draws, z = 3; Philox
noise keyed by a device seed.  Dropout and the reparameterisation noise are
off, so that a step draws nothing from torch's generator (a capture would draw
it at another offset) and a replay computes what the eager step computes."""
import argparse

import numpy as np
import pytest
import torch

import mpvae
import mpvae_step
from guarded_alloc import same_bits

DEV = "cuda:0"
N_, B_, L_, F_, S_, Z_ = 20, 8, 5, 6, 4, 3
CENTROIDS = np.array([[0, 0], [0, 1], [1, 0]], np.int64)


def _args(dev, **kw):
    a = argparse.Namespace(feature_dim=F_, latent_dim=8, label_dim=L_, z_dim=Z_, keep_prob=0.0,
                           scale_coeff=1.0, residue_sigma="", n_train_sample=S_,
                           n_test_sample=S_, mode="train", nll_coeff=0.5, c_coeff=10.0,
                           mpvae_noise="philox",
                           mpvae_seed=torch.tensor([41], dtype=torch.int64, device=dev),
                           fair_coeff=2.0, fairness_loss_norm="l2", learn_logit=True)
    a.__dict__.update(kw)
    return a


def _data(seed=0):
    rng = np.random.default_rng(seed)
    labels = (rng.random((N_, L_)) < 0.4).astype(np.uint8)
    labels[:, 0], labels[:, 1] = 1, 0
    dists = [{"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1)) for r in labels[i::3]}
             for i in range(2)]
    return dict(labels=labels, feats=rng.standard_normal((N_, F_)),
                sens=CENTROIDS[np.arange(N_) % 3], dists=dists)


def _batch(d, rows, dev=DEV):
    return (torch.from_numpy(d["labels"][rows]).float().to(dev),
            torch.from_numpy(d["feats"][rows]).float().to(dev),
            torch.from_numpy(d["sens"][rows]).to(dev))


def _make(kind, d, dev=DEV):
    import mpvae_fair as mf
    args = _args(dev)
    torch.manual_seed(3)
    np.random.seed(3)
    model = mpvae.VAE(args).to(dev).train()
    model.reparam_noise = torch.zeros_like
    tables = [mf.LabelDistanceTable(t, L_, dev) for t in d["dists"]] if dev == DEV else []
    if kind == "calib":
        thr = torch.rand(1, L_, 3, generator=torch.Generator().manual_seed(1)) * .1 + .45
        x = torch.log(thr / (1 - thr)).to(dev).requires_grad_(True)
        opt = torch.optim.Adam([x], lr=2e-2, weight_decay=1e-5, fused=True, capturable=True)
        sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
        return mpvae_step.CalibrationStep(model, x, opt, args, tables,
                                          torch.from_numpy(CENTROIDS).to(dev), scheduler=sched)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5, fused=True,
                           capturable=dev == DEV)
    if kind == "train":
        return mpvae_step.TrainStep(model, opt, args)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5) if dev == DEV else None
    return mpvae_step.FairTrainStep(model, opt, args, tables, max_groups=3, scheduler=sched)


def _state(step):
    """Everything a step changes: parameters and buffers, the Adam state, the
    update count, the Philox key and, while the step owns it, the device StepLR."""
    out = [p.detach() for p in step.params] + list(step.model.state_dict().values())
    for p in step.params:
        out += [v for _, v in sorted(step.opt.state[p].items())]
    sched = [] if step.sched is None else [step.sched.lr, step.sched.last_epoch]
    return out + [step.updates, step.args.mpvae_seed] + sched


def _same(got, want):
    """Equal returns: step counts, or tuples of tensors bit for bit."""
    if isinstance(want, int):
        return got == want
    return len(got) == len(want) and all(same_bits(a, b) for a, b in zip(got, want))


def _assert_twins(g, a, got, want, what):
    torch.cuda.synchronize()
    assert _same(got, want), what
    sg, sa = _state(g), _state(a)
    assert len(sg) == len(sa)
    assert all(same_bits(u, v) for u, v in zip(sg, sa)), what
    if isinstance(g, mpvae_step.FairTrainStep):
        tg, ta = g.read_totals(), a.read_totals()
        assert tg == ta and tg["steps"] + tg["valid"]["steps"] > 0, what


def _captured_and_eager(kind, d, order0):
    """``g`` with a captured step (on batch0) and a captured epoch, and ``a``,
    which takes the two warm-up steps of the captures eagerly."""
    g, a = _make(kind, d), _make(kind, d)
    splits = [mpvae_step.DeviceSplit(d["labels"], d["feats"], d["sens"], device=DEV)
              for _ in range(2)]
    for s in splits:
        s.set_order(order0)
    batch0 = _batch(d, np.arange(B_))
    g.capture(*batch0, warmup=1)
    got = g.capture_epoch(splits[0], B_, warmup=1)
    assert g.graph is not None and got is g._epoch.graph and got is not g.graph
    a.step(*batch0)
    a.step(*_batch(d, order0[:B_]))
    _assert_twins(g, a, 0, 0, "after the captures")
    return g, a, splits


# ------------------------------------------------------------ 1. interleaving
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fair", "calib"])
def test_captured_step_captured_epoch_and_eager_calls_interleave(kind):
    """A captured step's static sensitive-feature buffer, the epoch graph's
    buffers and the tensors of eager calls (the ragged tail, validate) are
    separate: after every call of step / run_epoch / validate / step /
    run_epoch the captured object equals its eager twin bit for bit in what
    the call returned, the state, and (FairTrainStep) read_totals()."""
    d = _data()
    rng = np.random.default_rng(1)
    orders = [rng.permutation(N_) for _ in range(3)]
    g, a, (sg, sa) = _captured_and_eager(kind, d, orders[0])
    # other rows, so other sensitive patterns, than the capture's batch0
    b0, b1, b2 = (_batch(d, rows) for rows in (orders[0][:B_], orders[1][4:4 + B_],
                                               orders[2][2:2 + B_]))
    calls = [("step b0", lambda s, sp: s.step(*b0)),
             ("epoch 1", lambda s, sp: s.run_epoch(sp, orders[1], B_)),
             ("validate", lambda s, sp: s.validate(*b1)),
             ("step b2", lambda s, sp: s.step(*b2)),
             ("epoch 2", lambda s, sp: s.run_epoch(sp, orders[2], B_))]
    for what, call in calls:
        if what == "validate" and kind == "calib":
            continue
        got, want = call(g, sg), call(a, sa)
        if what.startswith("epoch"):
            assert got == 3 and int(sg.cursor) == int(sa.cursor) == 16
        _assert_twins(g, a, got, want, what)
    sg.check()
    sa.check()
    assert int(g.updates) == 2 + 2 + 2 * 3


# ----------------------------------------------------- 2. release_scheduler
@pytest.mark.gpu
def test_release_scheduler_drops_both_records():
    """After capture() and capture_epoch(): no graph is left, and run_epoch runs
    eagerly on the host's learning rate -- at lr 0 it moves no parameter, which
    a replay on the device lr would -- bit for bit as an eager twin's."""
    d = _data()
    rng = np.random.default_rng(2)
    order0, order = rng.permutation(N_), rng.permutation(N_)
    g, a, (sg, sa) = _captured_and_eager("fair", d, order0)
    assert g.release_scheduler() == a.release_scheduler() == [1e-3 * 0.5]
    assert g.graph is None and g.out is None and g._epoch is None and g.sched is None
    for step in (g, a):
        step.opt.param_groups[0]["lr"] = 0.0
    before = [p.detach().clone() for p in g.params]
    got, want = g.run_epoch(sg, order, B_), a.run_epoch(sa, order, B_)
    assert got == 3
    _assert_twins(g, a, got, want, "eager epoch after release")
    assert all(same_bits(p, q) for p, q in zip(g.params, before))
    assert int(g.updates) == 2 + 3
    sg.check()


# ------------------------------------------------------------------ 3. arity
def test_wrong_number_of_tensors_is_a_type_error_before_anything_runs():
    d = _data()
    label, feat, sens = _batch(d, np.arange(B_), "cpu")
    fair, plain = _make("fair", d, "cpu"), _make("train", d, "cpu")
    assert plain.inputs == ("label", "feat")
    assert fair.inputs == mpvae_step.CalibrationStep.inputs == ("label", "feat", "sensitive_feat")
    for step, batch, match in ((fair, (label, feat), "sensitive_feat"),
                               (plain, (label, feat, sens), r"\(label, feat\)")):
        before = [t.clone() for t in step.model.state_dict().values()]
        seed = int(step.args.mpvae_seed)
        with pytest.raises(TypeError, match=match):
            step.step(*batch)
        with pytest.raises(TypeError, match=match):
            step(*batch)
        with pytest.raises(TypeError, match=match):
            step.capture(*batch, warmup=1)
        assert int(step.updates) == 0 and int(step.args.mpvae_seed) == seed
        assert step.graph is None and not step.opt.state
        assert all(p.grad is None for p in step.params)
        assert all(same_bits(u, v) for u, v in zip(step.model.state_dict().values(), before))


# ---------------------------------------------------------- 4. a raising body
@pytest.mark.gpu
def test_validate_that_raises_leaves_nothing_behind():
    """validate() on a model whose forward raises: the model's mode is put
    back, and the next step equals that of a twin that never saw the failure."""
    d = _data()
    hit, twin = _make("fair", d), _make("fair", d)
    b0, b1 = _batch(d, np.arange(B_)), _batch(d, np.arange(B_, 2 * B_))
    hit.step(*b0)
    twin.step(*b0)

    def broken(label, feat):
        raise RuntimeError("forward failed")
    for training in (True, False):
        hit.model.train(training)
        hit.model.forward = broken
        with pytest.raises(RuntimeError, match="forward failed"):
            hit.validate(*b1)
        del hit.model.forward
        assert hit.model.training is training
    hit.model.train()
    got, want = hit.step(*b1), twin.step(*b1)
    _assert_twins(hit, twin, got, want, "the step after the failure")
    assert int(hit.updates) == 2
