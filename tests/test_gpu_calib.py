"""GPU: post-process threshold calibration (csrc/calib.hip through
mpvae_fair.calibration_loss / calibrate / fair_mean_diff and
mpvae_step.CalibrationStep) against the golden records of the reference, the
restatement tests/calib_ref.py at the kernels' edges, and torch's own Adam.

Tolerances.  The kernels compute in fp64 from the fp32 inputs, so against the
fp64 record (or the fp64 restatement) the losses differ by the order of a few
hundred fp64 additions and libm ulps (1e-10 relative is ample), ``bce`` after
its cast by half an fp32 ulp more (1.2e-7 in all), ``cal_prob`` by its one
rounding to fp32 (one ulp) and the fp32 gradients by theirs (1e-6 of the
tensor's largest entry, as tests/test_gpu_fair.py).  Against the fp32 record
-- the reference as it is -- the bound is twice the reference's own recorded
|fp32 - fp64| of that tensor plus the same rounding term.

Measured on the MI355X over the eight golden cases, against the fp64 record:
losses <= 2.1e-16 relative, ``cal_prob`` <= 0.50 fp32 ulp, gradients <= 5.4e-8
of the largest entry; against the fp32 record the threshold gradient sits at
the reference's own gap (1.5e-7 to 7.5e-7, 1.2e-3 on the edge draw)."""
import argparse

import numpy as np
import pytest
import torch

import calib_ref as cr
import mpvae
import mpvae_fair as mf
import mpvae_hip as H
import mpvae_step
from calib_io import calib_fixtures, gap
from tolerances import GRAD_RTOL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAL = calib_fixtures()
BY = {f["name"]: f for f in CAL}
LOSS_RTOL, BCE_F32_RTOL, GRAD_RND = 1e-10, 1.2e-7, 1e-6


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _tables(f):
    return [mf.LabelDistanceTable(d, f["labels"].shape[1], DEV) for d in f["dists"]]


def _raw(f, R, g_bce=1.0, g_fair=1.0, p_grad=True):
    """The autograd Function itself: the fp64 losses before calibration_loss
    casts them, and the gradients of g_bce * bce + g_fair * fair."""
    p = _dev(f["p"]).requires_grad_(p_grad)
    x = _dev(f["threshold"]).requires_grad_(True)
    y = _dev(f["labels"], torch.float32)
    tables = _tables(f)
    w = mf.label_weights(y, tables)[0] if tables else None
    G = len(f["centroids"])
    gid, unmatched = mf.centroid_ids(_dev(f["sensitive"]), _dev(f["centroids"]))
    order, goff = mf._group_layout(gid, G)
    bce, fair, cal, nterms = mf._Calibration.apply(p, x, y, w, order, goff, G, R, f["learn_logit"])
    assert bce.dtype == fair.dtype == torch.float64 and not cal.requires_grad
    (g_bce * bce + g_fair * fair).backward()
    return dict(bce=float(bce.detach()), fair=float(fair.detach()), nterms=int(nterms),
                cal_prob=cal.cpu().numpy(), g_threshold=x.grad.cpu().numpy(),
                g_p=p.grad.cpu().numpy() if p_grad else None, bits=(bce.detach(), fair.detach(),
                                                                   cal, x.grad, p.grad))


def _ulp32(ref64):
    return np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


def _check_values(got, ref, active):
    """One run against fp64 values of the same quantities: every element."""
    assert abs(got["bce"] - ref["bce"]) <= LOSS_RTOL * abs(ref["bce"])
    assert abs(got["fair"] - ref["fair"]) <= LOSS_RTOL * abs(ref["fair"])
    assert (got["nterms"] > 0) == active
    assert (np.abs(got["cal_prob"] - ref["cal_prob"]) <= _ulp32(ref["cal_prob"])).all()
    for k in ("g_threshold", "g_p"):
        assert np.abs(got[k] - ref[k]).max() <= GRAD_RND * np.abs(ref[k]).max(), k


# ------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("f", CAL, ids=[f["name"] for f in CAL])
def test_calibration_matches_the_golden_records(f):
    coeff = f["fair_coeff"]
    R = 2
    tot, bce_only = _raw(f, R, 1.0, coeff), _raw(f, R, 1.0, 0.0)
    runs = [("g_bce_", bce_only)] + ([("g_", tot)] if f["active"] else [])
    # against the fp64 record
    _check_values(dict(tot, g_threshold=bce_only["g_threshold"], g_p=bce_only["g_p"]),
                  dict(bce=float(f["bce_64"]), fair=float(f["fair_64"]), cal_prob=f["cal_prob_64"],
                       g_threshold=f["g_bce_threshold_64"], g_p=f["g_bce_p_64"]), f["active"])
    if f["active"]:
        total = tot["fair"] * coeff + tot["bce"]
        assert abs(total - float(f["total_64"])) <= LOSS_RTOL * abs(float(f["total_64"]))
        for k in ("threshold", "p"):
            ref = f[f"g_{k}_64"]
            assert np.abs(tot["g_" + k] - ref).max() <= GRAD_RND * np.abs(ref).max(), k
    # against the fp32 record: twice the reference's own fp32 error + the rounding
    for k in ("bce", "fair"):
        ref = float(f[k])
        assert abs(tot[k] - ref) <= 2 * gap(f, k) + BCE_F32_RTOL * abs(ref), k
    assert (np.abs(tot["cal_prob"] - f["cal_prob"])
            <= 2 * gap(f, "cal_prob") + _ulp32(f["cal_prob_64"])).all()
    for pre, run in runs:
        for k in ("threshold", "p"):
            ref = f[pre + k].astype(np.float64)
            assert np.abs(run["g_" + k] - ref).max() <= \
                2 * gap(f, pre + k) + GRAD_RND * np.abs(ref).max(), pre + k
    # the public call: the same numbers, cast as documented
    p, x = _dev(f["p"]).requires_grad_(True), _dev(f["threshold"]).requires_grad_(True)
    bce, fair, cal, active, contributed = mf.calibration_loss(
        p, x, _dev(f["labels"]), _dev(f["sensitive"]), _dev(f["centroids"]), _tables(f),
        f["learn_logit"], slices=R)
    assert bce.dtype == torch.float32 and active.dtype == torch.bool and active.dim() == 0
    assert float(bce.detach()) == float(np.float32(tot["bce"]))
    assert abs(float(bce.detach()) - float(f["bce_64"])) <= BCE_F32_RTOL * abs(float(f["bce_64"]))
    assert bool(active) == f["active"] and int(contributed) == int(f["contributed"])
    assert fair.dtype == (torch.float32 if f["pyfloat"] else torch.float64)
    if f["active"]:
        assert str(fair.dtype) == "torch." + str(f["fair_dtype"])
    assert float(fair.detach()) == float(torch.tensor(tot["fair"], dtype=torch.float64).to(fair.dtype))
    assert np.array_equal(cal.cpu().numpy(), tot["cal_prob"]) and not cal.requires_grad
    (fair * coeff + bce).backward()
    ref = f["g_threshold_64"] if f["active"] else f["g_bce_threshold_64"]
    assert np.abs(x.grad.cpu().numpy() - ref).max() <= GRAD_RND * np.abs(ref).max()


# ------------------------------------------------------------- 2. kernel edges
def _edge_case(B, L, T, G, empty_group, learn_logit, seed, small_group=False):
    rng = np.random.default_rng(seed)
    labels = (rng.random((B, L)) < 0.4).astype(np.int64)
    labels[B // 2:] = labels[:B - B // 2]
    cents = np.array([[k, 1] for k in range(G)], np.int64)
    live = [k for k in range(G) if k != empty_group]
    gsel = np.array([live[i % len(live)] for i in range(B)])
    if small_group and len(live) > 1:  # the last live group keeps two rows (or one)
        keep = np.where(gsel == live[-1])[0][:2]
        gsel[gsel == live[-1]] = live[0]
        gsel[keep] = live[-1]
    rng.shuffle(gsel)
    dists = [{"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1)) for r in labels[t::2]}
             for t in range(T)]
    thr = rng.uniform(0.3, 0.7, (1, L, G))
    return dict(p=rng.uniform(0.02, 0.98, (B, L)).astype(np.float32),
                threshold=(np.log(thr / (1 - thr)) if learn_logit else thr).astype(np.float32),
                labels=labels, sensitive=cents[gsel], centroids=cents, dists=dists,
                learn_logit=learn_logit)


# B, L, T, G, the group with no rows (-1: none), learn_logit, R > 1, a two-row group
EDGES = {
    "one_row": (1, 5, 1, 2, 1, True, 3, False),
    "one_label_one_group": (7, 1, 1, 1, -1, False, 2, False),
    "l257_t3_g5_small_group": (37, 257, 3, 5, -1, True, 4, True),       # two rows < R slices
    "no_tables": (53, 38, 0, 3, -1, False, 3, False),
    "t5_past_the_register_tile": (41, 300, 5, 2, -1, True, 8, False),  # kCalTile = 4 targets
    "zero_row_group_g5": (19, 12, 3, 5, 2, False, 7, True),
    "l256_exact": (23, 256, 2, 3, -1, True, 5, False),
}


@pytest.mark.parametrize("name", EDGES)
def test_kernel_edges_against_the_restatement(name):
    B, L, T, G, empty, ll, R, small = EDGES[name]
    f = _edge_case(B, L, T, G, empty, ll, seed=len(name), small_group=small)
    ref = cr.run64(f["p"], f["threshold"], f["labels"], f["sensitive"], f["centroids"], f["dists"],
                   ll, g_bce=0.75, g_fair=1.5)
    one, many, again = (_raw(f, r, 0.75, 1.5) for r in (1, R, R))
    for run in (one, many):
        _check_values(run, ref, ref["nterms"] > 0)
        assert run["nterms"] == ref["nterms"]
    if empty >= 0:  # the thresholds of a group without rows get an exact zero
        assert (many["g_threshold"][0, :, empty] == 0).all()
    # two calls: the same bits; R = 1 and R > 1: equal to rounding
    assert all(torch.equal(a, b) for a, b in zip(many["bits"], again["bits"]))
    for k in ("bce", "fair"):
        assert abs(one[k] - many[k]) <= 1e-12 * abs(many[k]), k
    assert (np.abs(one["cal_prob"] - many["cal_prob"]) <= _ulp32(ref["cal_prob"])).all()
    for k in ("g_threshold", "g_p"):
        assert np.abs(one[k] - many[k]).max() <= 2.0 ** -23 * np.abs(many[k]).max(), k


# -------------------------------------------------------- 3. needs_input_grad
def test_detached_indiv_prob_gets_no_gradient_buffer(monkeypatch):
    f = BY["c1_logit"]
    lib, seen = H.load_library(), []
    native = lib.mpv_calib_bwd

    def spy(a, gout, gx, gp, ws, n, st):
        seen.append(gp)
        return native(a, gout, gx, gp, ws, n, st)

    monkeypatch.setattr(lib, "mpv_calib_bwd", spy)
    both = _raw(f, 3, 1.0, f["fair_coeff"], p_grad=True)
    only_x = _raw(f, 3, 1.0, f["fair_coeff"], p_grad=False)
    assert seen[0] is not None and seen[1] is None  # NULL: no d indiv_prob pass
    assert only_x["g_p"] is None
    assert np.array_equal(both["g_threshold"], only_x["g_threshold"])


# ------------------------------------------------- 4. chained through compute_loss
def test_gradient_chains_through_compute_loss():
    torch.manual_seed(5)
    rng = np.random.default_rng(5)
    B, L, z, d, S = 24, 10, 6, 8, 16
    args = argparse.Namespace(n_train_sample=S, n_test_sample=S, mode="train", nll_coeff=0.5,
                              c_coeff=10.0, z_dim=z, label_dim=L,
                              mpvae_noise=torch.randn(S, B, z, device=DEV))
    y = (torch.rand(B, L) < 0.3).float()
    y[:, 0], y[:, 1] = 1, 0
    y[B // 2:] = y[:B // 2]
    y = y.to(DEV)
    leaves = [torch.randn(B, n, device=DEV) * s for n, s in ((L, 1), (d, .3), (d, .3), (L, 1),
                                                             (d, .3), (d, .3))]
    Rm = (torch.randn(L, z, dtype=torch.float64, device=DEV) * 0.3)
    cents = torch.tensor([[0, 0], [0, 1], [1, 1]], device=DEV)
    sens = cents[torch.from_numpy(rng.integers(0, 3, B)).to(DEV)]
    ynp = y.cpu().numpy().astype(np.int64)
    dists = [{"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1)) for r in ynp[t::2]}
             for t in range(2)]
    tables = [mf.LabelDistanceTable(dd, L, DEV) for dd in dists]
    x0 = torch.from_numpy(rng.uniform(-0.4, 0.4, (1, L, 3)).astype(np.float32)).to(DEV)
    coeff = 1.3

    def grads(kernel):
        ins = [t.clone().requires_grad_(True) for t in leaves]
        Rl = Rm.clone().requires_grad_(True)
        x = x0.clone().requires_grad_(True)
        res = mpvae.compute_loss(y, *ins, Rl, args)
        if kernel:
            bce, fair, _, active, _ = mf.calibration_loss(res[6], x, y, sens, cents, tables, True)
            assert bool(active)
        else:  # the torch-op restatement on the same indiv_prob tensor, fp64
            gid = mf.centroid_ids(sens, cents)[0].long()
            w = torch.from_numpy(cr.weights(ynp, dists)).to(DEV)
            bce, fair, n, _ = cr.losses(res[6].double(), x.double(), y.double(), gid, w, True)
            assert n > 0
        (fair * coeff + bce).backward()
        return ins[0].grad, ins[3].grad, Rl.grad, x.grad

    ours, ref = grads(True), grads(False)
    # indiv_prob is the feature branch's: nothing reaches fe_out on either side
    assert all(g is None or not g.any() for g in (ours[0], ref[0]))
    for k, a, b in zip(("fx_out", "R", "threshold"), ours[1:], ref[1:]):
        assert float(b.abs().max()) > 0, k
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= GRAD_RTOL, k


# ------------------------------------------------------------ the step's fixture
def _step_setup(learn_logit=True, seed=11, lr=2e-2):
    """A small frozen VAE, thresholds, tables hitting half of the label
    patterns, and batches: three active ones and one no dict knows."""
    F_, L, G, B = 12, 9, 3, 20
    a = argparse.Namespace(feature_dim=F_, latent_dim=6, label_dim=L, z_dim=5, keep_prob=0.5,
                           scale_coeff=1.0, residue_sigma="", n_train_sample=8, n_test_sample=8,
                           mode="train", nll_coeff=0.5, c_coeff=10.0, mpvae_noise="philox",
                           mpvae_seed=torch.tensor([seed], dtype=torch.int64, device=DEV),
                           fair_coeff=1.7, learn_logit=learn_logit)
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = mpvae.VAE(a).to(DEV).eval()
    model.reparam_noise = torch.zeros_like
    g = torch.Generator().manual_seed(seed)
    cents = torch.tensor([[0, 0], [0, 1], [1, 0]], device=DEV)
    batches, known = [], {}
    for i in range(4):
        y = (torch.rand(B, L, generator=g) < 0.35).float()
        y[:, 0], y[:, 1] = (1, 0) if i < 3 else (0, 1)  # the last batch: patterns of its own
        for r in y[::2] if i < 3 else []:
            known["".join(str(int(v)) for v in r)] = np.float64(0.2 + 0.1 * (len(known) % 7))
        sens = cents[torch.randint(0, G, (B,), generator=g)]
        batches.append((y.to(DEV), torch.randn(B, F_, generator=g).to(DEV), sens))
    tables = [mf.LabelDistanceTable(known, L, DEV)]
    thr = torch.rand(1, L, G, generator=g) * .1 + .45
    x = (torch.log(thr / (1 - thr)) if learn_logit else thr).to(DEV).requires_grad_(True)
    opt = torch.optim.Adam([x], lr=lr, weight_decay=1e-5, fused=True, capturable=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    return a, model, x, opt, sched, tables, cents, batches


# ------------------------------------------------------------ 5. NaN behaviour
def test_unmatched_row_gives_nan_losses():
    f = BY["c1_logit"]
    sens = f["sensitive"].copy()
    sens[3] = 9
    bce, fair, cal, active, _ = mf.calibration_loss(
        _dev(f["p"]), _dev(f["threshold"]).requires_grad_(True), _dev(f["labels"]), _dev(sens),
        _dev(f["centroids"]), _tables(f), True)
    assert torch.isnan(bce) and torch.isnan(fair) and bce.dtype == torch.float32


def test_bad_threshold_is_nan_and_the_step_skips_the_update():
    a, model, x, opt, sched, tables, cents, batches = _step_setup(learn_logit=False)
    step = mpvae_step.CalibrationStep(model, x, opt, a, tables, cents, scheduler=sched)
    step.step(*batches[0])
    assert int(step.updates) == 1
    with torch.no_grad():
        x[0, 2, 1] = 1.5  # outside (0, 1): log of a negative number
    before = [t.clone() for t in (x, opt.state[x]["exp_avg"], opt.state[x]["exp_avg_sq"],
                                  opt.state[x]["step"], step.sched.lr, step.sched.last_epoch)]
    total, bce, fair, cal, _ = step.step(*batches[1])
    assert torch.isnan(x.grad).any() and torch.isnan(total)
    after = (x, opt.state[x]["exp_avg"], opt.state[x]["exp_avg_sq"], opt.state[x]["step"],
             step.sched.lr, step.sched.last_epoch)
    assert all(torch.equal(b, t) for b, t in zip(before, after))
    assert int(step.updates) == 1
    # not clamped either: the bad entry is still there (the reference's clip is a no-op)
    assert float(x.detach()[0, 2, 1]) == 1.5


# --------------------------------------------------------- 6. the step's plumbing
def test_step_equals_a_hand_written_loop():
    a1, m1, x1, o1, s1, tables, cents, batches = _step_setup()
    a2, m2, x2, o2, s2, _, _, _ = _step_setup()
    step = mpvae_step.CalibrationStep(m1, x1, o1, a1, tables, cents, scheduler=s1)
    a2.mpvae_seed_advance = True
    for i, (y, feat, sens) in enumerate(batches):
        total, bce, fair, cal, contributed = step.step(y, feat, sens)
        o2.zero_grad(set_to_none=True)
        with torch.no_grad():
            res = mpvae.compute_loss(y, *m2(y, feat), m2.r_sqrt_sigma, a2)
        rb, rf, rc, ract, rn = mf.calibration_loss(res[6], x2, y, sens, cents, tables, True)
        assert bool(ract) == (i < 3)
        rtotal = rf * a2.fair_coeff + rb
        if bool(ract):
            rtotal.backward()
        else:  # the reference's total does not reach threshold_: zeroed gradients
            x2.grad = torch.zeros_like(x2)
            rtotal = res[0]
        o2.step()
        s2.step()
        assert torch.equal(total, rtotal.detach().to(total.dtype)), i
        assert torch.equal(bce, rb.detach()) and torch.equal(fair, rf.detach())
        assert torch.equal(cal, rc) and int(contributed) == int(rn)
        assert torch.equal(x1, x2), i
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(o1.state[x1][k], o2.state[x2][k]), (i, k)
    assert int(contributed) == 0 and not x1.grad.any()  # the inactive batch
    assert int(step.updates) == 4
    assert step.sync_scheduler() == [o2.param_groups[0]["lr"]] == [2e-2 * 0.25]
    assert torch.equal(a1.mpvae_seed, a2.mpvae_seed)


def test_step_wants_a_native_adam_and_a_leaf():
    a, model, x, opt, sched, tables, cents, _ = _step_setup()
    with pytest.raises(ValueError, match="fused"):
        mpvae_step.CalibrationStep(model, x, torch.optim.Adam([x], lr=1e-3), a, tables, cents)
    with pytest.raises(ValueError, match="leaf"):
        mpvae_step.CalibrationStep(model, x * 1.0, opt, a, tables, cents)


# ------------------------------------------------------------ 7. graph capture
def test_calibration_loss_is_graph_capturable():
    f = BY["c4_dead_target"]
    tables, cents = _tables(f), _dev(f["centroids"])
    y, sens = _dev(f["labels"]), _dev(f["sensitive"])
    p, x = _dev(f["p"]).requires_grad_(True), _dev(f["threshold"]).requires_grad_(True)

    def run():
        bce, fair, cal, active, n = mf.calibration_loss(p, x, y, sens, cents, tables, False)
        (fair * 0.9 + bce).backward()
        return bce, fair, cal, active, n

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            p.grad = x.grad = None
            out = run()
    torch.cuda.current_stream().wait_stream(side)
    p.grad = x.grad = None
    del out
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    rng = np.random.default_rng(1)
    for it in range(2):
        with torch.no_grad():
            p.copy_(_dev(rng.uniform(0.02, 0.98, f["p"].shape).astype(np.float32)))
            sens.copy_(sens[torch.randperm(len(sens), device=DEV)])
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out + (p.grad, x.grad)]
        pe, xe = p.detach().clone().requires_grad_(True), x.detach().clone().requires_grad_(True)
        bce, fair, cal, active, n = mf.calibration_loss(pe, xe, y, sens, cents, tables, False)
        (fair * 0.9 + bce).backward()
        for a, b in zip(got, (bce, fair, cal, active, n, pe.grad, xe.grad)):
            assert torch.equal(a, b.detach())


def test_captured_step_equals_eager():
    ag, mg, xg, og, sg, tables, cents, batches = _step_setup()
    ae, me, xe, oe, se, _, _, _ = _step_setup()
    tg = mpvae_step.CalibrationStep(mg, xg, og, ag, tables, cents, scheduler=sg)
    te = mpvae_step.CalibrationStep(me, xe, oe, ae, tables, cents, scheduler=se)
    tg.capture(*batches[0], warmup=1)
    te.step(*batches[0])
    for b in batches[1:]:
        got = [o.clone() for o in tg.step(*b)]
        ref = te.step(*b)
        torch.cuda.synchronize()
        assert all(torch.equal(a, r) for a, r in zip(got, ref))
        assert torch.equal(xg, xe)
    assert int(tg.updates) == int(te.updates) == 4
    assert tg.sync_scheduler() == te.sync_scheduler() == [2e-2 * 0.25]


# --------------------------------------------------------------- 8. evaluation
@pytest.mark.parametrize("f", CAL, ids=[f["name"] for f in CAL])
def test_evaluation_matches_the_golden_block(f):
    sens, cents, tables = _dev(f["sensitive"]), _dev(f["centroids"]), _tables(f)
    cal = mf.calibrate(_dev(f["p"]), _dev(f["eval_threshold"]), sens, cents, slices=2)
    got = cal.cpu().numpy()
    assert cal.dtype == torch.float32
    assert (np.abs(got - f["eval_cal_prob_64"]) <= _ulp32(f["eval_cal_prob_64"])).all()
    assert (np.abs(got - f["eval_cal_prob"])
            <= 2 * gap(f, "eval_cal_prob") + _ulp32(f["eval_cal_prob_64"])).all()
    # the reference's numpy block is fp64 on its fp32 cal_prob: the same inputs here
    md = mf.fair_mean_diff(_dev(f["eval_cal_prob"]), _dev(f["labels"]), sens, cents, tables,
                           slices=2)
    ref = float(f["eval_mean_diff"])
    assert md.dtype == torch.float64 and md.dim() == 0
    if np.isnan(ref):
        assert not f["active"] and torch.isnan(md)
    else:
        assert abs(float(md) - ref) <= LOSS_RTOL * abs(ref)
    m = mf.compute_metrics(cal, _dev(f["labels"], torch.float32), 0.5)
    assert 0.0 <= float(m["ACC"]) <= 1.0 and 0.0 <= float(m["HA"]) <= 1.0


def test_fair_mean_diff_over_a_split():
    """A split of a few thousand rows with the default slices (R = 64 here)."""
    rng = np.random.default_rng(9)
    N, L, G = 4099, 38, 4
    labels = (rng.random((N, L)) < 0.1).astype(np.int64)
    labels[N // 3:] = labels[:N - N // 3]
    cents = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.int64)
    sens = cents[rng.integers(0, G, N)]
    dists = [{"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1)) for r in labels[t::5]}
             for t in range(2)]
    q = rng.uniform(0.01, 0.99, (N, L)).astype(np.float32)
    assert mf.calib_slices(N, L, G, DEV) > 1
    md = mf.fair_mean_diff(_dev(q), _dev(labels), _dev(sens), _dev(cents),
                           [mf.LabelDistanceTable(d, L, DEV) for d in dists])
    ref = cr.mean_diff(q, labels, sens, cents, dists)
    assert abs(float(md) - ref) <= LOSS_RTOL * abs(ref)
    assert torch.isnan(mf.fair_mean_diff(_dev(q), _dev(labels), _dev(sens), _dev(cents), []))
