"""The per-step random r_sqrt_sigma on the device (``args.mpvae_r_draw``):
mpv_r_uniform_philox against its numpy restatement (tests/r_draw_ref.py) bit for
bit between guard bands, its argument checks, the separation of its stream from
the probit noise's, and the steps that draw with it -- eager against a hand
loop, captured against eager, single steps and epochs.

Steps: B 8, S 16, L 25, z 10, F 20, d 8; N = 29 rows (three batches and a tail
of 5), two sensitive patterns.  Dropout and the reparameterisation noise are
off wherever a capture is compared, so that a step draws nothing from torch's
generator (a capture would draw it at another offset)."""
import argparse
import copy
import ctypes

import numpy as np
import pytest
import torch

import guarded_alloc
import mpvae
import mpvae_fair as mf
import mpvae_hip as H
import mpvae_step
import r_draw_ref
from guarded_alloc import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096  # bytes on either side of every buffer
T_, MAXB = H.R_UNIFORM_THREADS, H.R_UNIFORM_MAX_BLOCKS
CAP = 2 * T_  # doubles of one full workgroup
M64 = 2 ** 64


def _i64(u):
    """The int64 with the bits of the 64-bit key u."""
    u %= M64
    return u - M64 if u >= 2 ** 63 else u


# ------------------------------------------------------ kernel vs restatement
def _kernel(L, z, bound, key, offset, dev_key, shift=0):
    """mpv_r_uniform_philox into a guarded (L, z) buffer (``shift``: starting 8
    bytes past a 16-B boundary, the scalar-store path); the device key, when
    used, is a guarded input.  Guards, the key and the shifted-over element are
    checked before the result is returned."""
    g = guarded_alloc.GuardedTorch(torch, GUARD, GUARD)
    n = L * z
    flat = g.alloc_like(torch.full((n + shift,), float("nan"), dtype=torch.float64, device=DEV),
                        "output")
    out = flat[shift:]
    assert out.data_ptr() % 16 == 8 * shift
    seed = g.alloc_like(torch.tensor([_i64(key)], dtype=torch.int64, device=DEV)) \
        if dev_key else None
    rc = H.load_library().mpv_r_uniform_philox(L, z, bound, 0 if dev_key else key % M64,
                                               H.ptr(seed), offset % M64, H.ptr(out),
                                               H.stream_of(DEV))
    H.check(rc, "mpv_r_uniform_philox")
    g.assert_clean()
    assert bool(torch.isnan(flat[:shift]).all())
    return out.view(L, z)


def _assert_kernel(L, z, key, offset=0, dev_key=False, shift=0):
    b = r_draw_ref.bound_of(L, z)
    got = _kernel(L, z, b, key, offset, dev_key, shift)
    want = torch.from_numpy(r_draw_ref.r_uniform(L, z, b, key, offset)).to(DEV)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (L, z, key, offset)


@pytest.mark.parametrize("dev_key", [False, True])
@pytest.mark.parametrize("L,z", [(1, 1), (3, 5), (25, 10), (38, 38), (128, 128)])
def test_kernel_is_the_restatement_at_the_models_shapes(L, z, dev_key):
    _assert_kernel(L, z, 41, dev_key=dev_key)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [CAP - 1, CAP, CAP + 1, CAP * MAXB + 3])
def test_kernel_at_workgroup_and_grid_edges(n, shift):
    """One short of, equal to and one past what one workgroup writes (two
    doubles per thread), and a count whose last counters fall to the grid's
    second pass -- with 16-B stores and, from an odd double, scalar ones."""
    assert (n + 1) // 2 > T_ * MAXB or n <= CAP + 1
    _assert_kernel(1, n, 0x5EED, dev_key=bool(shift), shift=shift)


@pytest.mark.parametrize("dev_key", [False, True])
@pytest.mark.parametrize("offset", [0, 2 ** 32 - 1, 2 ** 64 - 1])
def test_kernel_counter_carries_and_wraps(offset, dev_key):
    """Offset 2^32 - 1: the second counter carries into the high word; 2^64 - 1:
    the second counter wraps to 0."""
    _assert_kernel(25, 10, 77, offset=offset, dev_key=dev_key)


@pytest.mark.parametrize("dev_key", [False, True])
@pytest.mark.parametrize("key", [0x123456789ABCDEF0, 0xFEDCBA9876543210, -3 % M64, 1 << 32])
def test_kernel_keys_with_a_high_word(key, dev_key):
    """Keys above 2^32, and above 2^63: negative as the int64 a device key is."""
    if dev_key and key >= 2 ** 63:
        assert _i64(key) < 0
    _assert_kernel(3, 5, key, offset=5, dev_key=dev_key)


def test_kernel_rejects_bad_arguments_before_any_launch():
    g = guarded_alloc.GuardedTorch(torch, GUARD, GUARD)
    out = g.alloc_like(torch.full((4, 4), float("nan"), dtype=torch.float64, device=DEV), "output")
    lib, st, b = H.load_library(), H.stream_of(DEV), 0.5
    bad = [(0, 4, b, out), (4, 0, b, out), (-1, 4, b, out), (1 << 20, 1 << 20, b, out),
           (1 << 40, 1, b, out), (1, 1 << 40, b, out), (1 << 62, 1 << 62, b, out),
           (4, 4, b, None), (4, 4, 0.0, out), (4, 4, -0.5, out), (4, 4, float("nan"), out),
           (4, 4, float("inf"), out), (4, 4, float("-inf"), out)]
    for L, z, bound, o in bad:
        assert lib.mpv_r_uniform_philox(L, z, bound, 1, None, 0, H.ptr(o), st) == H.EINVAL, \
            (L, z, bound)
        assert lib.mpv_last_error()
    torch.cuda.synchronize()
    g.assert_clean()
    assert bool(torch.isnan(out).all())
    assert lib.mpv_r_uniform_philox(4, 4, b, 1, None, 0, H.ptr(out), st) == H.OK
    assert bool((out.abs() <= b).all())


def test_draw_function_philox_mode():
    """draw_r_sqrt_sigma: key args.mpvae_seed (an int or the device tensor),
    offset 0, the reference's bound; ``out`` is filled in place; a bad device
    seed is HipShardBackend._check_seed's ValueError."""
    b = r_draw_ref.bound_of(25, 10)
    a = argparse.Namespace(label_dim=25, z_dim=10, mpvae_r_draw="philox", mpvae_seed=-5)
    want = torch.from_numpy(r_draw_ref.r_uniform(25, 10, b, -5)).to(DEV)
    r = mpvae.draw_r_sqrt_sigma(a, DEV)
    assert same_bits(r, want) and not r.requires_grad
    a.mpvae_seed = torch.tensor([-5], dtype=torch.int64, device=DEV)
    buf = torch.zeros((25, 10), dtype=torch.float64, device=DEV)
    assert mpvae.draw_r_sqrt_sigma(a, DEV, out=buf) is buf and same_bits(buf, want)
    assert int(a.mpvae_seed) == -5  # read, not advanced
    for seed in (torch.tensor([1], dtype=torch.int64), None,
                 torch.tensor([1, 2], dtype=torch.int64, device=DEV),
                 torch.tensor([1], dtype=torch.int32, device=DEV)):
        a.mpvae_seed = seed
        with pytest.raises(ValueError, match="seed"):
            mpvae.draw_r_sqrt_sigma(a, DEV)
    H.load_library().mpv_timing_enable(1)
    try:
        H.load_library().mpv_timing_reset()
        a.mpvae_seed = 3
        mpvae.draw_r_sqrt_sigma(a, DEV, out=buf)
        assert H.kernel_times()["r_uniform"][0] == 1
    finally:
        H.load_library().mpv_timing_enable(0)
        H.load_library().mpv_timing_reset()


# ------------------------------------------------------------------ the steps
N_, B_, S_, L_, Z_, F_, D_ = 29, 8, 16, 25, 10, 20, 8
KEY0 = 41
CENTROIDS = np.array([[0, 0], [0, 1]], np.int64)


def _args(**kw):
    a = argparse.Namespace(feature_dim=F_, latent_dim=D_, label_dim=L_, z_dim=Z_, keep_prob=0.0,
                           scale_coeff=1.0, residue_sigma="random", n_train_sample=S_,
                           n_test_sample=S_, mode="train", nll_coeff=0.5, c_coeff=10.0,
                           mpvae_noise="philox",
                           mpvae_seed=torch.tensor([KEY0], dtype=torch.int64, device=DEV),
                           mpvae_r_draw="philox", fair_coeff=2.0, fairness_loss_norm="l2",
                           learn_logit=True)
    a.__dict__.update(kw)
    return a


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(0)
    labels = (rng.random((N_, L_)) < 0.4).astype(np.uint8)
    labels[:, 0], labels[:, 1] = 1, 0
    dists = {"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1)) for r in labels[::2]}
    return dict(labels=labels, feats=rng.standard_normal((N_, F_)),
                sens=CENTROIDS[np.arange(N_) % 2], dists=dists)


def _batch(d, rows):
    return (torch.from_numpy(d["labels"][rows]).float().to(DEV),
            torch.from_numpy(d["feats"][rows]).float().to(DEV),
            torch.from_numpy(d["sens"][rows]).to(DEV))


def _make(kind, d, **kw):
    args = _args(**kw)
    torch.manual_seed(3)
    np.random.seed(3)
    model = mpvae.VAE(args).to(DEV).train()
    if args.keep_prob == 0.0:
        model.reparam_noise = torch.zeros_like
    tables = [mf.LabelDistanceTable(d["dists"], L_, DEV)]
    if kind == "calib":
        thr = torch.rand(1, L_, 2, generator=torch.Generator().manual_seed(1)) * .1 + .45
        x = torch.log(thr / (1 - thr)).to(DEV).requires_grad_(True)
        opt = torch.optim.Adam([x], lr=2e-2, weight_decay=1e-5, fused=True, capturable=True)
        sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
        return mpvae_step.CalibrationStep(model, x, opt, args, tables,
                                          torch.from_numpy(CENTROIDS).to(DEV), scheduler=sched)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5, fused=True,
                           capturable=True)
    if kind == "train":
        return mpvae_step.TrainStep(model, opt, args)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    return mpvae_step.FairTrainStep(model, opt, args, tables, max_groups=2, scheduler=sched)


def _take(step, d, rows):
    return _batch(d, rows)[:len(step.inputs)]


def _state(step):
    """Everything a step changes: parameters and buffers, the Adam state, the
    update count, the Philox key, the drawn R and the device StepLR."""
    out = [p.detach() for p in step.params] + list(step.model.state_dict().values())
    for p in step.params:
        out += [v for _, v in sorted(step.opt.state[p].items())]
    sched = [] if step.sched is None else [step.sched.lr, step.sched.last_epoch]
    drawn = [] if step.r_drawn is None else [step.r_drawn]
    return out + [step.updates, step.args.mpvae_seed] + sched + drawn


def _tensors(out):
    return [t for t in out if isinstance(t, torch.Tensor)]


def _same(got, want):
    if isinstance(want, int):
        return got == want
    got, want = _tensors(got), _tensors(want)
    return len(got) == len(want) and all(same_bits(a, b) for a, b in zip(got, want))


def _assert_twins(g, a, got, want, what):
    torch.cuda.synchronize()
    assert _same(got, want), what
    sg, sa = _state(g), _state(a)
    assert len(sg) == len(sa) and all(same_bits(u, v) for u, v in zip(sg, sa)), what
    if isinstance(g, mpvae_step.FairTrainStep):
        assert g.read_totals(reset=False) == a.read_totals(reset=False), what


def _r_ref(key):
    return torch.from_numpy(r_draw_ref.r_uniform(L_, Z_, r_draw_ref.bound_of(L_, Z_), key)).to(DEV)


class _ModelR:
    """model.r_sqrt_sigma keeps its bits and gets no gradient."""

    def __init__(self, step):
        self.p = step.model.r_sqrt_sigma
        self.bits = self.p.detach().clone()

    def check(self):
        assert same_bits(self.p.detach(), self.bits) and self.p.grad is None
        assert not self.p.requires_grad


def test_stream_separation_the_noise_is_the_same_with_and_without_the_draw(data):
    """One TrainStep step with the device draw under key k, and compute_loss on
    a twin model's forward with the restated R(k) passed explicitly under the
    same key (no draw launch at all): the eight outputs are equal bit for bit,
    so the draw consumed nothing of the noise's stream."""
    ts = _make("train", data)
    twin = copy.deepcopy(ts.model)
    twin.reparam_noise = torch.zeros_like
    label, feat = _take(ts, data, np.arange(B_))
    got = ts(label, feat)
    assert same_bits(ts.r_drawn, _r_ref(KEY0))
    plain = _args(mpvae_r_draw=None, mpvae_seed=KEY0)
    want = mpvae.compute_loss(label, *twin(label, feat), _r_ref(KEY0), plain)
    assert len(got) == 8 and _same(got, want)
    # and another R under the same key gives other outputs: R is what differed
    other = mpvae.compute_loss(label, *twin(label, feat), twin.r_sqrt_sigma, plain)
    assert not same_bits(got[6], other[6])


def test_train_step_draws_a_fresh_r_every_step_and_equals_a_hand_loop(data):
    """Four eager steps: r_drawn after step i is the restatement at key0 + i,
    and outputs and state equal a loop of draw_r_sqrt_sigma + compute_loss."""
    ts, hand = _make("train", data), _make("train", data, mpvae_r_draw=None)
    keep = [_ModelR(ts), _ModelR(hand)]
    draw_args = _args(mpvae_seed=hand.args.mpvae_seed)  # the hand loop's key, shared
    for i in range(4):
        label, feat = _take(ts, data, np.arange(B_) + 5 * i)
        got = ts(label, feat)
        assert same_bits(ts.r_drawn, _r_ref(KEY0 + i)), i
        assert int(ts.args.mpvae_seed) == KEY0 + i + 1
        hand.opt.zero_grad(set_to_none=True)
        fwd = hand.model(label, feat)
        r = mpvae.draw_r_sqrt_sigma(draw_args, DEV)
        want = mpvae.compute_loss(label, *fwd, r, mpvae_step.step_args(hand.args))
        want[0].backward()
        hand._clip()
        hand._gated_update()
        assert _same(got, want), i
        hand.r_drawn = r  # for _state's comparison
        _assert_twins(ts, hand, got, want, i)
        hand.r_drawn = None
        for k in keep:
            k.check()
    assert int(ts.updates) == 4


@pytest.mark.parametrize("kind", ["train", "fair", "calib"])
def test_captured_step_equals_eager(kind, data):
    """capture() (two warm-up steps), then four replays, against an eager twin's
    six steps: outputs, parameters, optimizer state, ``updates``, the final key
    and every drawn R, bit for bit."""
    g, a = _make(kind, data), _make(kind, data)
    keep = [_ModelR(g), _ModelR(a)]
    batch0 = _take(g, data, np.arange(B_))
    g.capture(*batch0, warmup=2)
    assert g.graph is not None
    a.step(*batch0)
    a.step(*batch0)
    _assert_twins(g, a, 0, 0, "after the capture")
    for i in range(4):
        batch = _take(g, data, np.arange(B_) + 5 * i + 1)
        got, want = g(*batch), a(*batch)
        _assert_twins(g, a, got, want, i)
        assert same_bits(g.r_drawn, _r_ref(KEY0 + 2 + i)), i
        for k in keep:
            k.check()
    assert int(g.updates) == int(a.updates) == 6
    assert int(g.args.mpvae_seed) == int(a.args.mpvae_seed) == KEY0 + 6


@pytest.mark.parametrize("kind", ["train", "fair", "calib"])
def test_epochs_captured_and_eager(kind, data):
    """run_epoch over three batches and a tail of 5, eager and through
    capture_epoch: the same steps, state and draws; the last draw of epoch e is
    the restatement at the key of its last step."""
    g, a = _make(kind, data), _make(kind, data)
    keep = [_ModelR(g), _ModelR(a)]
    rng = np.random.default_rng(4)
    orders = [rng.permutation(N_) for _ in range(3)]
    sg, sa = (mpvae_step.DeviceSplit(data["labels"], data["feats"], data["sens"], device=DEV)
              for _ in range(2))
    for s in (sg, sa):
        s.set_order(orders[0])
    g.capture_epoch(sg, B_, warmup=1)
    a.step(*_take(a, data, orders[0][:B_]))
    _assert_twins(g, a, 0, 0, "after the capture")
    for e, order in enumerate(orders[1:]):
        got, want = g.run_epoch(sg, order, B_), a.run_epoch(sa, order, B_)
        assert got == want == 4
        _assert_twins(g, a, got, want, e)
        assert same_bits(g.r_drawn, _r_ref(KEY0 + 1 + 4 * (e + 1) - 1)), e
        for k in keep:
            k.check()
    sg.check()
    sa.check()
    assert int(g.updates) == 1 + 8


def test_validate_draws_too(data):
    """FairTrainStep.validate and validate_epoch draw a fresh R per batch."""
    f = _make("fair", data)
    keep = _ModelR(f)
    f.validate(*_batch(data, np.arange(B_)))
    assert same_bits(f.r_drawn, _r_ref(KEY0))
    split = mpvae_step.DeviceSplit(data["labels"], data["feats"], data["sens"], device=DEV)
    assert f.validate_epoch(split, None, B_) == 4
    assert same_bits(f.r_drawn, _r_ref(KEY0 + 4)) and int(f.args.mpvae_seed) == KEY0 + 5
    assert int(f.updates) == 0
    keep.check()


# ------------------------------------- "numpy" mode on the GPU-only step classes
def _numpy_kw():
    return dict(mpvae_r_draw="numpy", mpvae_noise="torch_cpu", mpvae_seed=None, keep_prob=0.5)


def _reference_draw(args):
    return torch.from_numpy(
        np.random.uniform(-np.sqrt(6.0 / (args.label_dim + args.z_dim)),
                          np.sqrt(6.0 / (args.label_dim + args.z_dim)),
                          (args.label_dim, args.z_dim))).to(DEV)


def _seed_all(seed):
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)


def test_numpy_mode_validate_is_the_reference_loop(data):
    """One FairTrainStep.validate batch with "numpy", torch_cpu noise and
    dropout on, against the hand loop with the reference's line
    (fairsoft_train.py:247-256): outputs and numpy's stream position."""
    ours, hand = _make("fair", data, **_numpy_kw()), \
        _make("fair", data, **dict(_numpy_kw(), mpvae_r_draw=None))
    label, feat, sens = _batch(data, np.arange(B_))
    _seed_all(9)
    got = ours.validate(label, feat, sens)
    tail = np.random.random()
    _seed_all(9)
    with mpvae_step._eval_mode(hand.model):
        fwd = hand.model(label, feat)
        res = mpvae.compute_loss(label, *fwd, _reference_draw(hand.args), hand.args)
        fair, contributed = mf.fairness_penalty(res[7], res[6], label, sens, hand.tables, "l2",
                                                hand.args.fair_coeff, max_groups=2, fused=True)
    assert np.random.random() == tail
    assert all(same_bits(a, b) for a, b in zip(got[1:8], res[1:]))
    assert same_bits(got.fairloss, fair.detach()) and int(got.contributed) == int(contributed)
    assert same_bits(got.total, (res[0].to(torch.float64) + fair).float())


def test_numpy_mode_calibration_step_is_the_reference_loop(data):
    """One CalibrationStep step with "numpy" against the hand loop with the
    reference's line (fairsoft_train_postprocess.py:97-106)."""
    ours, hand = _make("calib", data, **_numpy_kw()), \
        _make("calib", data, **dict(_numpy_kw(), mpvae_r_draw=None))
    label, feat, sens = _batch(data, np.arange(B_))
    _seed_all(9)
    total, bce, fair, cal, contributed = ours.step(label, feat, sens)
    tail = np.random.random()
    _seed_all(9)
    hand.opt.zero_grad(set_to_none=True)
    with torch.no_grad():
        fwd = hand.model(label, feat)
        res = mpvae.compute_loss(label, *fwd, _reference_draw(hand.args), hand.args)
    rb, rf, rc, ract, rn = mf.calibration_loss(res[6], hand.threshold_, label, sens,
                                               hand.centroids, hand.tables, True)
    assert bool(ract)
    (rf * hand.args.fair_coeff + rb).backward()
    hand._gated_update()
    assert np.random.random() == tail
    assert same_bits(cal, rc) and same_bits(bce, rb.detach()) and same_bits(fair, rf.detach())
    assert same_bits(total, (rf * hand.args.fair_coeff + rb).detach())
    assert same_bits(ours.threshold_.detach(), hand.threshold_.detach())
    assert ours.model.r_sqrt_sigma.grad is None
