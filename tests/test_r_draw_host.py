"""The per-step random r_sqrt_sigma (``args.mpvae_r_draw``) without a GPU: the
draw rule's word -> double -> affine map against numpy's own generator, the
distribution of the restated Philox draw (tests/r_draw_ref.py, which the kernel
is held to bit for bit in tests/test_gpu_r_draw.py), the "numpy" mode of
TrainStep against a hand-written loop with the reference's line, the refusals,
and the knob's default (absent: the model's r_sqrt_sigma, as before).

FairTrainStep.validate and CalibrationStep run their penalty, metrics and Adam
on the GPU only, so their "numpy" loops are compared in test_gpu_r_draw.py.

Shapes: B 8, S 16, L 25, z 10, F 20, d 8."""
import argparse

import numpy as np
import pytest
import torch

import mpvae
import mpvae_dist
import mpvae_step
import r_draw_ref
from guarded_alloc import same_bits

B_, S_, L_, Z_, F_, D_ = 8, 16, 25, 10, 20, 8


def _args(**kw):
    a = argparse.Namespace(feature_dim=F_, latent_dim=D_, label_dim=L_, z_dim=Z_, keep_prob=0.5,
                           scale_coeff=1.0, residue_sigma="random", n_train_sample=S_,
                           n_test_sample=S_, mode="train", nll_coeff=0.5, c_coeff=10.0)
    a.__dict__.update(kw)
    return a


def _batches(n):
    rng = np.random.default_rng(11)
    out = []
    for _ in range(n):
        y = (rng.random((B_, L_)) < 0.4).astype(np.float32)
        y[:, 0], y[:, 1] = 1, 0
        out.append((torch.from_numpy(y), torch.from_numpy(rng.standard_normal((B_, F_))).float()))
    return out


def _make(args, seed=5):
    np.random.seed(seed)
    torch.manual_seed(seed)
    model = mpvae.VAE(args).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5, fused=True)
    return mpvae_step.TrainStep(model, opt, args)


# ------------------------------------------------------------------ word rule
def test_word_rule_is_numpys_uniform_bit_for_bit():
    b = r_draw_ref.bound_of(38, 38)
    words = np.random.RandomState(7).randint(0, 2 ** 32, 2000, dtype=np.uint64)
    got = r_draw_ref.affine(r_draw_ref.doubles_from_words(words[0::2], words[1::2]), b)
    want = np.random.RandomState(7).uniform(-b, b, 1000)
    assert got.dtype == want.dtype == np.float64
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


# --------------------------------------------------------------- distribution
@pytest.mark.parametrize("L,z", [(38, 38), (25, 10), (128, 128), (1024, 1024)])
def test_restated_draw_is_uniform_in_the_bound(L, z):
    """Every value in [-b, b); the sample mean within 4 standard errors b /
    sqrt(3 n) of 0 and the sample variance within 4 of its standard errors
    b^2 sqrt(4 / (45 n)) of b^2 / 3 (the variance of (x - mu)^2 for a uniform
    is 4 b^4 / 45), for seeds 0..4."""
    b, n = r_draw_ref.bound_of(L, z), L * z
    for seed in range(5):
        r = r_draw_ref.r_uniform(L, z, b, seed)
        assert r.shape == (L, z) and r.dtype == np.float64
        assert r.min() >= -b and r.max() < b
        mean_err = abs(r.mean()) / (b / np.sqrt(3 * n))
        var_err = abs(r.var() - b * b / 3) / (b * b * np.sqrt(4 / (45 * n)))
        print(f"L={L} z={z} seed={seed}: mean {mean_err:.2f} se, variance {var_err:.2f} se")
        assert mean_err <= 4 and var_err <= 4, (seed, mean_err, var_err)


def test_restated_streams_differ_by_key_offset_and_domain():
    """Another key, another offset: other values; offset 1 is the draw shifted
    by one counter (two doubles); the noise's counter domain (third word 0)
    gives other words than the draw's (third word 1)."""
    from oracle.philox import philox4x32_10
    b = r_draw_ref.bound_of(L_, Z_)
    r0 = r_draw_ref.r_uniform(L_, Z_, b, 9)
    assert not np.array_equal(r0, r_draw_ref.r_uniform(L_, Z_, b, 10))
    r1 = r_draw_ref.r_uniform(L_, Z_, b, 9, offset=1)
    assert np.array_equal(r0.reshape(-1)[2:], r1.reshape(-1)[:-2])
    w_noise = philox4x32_10([0], [0], [0], [0], [9], [0])
    w_draw = philox4x32_10([0], [0], [1], [0], [9], [0])
    assert all(int(a[0]) != int(c[0]) for a, c in zip(w_noise, w_draw))


# ----------------------------------------------------- reference-loop equality
def test_numpy_mode_is_the_reference_loop_bit_for_bit():
    """Three TrainStep steps with mpvae_r_draw = "numpy" on CPU tensors against
    a loop that draws with the reference's own line (fairsoft_train.py:60-69)
    and calls compute_loss: the eight outputs of every step, every parameter
    afterwards and the position of numpy's global stream are the same."""
    batches = _batches(3)

    def run(hand):
        args = _args() if hand else _args(mpvae_r_draw="numpy")
        ts = _make(args)
        r0 = ts.model.r_sqrt_sigma.detach().clone()
        outs = []
        for label, feat in batches:
            if not hand:
                outs.append(ts(label, feat))
                continue
            ts.opt.zero_grad(set_to_none=True)
            fwd = ts.model(label, feat)
            r_sqrt_sigma = torch.from_numpy(
                np.random.uniform(-np.sqrt(6.0 / (args.label_dim + args.z_dim)),
                                  np.sqrt(6.0 / (args.label_dim + args.z_dim)),
                                  (args.label_dim, args.z_dim))).to("cpu")
            res = mpvae.compute_loss(label, *fwd, r_sqrt_sigma, args)
            res[0].backward()
            ts._clip()
            ts._gated_update()
            outs.append(res)
        assert same_bits(ts.model.r_sqrt_sigma, r0) and ts.model.r_sqrt_sigma.grad is None
        if not hand:
            assert ts.r_drawn.dtype == torch.float64 and not ts.r_drawn.requires_grad
            assert same_bits(ts.r_drawn, r_sqrt_sigma_of(3))
        return outs, [p.detach().clone() for p in ts.model.parameters()], np.random.random(), \
            int(ts.updates)

    def r_sqrt_sigma_of(step):
        """The draw of step `step` (1-based) on the seeded global stream."""
        state = np.random.get_state()
        try:
            _make(_args())  # seeds, and the model's own r_sqrt_sigma draw
            b = np.sqrt(6.0 / (L_ + Z_))
            for _ in range(step):
                r = np.random.uniform(-b, b, (L_, Z_))
            return torch.from_numpy(r)
        finally:
            np.random.set_state(state)

    got, want = run(False), run(True)
    assert got[3] == want[3] == 3
    for g, w in zip(got[0], want[0]):
        assert len(g) == len(w) == 8 and all(same_bits(a, c) for a, c in zip(g, w))
    assert len(got[1]) == len(want[1]) and all(same_bits(a, c) for a, c in zip(got[1], want[1]))
    assert got[2] == want[2]
    # three different draws were used: the outputs of two steps on one batch differ
    assert not same_bits(got[0][0][6], got[0][1][6])


def test_draw_function_numpy_mode_and_out():
    args = _args(mpvae_r_draw="numpy")
    b = np.sqrt(6.0 / (L_ + Z_))
    np.random.seed(2)
    want = np.random.uniform(-b, b, (L_, Z_))
    tail = np.random.random()
    np.random.seed(2)
    r = mpvae.draw_r_sqrt_sigma(args, "cpu")
    assert r.dtype == torch.float64 and same_bits(r, torch.from_numpy(want))
    assert np.random.random() == tail
    np.random.seed(2)
    buf = torch.zeros((L_, Z_), dtype=torch.float64)
    assert mpvae.draw_r_sqrt_sigma(args, "cpu", out=buf) is buf
    assert same_bits(buf, torch.from_numpy(want))
    for bad in (torch.zeros((L_, Z_)), torch.zeros((Z_, L_), dtype=torch.float64),
                torch.zeros((Z_, L_), dtype=torch.float64).t()):
        with pytest.raises(ValueError, match="out must be"):
            mpvae.draw_r_sqrt_sigma(args, "cpu", out=bad)
    with pytest.raises(ValueError, match="mpvae_r_draw"):
        mpvae.draw_r_sqrt_sigma(_args(), "cpu")
    with pytest.raises(ValueError, match="mpvae_r_draw"):
        mpvae.draw_r_sqrt_sigma(_args(mpvae_r_draw="mt19937"), "cpu")


# ------------------------------------------------------------------- refusals
def test_philox_draw_refuses_cpu_tensors():
    """As HostShardBackend.make_noise refuses Philox noise: a ValueError."""
    with pytest.raises(ValueError, match="draws on the GPU"):
        mpvae.draw_r_sqrt_sigma(_args(mpvae_r_draw="philox", mpvae_seed=3), "cpu")
    ts = _make(_args(mpvae_r_draw="philox", mpvae_seed=3))
    with pytest.raises(ValueError, match="draws on the GPU"):
        ts(*_batches(1)[0])


@pytest.mark.parametrize("residue_sigma", ["", "zero"])
@pytest.mark.parametrize("mode", ["numpy", "philox"])
def test_refused_without_a_random_model(residue_sigma, mode):
    with pytest.raises(ValueError, match="residue_sigma"):
        _make(_args(residue_sigma=residue_sigma, mpvae_r_draw=mode, mpvae_seed=1))


def test_refused_for_an_unknown_mode():
    with pytest.raises(ValueError, match="mpvae_r_draw"):
        _make(_args(mpvae_r_draw="host"))


def test_numpy_mode_refuses_a_capture():
    ts = _make(_args(mpvae_r_draw="numpy"))
    label, feat = _batches(1)[0]
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="on the host"):
        ts.capture(label, feat)
    split = mpvae_step.DeviceSplit(label.numpy(), feat.numpy())
    with pytest.raises(ValueError, match="on the host"):
        ts.capture_epoch(split, B_)
    assert ts.graph is None and int(ts.updates) == 0
    assert np.array_equal(np.random.get_state()[1], state)  # nothing was drawn


@pytest.mark.parametrize("kw", [dict(), dict(mpvae_noise="philox", mpvae_seed=7),
                                dict(mpvae_noise="torch_cpu",
                                     mpvae_seed=torch.tensor([7], dtype=torch.int64))])
def test_philox_mode_needs_device_philox_noise_to_capture(kw):
    """capture() with mpvae_r_draw = "philox" needs Philox noise and a device
    seed (the key the draw reads at every replay); the message says so."""
    kw.setdefault("mpvae_seed", 7)
    ts = _make(_args(mpvae_r_draw="philox", **kw))
    label, feat = _batches(1)[0]
    with pytest.raises(ValueError, match="mpvae_r_draw = 'philox' draws r_sqrt_sigma from the key"):
        ts.capture(label, feat)
    with pytest.raises(ValueError, match="mpvae_r_draw = 'philox' draws r_sqrt_sigma from the key"):
        ts.capture_epoch(mpvae_step.DeviceSplit(label.numpy(), feat.numpy()), B_)
    assert ts.graph is None


@pytest.mark.parametrize("world,force", [(2, False), (1, True)])
def test_refused_with_an_active_shard_exchange(monkeypatch, world, force):
    """A process group of two ranks (or of one with mpvae_force_exchange) and
    args.mpvae_shard: the step raises before it draws."""
    monkeypatch.setattr(mpvae_dist.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(mpvae_dist.dist, "get_world_size", lambda group=None: world)
    args = _args(mpvae_r_draw="numpy", mpvae_shard=True, mpvae_force_exchange=force)
    assert mpvae_dist.exchange_active(args)
    ts = _make(args)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="mpvae_shard"):
        ts(*_batches(1)[0])
    assert np.array_equal(np.random.get_state()[1], state)
    assert int(ts.updates) == 0
    # not active: one rank without the rehearsal flag, or no mpvae_shard
    monkeypatch.setattr(mpvae_dist.dist, "get_world_size", lambda group=None: 1)
    assert not mpvae_dist.exchange_active(_args(mpvae_shard=True))
    assert not mpvae_dist.exchange_active(_args(mpvae_shard=False, mpvae_force_exchange=True))


# ----------------------------------------------------------------- regression
@pytest.mark.parametrize("knob", ["absent", None])
def test_without_the_knob_the_step_uses_the_models_r_sqrt_sigma(knob):
    """A 'random' model stepped with mpvae_r_draw absent (or None): the outputs
    are compute_loss's on model.r_sqrt_sigma, numpy's stream is not touched,
    and the step owns no draw buffer."""
    batches = _batches(2)

    def run(hand):
        args = _args() if knob == "absent" or hand else _args(mpvae_r_draw=None)
        ts = _make(args)
        assert ts.r_draw is None and ts.r_drawn is None
        outs = []
        for label, feat in batches:
            if not hand:
                outs.append(ts(label, feat))
                continue
            ts.opt.zero_grad(set_to_none=True)
            res = mpvae.compute_loss(label, *ts.model(label, feat), ts.model.r_sqrt_sigma, args)
            res[0].backward()
            ts._clip()
            ts._gated_update()
            outs.append(res)
        assert ts.model.r_sqrt_sigma.grad is None
        return outs, [p.detach().clone() for p in ts.model.parameters()], np.random.random()

    got, want = run(False), run(True)
    for g, w in zip(got[0], want[0]):
        assert all(same_bits(a, c) for a, c in zip(g, w))
    assert all(same_bits(a, c) for a, c in zip(got[1], want[1]))
    np.random.seed(5)
    b = np.sqrt(6.0 / (L_ + Z_))
    np.random.uniform(-b, b, (L_, Z_))  # the model's own draw, and nothing since
    assert got[2] == want[2] == np.random.random()


def test_binding_declares_the_entry_point():
    import mpvae_hip as H
    assert H.ABI_VERSION >= 19 and "r_uniform" in H.KERNELS
    res, argtypes = H.SIGNATURES["mpv_r_uniform_philox"]
    assert len(argtypes) == 8 and H.R_UNIFORM_THREADS == 256 and H.R_UNIFORM_MAX_BLOCKS >= 1
