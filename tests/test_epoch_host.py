"""CPU: ``mpvae_step.DeviceSplit`` on CPU tensors (torch indexing with
mpv_gather_batch's semantics), the epoch batch rule, the host range check of a
numpy order, and ``TrainStep.run_epoch`` against the hand-fed loop."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import mpvae
import mpvae_hip as H
import mpvae_step
from guarded_alloc import same_bits

DTYPES = [np.float32, np.float64, np.int32, np.int64, np.uint8]


def _data(n, L=6, F=5, n_sens=2, label_dtype=np.uint8, feat_dtype=np.float64,
          sens_dtype=np.int64, seed=0):
    rng = np.random.default_rng(seed)
    labels = (rng.random((n, L)) < 0.4).astype(label_dtype)
    feats = rng.standard_normal((n, F)).astype(feat_dtype)
    sens = rng.integers(0, 3, (n, n_sens)).astype(sens_dtype)
    return labels, feats, sens


def test_binding_knows_the_gather_entry():
    assert "mpv_gather_batch" in H.SIGNATURES and "gather_batch" in H.KERNELS
    assert H.EL_U8 == 4 and H.ABI_VERSION >= 18
    # mpv_gather_args: 4 x (8 + 4 + 8 + 8 + 4) B of per-source fields, then n_sources and
    # advance (4 B each, padded to 8) and seven 8-B fields
    assert ctypes.sizeof(H.GatherArgs) == 4 * 32 + 2 * 8 + 7 * 8


@pytest.mark.parametrize("sens_dtype", DTYPES)
@pytest.mark.parametrize("label_dtype", DTYPES)
def test_gather_returns_what_float_of_the_host_gather_gives(label_dtype, sens_dtype):
    labels, feats, sens = _data(11, label_dtype=label_dtype, sens_dtype=sens_dtype)
    split = mpvae_step.DeviceSplit(labels, feats, sens)
    assert split.labels.dtype == torch.from_numpy(labels).dtype  # kept, not cast
    assert split.sens.dtype == torch.from_numpy(sens).dtype
    order = np.array([3, 3, 10, 0, 7, 1, 1, 9])
    for start, B in ((0, 8), (2, 5), (7, 1)):
        y, x, s = split.gather(order, start, B)
        idx = order[start:start + B]
        assert same_bits(y, torch.from_numpy(labels[idx]).float())
        assert same_bits(x, torch.from_numpy(feats[idx]).float())
        assert same_bits(s, torch.from_numpy(sens[idx]))
    # the identity order, a tensor order, a tensor start, and out=
    y, x, s = split.gather(None, 4, 3)
    assert same_bits(x, torch.from_numpy(feats[4:7]).float())
    out = split.gather(torch.from_numpy(order), torch.tensor(2), 4)
    again = split.gather(torch.from_numpy(order), 2, 4, out=out)
    assert all(a is b for a, b in zip(out, again))
    assert same_bits(out[0], torch.from_numpy(labels[order[2:6]]).float())
    split.check()
    assert int(split.bad) == 0


def test_split_without_sensitive_features_and_rejected_inputs():
    labels, feats, _ = _data(5)
    split = mpvae_step.DeviceSplit(torch.from_numpy(labels), torch.from_numpy(feats))
    y, x, s = split.gather(None, 0, 5)
    assert s is None and y.dtype == x.dtype == torch.float32
    with pytest.raises(ValueError, match="fp32, fp64, int32, int64 or uint8"):
        mpvae_step.DeviceSplit(labels.astype(bool), feats)
    with pytest.raises(ValueError, match="same number"):
        mpvae_step.DeviceSplit(labels[:4], feats)
    with pytest.raises(ValueError, match="2-D"):
        mpvae_step.DeviceSplit(labels[:, 0], feats)
    with pytest.raises(ValueError, match="at least one row"):
        split.gather(None, 0, 0)
    with pytest.raises(ValueError, match="no sensitive_feat"):
        split.next_batch(2, sens=True)


@pytest.mark.parametrize("sens_dtype", [np.int64, np.float64, np.uint8])
def test_out_of_range_rows_are_nan_or_zero_and_flagged(sens_dtype):
    labels, feats, sens = _data(7, sens_dtype=sens_dtype)
    split = mpvae_step.DeviceSplit(labels, feats, sens)
    order = torch.tensor([2, -1, 5, 7, 0, 6])  # a tensor: not checked on the host
    y, x, s = split.gather(order, 1, 7)          # rows 5 and 6 of the batch: past the order
    bad = [0, 2, 5, 6]
    good = [1, 3, 4]
    src = order[1:6][good].numpy()
    assert same_bits(y[good], torch.from_numpy(labels[src]).float())
    assert same_bits(x[good], torch.from_numpy(feats[src]).float())
    assert same_bits(s[good], torch.from_numpy(sens[src]))
    assert torch.isnan(y[bad]).all() and torch.isnan(x[bad]).all()
    if s.dtype.is_floating_point:
        assert torch.isnan(s[bad]).all()
    else:
        assert (s[bad] == 0).all()
    assert int(split.bad) == 1
    with pytest.raises(IndexError, match="out-of-range index"):
        split.check()
    split.check()  # the flag was cleared
    # a negative start
    y, _, _ = split.gather(None, -2, 4)
    assert torch.isnan(y[:2]).all() and not torch.isnan(y[2:]).any()
    with pytest.raises(IndexError):
        split.check()


def test_numpy_order_is_range_checked_on_the_host():
    labels, feats, sens = _data(7)
    split = mpvae_step.DeviceSplit(labels, feats, sens)
    for order in (np.array([0, 7]), np.array([-1, 2])):
        with pytest.raises(IndexError, match=r"outside \[0, 7\)"):
            split.gather(order, 0, 2)
        with pytest.raises(IndexError, match=r"outside \[0, 7\)"):
            split.set_order(order)
    with pytest.raises(ValueError, match="integer"):
        split.set_order(np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="at most"):
        split.set_order(np.zeros(8, np.int64))
    assert int(split.bad) == 0
    assert split.set_order(np.array([4, 2, 6], np.int32)) == 3
    assert split.order.tolist() == [4, 2, 6, -1, -1, -1, -1] and int(split.cursor) == 0
    assert split.set_order(None) == 7 and split.order.tolist() == list(range(7))


@pytest.mark.parametrize("n,B,want", [(43, 8, (5, 3)), (40, 8, (5, 0)), (3, 8, (0, 3)),
                                      (8, 8, (1, 0)), (0, 8, (0, 0)), (9, 1, (9, 0))])
def test_epoch_batches_are_the_reference_loops(n, B, want):
    """fairsoft_train.py:48-56: ``for i in range(N // B + 1)`` over ``[i B,
    min((i + 1) B, N))``; the empty last batch draws nothing."""
    sizes = [min((i + 1) * B, n) - i * B for i in range(n // B + 1)]
    sizes = [s for s in sizes if s > 0]
    full, tail = mpvae_step.epoch_batches(n, B)
    assert (full, tail) == want
    assert [B] * full + ([tail] if tail else []) == sizes
    with pytest.raises(ValueError):
        mpvae_step.epoch_batches(n, 0)


def test_cursor_walks_the_order():
    labels, feats, sens = _data(9)
    split = mpvae_step.DeviceSplit(labels, feats, sens)
    order = np.array([8, 1, 6, 3, 4, 5, 2])
    split.set_order(order)
    for i in range(3):
        y, _, s = split.next_batch(2)
        assert int(split.cursor) == 2 * (i + 1)
        assert same_bits(s, torch.from_numpy(sens[order[2 * i:2 * i + 2]]))
    y, x, none = split.next_batch(1, advance=False, sens=False)
    assert none is None and int(split.cursor) == 6
    assert same_bits(x, torch.from_numpy(feats[order[6:7]]).float())
    split.check()
    split.next_batch(2, advance=False)  # one row past the order: the buffer holds -1 there
    with pytest.raises(IndexError):
        split.check()


# ------------------------------------------------------------- run_epoch
def _args():
    return argparse.Namespace(feature_dim=12, latent_dim=8, label_dim=6, z_dim=4, keep_prob=0.5,
                              scale_coeff=1.0, residue_sigma="", n_train_sample=10,
                              n_test_sample=10, mode="train", nll_coeff=0.5, c_coeff=10.0)


@pytest.mark.parametrize("n,steps", [(8 * 5 + 3, 6), (8 * 5, 5), (3, 1)])
def test_run_epoch_equals_the_hand_fed_loop_on_the_cpu(n, steps):
    """Two epochs of TrainStep on CPU tensors (the host backend), one fed by
    run_epoch from a DeviceSplit, one by the reference's per-batch
    ``from_numpy(data[idx]).float()``: the same RNG stream, so the parameters,
    the Adam state and ``updates`` are equal bit for bit."""
    B, args = 8, _args()
    labels, feats, _ = _data(n, L=6, F=12, seed=n)
    labels[:, 0], labels[:, 1] = 1, 0
    rng = np.random.default_rng(1)
    orders = [rng.permutation(n), rng.permutation(n)]

    def run(epoch_fed):
        torch.manual_seed(0)
        np.random.seed(0)
        model = mpvae.VAE(args).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5, fused=True)
        ts = mpvae_step.TrainStep(model, opt, args)
        split = mpvae_step.DeviceSplit(labels, feats)
        torch.manual_seed(1)
        count = 0
        for order in orders:
            if epoch_fed:
                count += ts.run_epoch(split, order, B)
                assert int(split.cursor) == n - n % B
                continue
            for i in range(n // B + 1):
                idx = order[i * B:min((i + 1) * B, n)]
                if len(idx):
                    ts(torch.from_numpy(labels[idx]).float(), torch.from_numpy(feats[idx]).float())
                    count += 1
        split.check()
        state = [s for p in model.parameters() for s in opt.state[p].values()]
        return count, list(model.state_dict().values()) + state, int(ts.updates)

    got, want = run(True), run(False)
    assert got[0] == want[0] == 2 * steps and got[2] == want[2] == 2 * steps
    assert len(got[1]) == len(want[1]) and all(same_bits(a, b) for a, b in zip(got[1], want[1]))
