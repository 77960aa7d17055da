"""predict_proba on CPU tensors (libmpvae_host.so's mpvh_probit_predict):
indiv_prob alone, without labels, bit for bit the host compute_loss's."""
import argparse
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mpvae
from golden_io import fixtures
from oracle import probit_elbo as pe
from tolerances import EXTREME_FWD_RTOL, FWD_RTOL, rel_err

FIX = fixtures()


def oracle_indiv(fx_out, R, noise):
    """mean_s E_x in fp64 from the oracle's fp32 E (oracle/probit_elbo.py)."""
    t = pe.noise_product(noise, R)
    return pe.probit_prob(t + np.asarray(fx_out, np.float32)[None]).astype(np.float64).mean(0)


def _loss_indiv(f, args):
    t = {k: torch.from_numpy(f[k].copy()) for k in
         ["y", "fe_out", "fe_mu", "fe_logvar", "fx_out", "fx_mu", "fx_logvar", "r_sqrt_sigma"]}
    with torch.no_grad():
        return mpvae.compute_loss(t["y"], t["fe_out"], t["fe_mu"], t["fe_logvar"], t["fx_out"],
                                  t["fx_mu"], t["fx_logvar"], t["r_sqrt_sigma"], args)[6]


@pytest.mark.parametrize("f", FIX, ids=[f.name for f in FIX])
def test_golden_fixtures(f):
    """Every golden fixture: the host compute_loss's indiv_prob bit for bit, the
    reference's recorded one and the numpy oracle's within the forward tolerance."""
    args = f.args(mpvae_noise=torch.from_numpy(f["noise"]))
    fx, R = torch.from_numpy(f["fx_out"].copy()), torch.from_numpy(f["r_sqrt_sigma"].copy())
    p = mpvae.predict_proba(fx, R, args)
    assert p.device.type == "cpu" and p.dtype == torch.float32 and p.shape == (f.B, f.L)
    assert torch.equal(p, _loss_indiv(f, args))
    tol = EXTREME_FWD_RTOL if f.extreme else FWD_RTOL
    e_gold = rel_err(p.double().numpy(), f["out_indiv_prob"])
    e_orc = rel_err(p.double().numpy(), oracle_indiv(f["fx_out"], f["r_sqrt_sigma"], f["noise"]))
    print(f"{f.name}: golden {e_gold:.3g} oracle {e_orc:.3g} (tol {tol:g})")
    assert e_gold <= tol and e_orc <= tol, (e_gold, e_orc)


def test_torch_cpu_noise_consumes_the_same_draw():
    """The default noise: predict_proba and compute_loss draw the same normals
    and leave torch's CPU generator in the same state."""
    f = next(f for f in FIX if f.name == "f1_l38")
    fx, R = torch.from_numpy(f["fx_out"].copy()), torch.from_numpy(f["r_sqrt_sigma"].copy())
    for k in (0, 7):
        torch.manual_seed(k)
        ref = _loss_indiv(f, f.args())
        state_loss = torch.get_rng_state()
        torch.manual_seed(k)
        p = mpvae.predict_proba(fx, R, f.args())
        assert torch.equal(torch.get_rng_state(), state_loss)
        assert torch.equal(p, ref)


def test_no_labels_and_no_autograd():
    """Nothing of shape (B, L) but fx_out goes in, and nothing differentiable comes out."""
    g = torch.Generator().manual_seed(5)
    B, L, z, S = 3, 7, 5, 9
    fx = torch.randn(B, L, generator=g, requires_grad=True)
    R = torch.randn(L, z, generator=g, dtype=torch.float64, requires_grad=True)
    args = argparse.Namespace(mode="test", n_train_sample=1, n_test_sample=S, z_dim=z,
                              mpvae_noise=torch.randn(S, B, z, generator=g))
    assert torch.is_grad_enabled()
    p = mpvae.predict_proba(fx, R, args)
    assert p.shape == (B, L) and p.grad_fn is None and not p.requires_grad
    assert bool(((p > 0) & (p < 1)).all())
    want = oracle_indiv(fx.detach().numpy(), R.detach().numpy(), args.mpvae_noise.numpy())
    assert rel_err(p.double().numpy(), want) <= FWD_RTOL
    assert "predict_proba" in mpvae.__all__


def test_edge_arguments():
    args = argparse.Namespace(mode="test", n_train_sample=4, n_test_sample=4, z_dim=5)
    R = torch.zeros(7, 5, dtype=torch.float64)
    p = mpvae.predict_proba(torch.zeros(0, 7), R, args)
    assert p.shape == (0, 7) and p.dtype == torch.float32
    args.n_test_sample = 0
    with pytest.raises(IndexError, match="sample axis is empty"):
        mpvae.predict_proba(torch.zeros(2, 7), R, args)
    args.n_test_sample = 4
    with pytest.raises(ValueError, match=r"r_sqrt_sigma must be \(label_dim, z_dim=5\)"):
        mpvae.predict_proba(torch.zeros(2, 7), torch.zeros(7, 6), args)
    with pytest.raises(ValueError, match=r"r_sqrt_sigma must be \(label_dim=7, z_dim\)"):
        mpvae.predict_proba(torch.zeros(2, 7), torch.zeros(8, 5), args)
    args.mpvae_noise = torch.zeros(4, 2, 6)
    with pytest.raises(ValueError, match="args.mpvae_noise must be"):
        mpvae.predict_proba(torch.zeros(2, 7), R, args)
    with pytest.raises(RuntimeError):  # CPU and device tensors mixed: never a fallback
        mpvae.predict_proba(torch.zeros(2, 7), torch.zeros(7, 5, device="meta"), args)


def test_closed_form_expectation():
    """Independent of the library's code: for t ~ N(0, |R_l|^2),
    E_t[Phi(m + t)] = Phi(m / sqrt(1 + |R_l|^2)).  E = Phi (1 - 1e-6) + 0.5e-6 moves
    a value by at most 0.5e-6; the mean of S samples of E, whose standard
    deviation is at most 0.5, lies within 5 sigma = 5 * 0.5 / sqrt(S) of it."""
    B, L, z, S = 4, 38, 38, 10000
    g = torch.Generator().manual_seed(2024)
    fx = torch.randn(B, L, generator=g)
    R = torch.randn(L, z, generator=g, dtype=torch.float64) * 0.2
    args = argparse.Namespace(mode="test", n_train_sample=1, n_test_sample=S, z_dim=z,
                              mpvae_noise=torch.randn(S, B, z, generator=g))
    p = mpvae.predict_proba(fx, R, args).double()
    m = fx.double() / torch.sqrt(1.0 + (R.float().double() ** 2).sum(1))[None]
    want = 0.5 * (1.0 + torch.erf(m / math.sqrt(2.0)))
    err = float((p - want).abs().max())
    bound = 5 * 0.5 / math.sqrt(S)
    print(f"closed form: max |indiv_prob - Phi| = {err:.4g}, bound {bound:.4g}")
    assert err <= bound


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_worker(rank, world, port, names, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = []
        for f in [f for f in fixtures() if f.name in names]:
            fx = torch.from_numpy(f["fx_out"].copy())
            R = torch.from_numpy(f["r_sqrt_sigma"].copy())
            noise = torch.from_numpy(f["noise"])
            whole = mpvae.predict_proba(fx, R, f.args(mpvae_noise=noise))
            part = mpvae.predict_proba(fx, R, f.args(mpvae_noise=noise, mpvae_shard=True,
                                                     mpvae_check_replicas=True))
            res.append((f.name, rel_err(part.double().numpy(), whole.double().numpy()),
                        part.grad_fn is None))
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_matches_unsharded(world):
    """Each rank predicts its slice of the sample axis; one all_reduce of the
    (B, L) column sums, then the division."""
    names = ["f1_l38", "f3_adult_like"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, names, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, res in results:
        assert len(res) == len(names)
        for name, err, nograd in res:
            assert err <= FWD_RTOL and nograd, (rank, name, err)
