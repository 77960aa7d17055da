"""predict_proba on the GPU (mpv_probit_predict: the PREDICT instantiations of
the forward tile kernels + predict_final): indiv_prob alone, without labels,
bit for bit compute_loss's at every tile, edge and partial-sum path."""
import argparse
import ctypes
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mpvae
import mpvae_hip as H
import mpvae_ops
from golden_io import fixtures
from oracle import probit_elbo as pe
from tolerances import EXTREME_FWD_RTOL, FWD_RTOL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = fixtures()

# (B, S, L, z): the smallest shapes that walk every tile and edge
SHAPES = [
    (3, 300, 38, 38),     # 48-label tile, two sample tiles, ragged L % 4, z % 32
    (2, 130, 81, 81),     # 96 x 128 tile, second tile of 2 rows
    (2, 129, 101, 50),    # 128 x 128 tile
    (2, 200, 260, 64),    # 256 x 128 tile, second label tile of 4 labels
    (2, 513, 300, 200),   # 256 x 256 tile, three sample tiles
    (4, 1, 38, 38),       # one sample, E published directly
    (1, 2000, 38, 38),    # folded column partials, nSc = 8
    (1, 17920, 8, 8),     # 70 chunks, the slab-sum path
    (4, 10000, 38, 38),   # the evaluation's sample count
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def oracle_indiv(fx_out, R, noise):
    t = pe.noise_product(noise, R)
    return pe.probit_prob(t + np.asarray(fx_out, np.float32)[None]).astype(np.float64).mean(0)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs of one shape (made once, never modified) and the oracle's indiv_prob."""
    B, S, L, z = shape
    g = torch.Generator().manual_seed(B * 1000003 + S * 1009 + L * 31 + z)
    d = 4
    y = (torch.rand(B, L, generator=g) < 0.3).float()
    y[:, 0], y[:, 1] = 1, 0
    mk = lambda *s: torch.randn(*s, generator=g)
    t = dict(y=y, fe_out=mk(B, L), fe_mu=mk(B, d), fe_logvar=0.1 * mk(B, d), fx_out=mk(B, L),
             fx_mu=mk(B, d), fx_logvar=0.1 * mk(B, d),
             r_sqrt_sigma=(torch.rand(L, z, generator=g, dtype=torch.float64) * 2 - 1)
             * float(np.sqrt(6.0 / (L + z))))
    noise = torch.randn(S, B, z, generator=g)
    want = oracle_indiv(t["fx_out"].numpy(), t["r_sqrt_sigma"].numpy(), noise.numpy())
    return {k: v.to(DEV) for k, v in t.items()}, noise.to(DEV), want


def _args(shape, **kw):
    B, S, L, z = shape
    return argparse.Namespace(label_dim=L, z_dim=z, n_train_sample=1, n_test_sample=S, mode="test",
                              nll_coeff=0.5, c_coeff=10.0, **kw)


def _loss_indiv(t, args):
    with torch.no_grad():
        return mpvae.compute_loss(t["y"], t["fe_out"], t["fe_mu"], t["fe_logvar"], t["fx_out"],
                                  t["fx_mu"], t["fx_logvar"], t["r_sqrt_sigma"], args)[6]


@pytest.mark.parametrize("gemm", ["f16x3", "f32"])
@pytest.mark.parametrize("noise", ["explicit", "philox"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bit_equal_to_compute_loss(shape, noise, gemm):
    """The same inputs and noise: compute_loss(...)[6]'s bits, in both GEMM
    modes, with an explicit noise tensor (also against the oracle) and with
    Philox noise from an int seed."""
    t, eps, want = _case(shape)
    kw = dict(mpvae_noise=eps) if noise == "explicit" else dict(mpvae_noise="philox",
                                                               mpvae_seed=4242)
    ref = _loss_indiv(t, _args(shape, mpvae_gemm=gemm, **kw))
    p = mpvae.predict_proba(t["fx_out"], t["r_sqrt_sigma"], _args(shape, mpvae_gemm=gemm, **kw))
    torch.cuda.synchronize()
    assert p.shape == ref.shape and p.dtype == torch.float32 and p.grad_fn is None
    nbad = int((p.view(torch.int32) != ref.view(torch.int32)).sum())
    print(f"{shape} {noise} {gemm}: differing elements {nbad}, "
          f"max |diff| {float((p - ref).abs().max()):.3g}")
    assert torch.equal(p, ref)
    if noise == "explicit":
        e = rel_err(p.cpu().double().numpy(), want)
        print(f"  oracle rel_err {e:.3g}")
        assert e <= FWD_RTOL, e


@pytest.mark.parametrize("f", FIX, ids=[f.name for f in FIX])
def test_golden_fixtures(f):
    t = {k: torch.from_numpy(f[k].copy()).to(DEV) for k in
         ["y", "fe_out", "fe_mu", "fe_logvar", "fx_out", "fx_mu", "fx_logvar", "r_sqrt_sigma"]}
    args = f.args(mpvae_noise=torch.from_numpy(f["noise"]))
    p = mpvae.predict_proba(t["fx_out"], t["r_sqrt_sigma"], args)
    assert torch.equal(p, _loss_indiv(t, args))
    tol = EXTREME_FWD_RTOL if f.extreme else FWD_RTOL
    e_gold = rel_err(p.cpu().double().numpy(), f["out_indiv_prob"])
    e_orc = rel_err(p.cpu().double().numpy(),
                    oracle_indiv(f["fx_out"], f["r_sqrt_sigma"], f["noise"]))
    print(f"{f.name}: golden {e_gold:.3g} oracle {e_orc:.3g} (tol {tol:g})")
    assert e_gold <= tol and e_orc <= tol, (e_gold, e_orc)


def test_no_labels_no_autograd_and_edges():
    shape = SHAPES[0]
    t, eps, _ = _case(shape)
    fx = t["fx_out"].clone().requires_grad_(True)
    R = t["r_sqrt_sigma"].clone().requires_grad_(True)
    p = mpvae.predict_proba(fx, R, _args(shape, mpvae_noise=eps))
    assert p.grad_fn is None and not p.requires_grad
    assert torch.equal(p, mpvae.predict_proba(t["fx_out"], t["r_sqrt_sigma"],
                                              _args(shape, mpvae_noise=eps)))
    e = mpvae.predict_proba(fx[:0], R, _args(shape, mpvae_noise=eps))
    assert e.shape == (0, shape[2]) and e.device == fx.device
    with pytest.raises(IndexError):
        mpvae.predict_proba(fx, R, _args((3, 0, 38, 38)))
    with pytest.raises(RuntimeError):
        mpvae.predict_proba(fx.cpu(), R, _args(shape, mpvae_noise=eps))


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[6], SHAPES[7]],
                         ids=[IDS[0], IDS[4], IDS[6], IDS[7]])
@pytest.mark.parametrize("gemm", ["f16x3", "f32"])
def test_deterministic_and_reads_nothing_stale(shape, gemm):
    """Two calls give the same bits, and so does a call whose workspace and
    output buffers were filled with NaN before the launch."""
    B, S, L, z = shape
    t, eps, _ = _case(shape)
    args = _args(shape, mpvae_noise=eps, mpvae_gemm=gemm)
    a = mpvae.predict_proba(t["fx_out"], t["r_sqrt_sigma"], args)
    b = mpvae.predict_proba(t["fx_out"], t["r_sqrt_sigma"], args)
    cfg = mpvae_ops.ElboConfig(S, S, 0, 0.0, 0.0, noise="explicit",
                               backend=mpvae_ops.HipShardBackend(gemm, poison=True))
    c = mpvae_ops.probit_predict(t["fx_out"], t["r_sqrt_sigma"], eps, cfg)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_device_key_advances_by_one_per_call():
    shape = SHAPES[0]
    t, _, _ = _case(shape)
    seed = torch.tensor([500], dtype=torch.int64, device=DEV)
    args = _args(shape, mpvae_noise="philox", mpvae_seed=seed, mpvae_seed_advance=True)
    seen = []
    for _ in range(3):
        k = int(seed.item())
        p = mpvae.predict_proba(t["fx_out"], t["r_sqrt_sigma"], args)
        assert int(seed.item()) == k + 1
        q = mpvae.predict_proba(t["fx_out"], t["r_sqrt_sigma"],
                                _args(shape, mpvae_noise="philox", mpvae_seed=k))
        assert torch.equal(p, q)
        seen.append(p)
    assert not torch.equal(seen[0], seen[1])


def test_captured_in_a_graph():
    """One torch.cuda.graph capture (Philox noise, device key advanced by the
    call): each of two replays equals the eager call with that replay's key."""
    shape = SHAPES[6]  # nSc = 8: the column partials' workspace comes from the graph pool
    t, _, _ = _case(shape)
    seed = torch.tensor([900], dtype=torch.int64, device=DEV)
    args = _args(shape, mpvae_noise="philox", mpvae_seed=seed, mpvae_seed_advance=True)
    run = lambda: mpvae.predict_proba(t["fx_out"], t["r_sqrt_sigma"], args)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        k = int(seed.item())
        graph.replay()
        torch.cuda.synchronize()
        assert int(seed.item()) == k + 1
        eager = mpvae.predict_proba(t["fx_out"], t["r_sqrt_sigma"],
                                    _args(shape, mpvae_noise="philox", mpvae_seed=k))
        assert torch.equal(out, eager)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        g = torch.Generator(device=DEV).manual_seed(11)
        B, L, z, S = 8, 100, 90, 777  # ragged: 389 + 388
        fx = torch.randn((B, L), device=DEV, generator=g)
        R = (torch.rand((L, z), device=DEV, generator=g, dtype=torch.float64) * 2 - 1) * 0.1
        base = dict(label_dim=L, z_dim=z, n_train_sample=S, n_test_sample=S, mode="test",
                    mpvae_noise="philox")
        whole = mpvae.predict_proba(fx, R, argparse.Namespace(**base, mpvae_seed=1000))
        part = mpvae.predict_proba(fx, R, argparse.Namespace(  # rank 0's seed must win
            **base, mpvae_seed=1000 + 17 * rank, mpvae_shard=True, mpvae_check_replicas=True))
        torch.cuda.synchronize()
        q.put((rank, rel_err(part.cpu().double().numpy(), whole.cpu().double().numpy())))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_unsharded():
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=150) for _ in procs]
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    assert sorted(r for r, _ in res) == list(range(world))
    for rank, err in res:
        assert err <= FWD_RTOL, (rank, err)


def test_abi_rejects_bad_arguments_before_any_launch():
    lib = H.load_library()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks
    assert lib.mpv_predict_workspace_bytes(H.Shape(0, 10, 0, 4, 8, 8)) == 0
    assert lib.mpv_probit_predict(H.Shape(0, 10, 0, 4, 8, 8), H.PredictArgs(), None) == 1
    ok = H.Shape(2000, 2000, 0, 1, 38, 38)  # nSc = 8: needs a workspace
    need = lib.mpv_predict_workspace_bytes(ok)
    assert need >= 8 * 38 * 4
    assert need < lib.mpv_fwd_workspace_bytes(ok)  # the column partials only
    a = H.PredictArgs(None, H.GEMM_F32, fake, fake, H.Split16(), H.Split16(), fake, fake, None,
                      fake, need)
    assert lib.mpv_probit_predict(ok, a, None) == 1
    assert b"NULL" in lib.mpv_last_error()
    a = H.PredictArgs(fake, H.GEMM_F32, fake, fake, H.Split16(), H.Split16(), fake, fake, None,
                      fake, need - 1)
    assert lib.mpv_probit_predict(ok, a, None) == 1
    assert b"workspace" in lib.mpv_last_error()
    a = H.PredictArgs(fake, H.GEMM_F32, None, fake, H.Split16(), H.Split16(), fake, fake, None,
                      fake, need)
    assert lib.mpv_probit_predict(ok, a, None) == 1
    short = H.Split16(fake, fake, 1, 64)       # one row: fewer than the tile's
    full = H.Split16(fake, fake, 1 << 20, 128)
    for R16, e16, what in ((short, full, b"R16"), (full, short, b"eps16"),
                           (H.Split16(fake, fake, 1 << 20, 32), full, b"ld")):
        a = H.PredictArgs(fake, H.GEMM_F16X3, None, None, R16, e16, fake, fake, None, fake, need)
        assert lib.mpv_probit_predict(ok, a, None) == 1
        assert what in lib.mpv_last_error(), lib.mpv_last_error()
    a = H.PredictArgs(fake, 7, fake, fake, H.Split16(), H.Split16(), fake, fake, None, fake, need)
    assert lib.mpv_probit_predict(ok, a, None) == 1
    torch.cuda.synchronize()  # nothing was launched: no fault is pending
