"""The backward's dispatch against references, on the GPU: which upstream
gradients are live, the kind of r_sqrt_sigma, which inputs require a gradient,
S-shards, and the forward's walks over several sample tiles.

  * test_live_subsets_match_reference: compute_loss in both GEMM modes against
    the reference's record of 13 objectives (tests/golden/live_l20.npz).
  * test_backward_lattice: at five shapes, each the smallest that selects its
    kernels, 13 upstream subsets x {fp64, fp32 non-zero, frozen fp64}
    r_sqrt_sigma x both GEMM modes against oracle.probit_elbo; every batch has
    10 % soft labels, a row with no positive label and (B >= 4) a row with no
    negative one.
  * test_shards_against_oracle: two S-shards through HipShardBackend, combined
    both ways, forward and backward against the oracle of the whole (dR
    on the live sets that leave it finite, its NaN pattern on the others).
  * test_forward_tile_walks: one workgroup walking several sample tiles
    (plan_fwd's tps > 1) for the 128x128, 256x128 and 256x256 tiles.

Measured on the MI355X (profiles/bwd_lattice_errs.jsonl, recorded by these
tests with MPVAE_RECORD_ERRS set); the bounds are tolerances.py's FWD_RTOL
2e-6 and GRAD_RTOL 5e-5.  Largest errors, forward outputs <= 2.0e-7 everywhere:

  lattice, gradients by shape   L=38 3.3e-6, L=100 2.1e-5, L=200 1.0e-5,
                                L=700 1.5e-5, L=1030 2.0e-5; KL gradients 2.7e-7
  by r_sqrt_sigma kind          fp64 2.1e-5, fp32 2.1e-5, frozen 2.0e-5
  by GEMM mode                  f16x3 2.1e-5, f32 2.1e-5
  by upstream subset            total 1.5e-5, nll 2.0e-5, nll_x 2.1e-5, c 3.2e-7,
                                c_x 3.0e-7, kl 2.4e-7, indiv_prob 4.7e-7,
                                indiv_prob_label 4.9e-7, {nll, c_x} 8.9e-6,
                                {nll_x, c} 2.0e-5, {kl, indiv_prob} 4.7e-7,
                                {nll, nll_x, kl} 2.0e-5, all eight 1.3e-5
  reference record (L=20)       gradients 2.1e-6 in both GEMM modes
  shards                        d fe_out / d fx_out: L=38 2.3e-6, L=200 1.5e-5;
                                finite dR ({nll, nll_x}, indiv_prob*): L=38 1.2e-6,
                                L=200 9.3e-6
  tile walks                    gradients 1.3e-6

The single-output objectives nll / nll_x measure the largest errors, the same
in both GEMM modes; no case comes within a factor of two of GRAD_RTOL.
"""
import argparse

import numpy as np
import pytest
import torch

import mpvae
from golden_io import OUTS
from live_io import (GRADS, KEYS, SCALARS, SUBSETS, LiveFixture, check_live,
                     compute_loss_runner)
from mpvae_ops import HipShardBackend
from oracle import probit_elbo as pe
from test_gpu_parity import _against_oracle
from tolerances import FWD_RTOL, GRAD_RTOL, record, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NLL_COEFF, C_COEFF = 0.5, 10.0
# fixed non-unit upstream gradients of total, nll, nll_x, c, c_x, kl
W = dict(zip(SCALARS, (0.7, 1.3, 0.6, 1.7, 0.9, 1.4)))


@pytest.mark.parametrize("gemm", ["f16x3", "f32"])
def test_live_subsets_match_reference(gemm):
    f = LiveFixture()
    record(f"live_l20_{gemm}",
           {"grad_max": check_live(f, compute_loss_runner(f, DEV, mpvae_gemm=gemm))})


# ------------------------------------------------------------------ lattice
def lattice_inputs(L, z, B, S, d, seed):
    """_against_oracle's recipe (test_gpu_parity.py) with 10 % soft labels, row 1
    without a positive label and, from B = 4, row 2 without a negative one."""
    rng = np.random.default_rng(seed)
    y = (rng.random((B, L)) < 0.25).astype(np.float32)
    y[:, 0], y[:, 1] = 1, 0
    m = rng.random((B, L)) < 0.1
    y[m] = rng.uniform(0.05, 0.95, int(m.sum())).astype(np.float32)
    y[1] = 0.0
    if B >= 4:
        y[2] = 1.0
    f32 = lambda a: a.astype(np.float32)
    inp = dict(y=y, fe_out=f32(rng.standard_normal((B, L))), fx_out=f32(rng.standard_normal((B, L))),
               fe_mu=f32(rng.standard_normal((B, d))), fe_logvar=f32(0.3 * rng.standard_normal((B, d))),
               fx_mu=f32(rng.standard_normal((B, d))), fx_logvar=f32(0.3 * rng.standard_normal((B, d))),
               r_sqrt_sigma=rng.uniform(-1, 1, (L, z)) * np.sqrt(6.0 / (L + z)))
    noise = f32(rng.standard_normal((S, B, z)))
    g_I, g_IL = f32(rng.standard_normal((B, L))), f32(rng.standard_normal((B, L)))
    return inp, noise, g_I, g_IL


def oracle_upstream(obj, g_I, g_IL):
    up = {"g_" + k: W[k] for k in obj if k in W}
    if "indiv_prob" in obj:
        up["g_I"] = g_I
    if "indiv_prob_label" in obj:
        up["g_IL"] = g_IL
    return up


def tag_of(obj):
    return "+".join(obj) if len(obj) < 8 else "all"


LATTICE_SHAPES = [
    # L, z, B, S, d        forward tile; element pass; dR tile
    (38, 38, 4, 37, 8),    # 48x256; bwd_elem RPI 25, bwd_coef's scalar path (S % 4); 64
    (100, 37, 3, 40, 8),   # 128x128; RPI 10, bwd_coef's 16-B path; 128
    (200, 64, 4, 40, 8),   # 256x128; TPR 50, RPI 5; 256 (dR16s)
    (700, 64, 3, 40, 8),   # 256x128; LDS ring with masked waves; 256
    (1030, 96, 3, 24, 8),  # 256x128; LDS ring, two column chunks; 256, 5 x 1 tiles
]
# shapes that also run with a part of the inputs requiring a gradient
NEED_SHAPES = {(100, 37, 3, 40, 8), (700, 64, 3, 40, 8)}
# (total and all eight have an all-NaN dR here: the other two give only-R finite values)
NEED_SUBSETS = [("total",), ("indiv_prob",), ("nll", "nll_x", "kl"), tuple(OUTS)]
ONLY_R = ("r_sqrt_sigma",)
ONLY_FX = ("fx_out", "fx_mu", "fx_logvar")


@pytest.mark.parametrize("gemm", ["f16x3", "f32"])
@pytest.mark.parametrize("rkind", ["r64", "r32", "rfrozen"])
@pytest.mark.parametrize("L,z,B,S,d", LATTICE_SHAPES)
def test_backward_lattice(L, z, B, S, d, rkind, gemm):
    """One case: the oracle's forward once, then every upstream subset (and, at
    NEED_SHAPES, two partial requires_grad sets) through compute_loss.  Per
    subset and gradient: the oracle's NaN pattern; a zero reference met by None
    or exact zeros; FWD_RTOL on the eight outputs, GRAD_RTOL on the gradients
    (the four KL ones included); a frozen r_sqrt_sigma keeps grad None, an fp32
    one gets an fp32 gradient.  Failures are collected over the subsets and
    asserted at the end."""
    inp, noise, g_I, g_IL = lattice_inputs(L, z, B, S, d, L * 7 + S)
    if rkind == "r32":
        inp["r_sqrt_sigma"] = inp["r_sqrt_sigma"].astype(np.float32)
        assert np.abs(inp["r_sqrt_sigma"]).min() > 0
    pos = [inp[k] for k in KEYS]
    fwd = pe.elbo_forward(*pos, inp["r_sqrt_sigma"], noise, NLL_COEFF, C_COEFF)
    ups = {k: torch.tensor(w, dtype=torch.float32, device=DEV) for k, w in W.items()}
    ups["indiv_prob"] = torch.from_numpy(g_I).to(DEV)
    ups["indiv_prob_label"] = torch.from_numpy(g_IL).to(DEV)
    dev_inp = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    noise_t = torch.from_numpy(noise)
    args = argparse.Namespace(label_dim=L, z_dim=z, n_train_sample=S, n_test_sample=S,
                              mode="train", nll_coeff=NLL_COEFF, c_coeff=C_COEFF,
                              mpvae_noise=noise_t, mpvae_gemm=gemm)
    bad, worst = [], {"fwd": 0.0, "grad": 0.0, "grad_kl": 0.0}

    def one(obj, need):
        tag = tag_of(obj) + ("" if len(need) == 7 else "|need=" + ",".join(need))
        t = {k: v.clone() for k, v in dev_inp.items()}
        for k in need:
            t[k].requires_grad_(True)
        out = mpvae.compute_loss(*[t[k] for k in KEYS], t["r_sqrt_sigma"], args)
        for k, o in zip(OUTS, out):
            e = rel_err(o.detach().cpu().double().numpy(), fwd[k])
            worst["fwd"] = max(worst["fwd"], e)
            if e > FWD_RTOL:
                bad.append((tag, k, e))
        sum((out[OUTS.index(k)] * ups[k]).sum() for k in obj).backward()
        rg = pe.elbo_backward(fwd, *pos, noise, NLL_COEFF, C_COEFF,
                              **oracle_upstream(obj, g_I, g_IL))
        for k in GRADS:
            g = t[k].grad
            if k not in need:
                if g is not None:
                    bad.append((tag, k, "a gradient for an input that requires none"))
                continue
            if g is not None and g.dtype != t[k].dtype:
                bad.append((tag, k, str(g.dtype)))
            g = None if g is None else g.cpu().double().numpy()
            if not np.isnan(rg[k]).any() and not rg[k].any():
                if g is not None and (g != 0).any():
                    bad.append((tag, k, "the reference is zero"))
                continue
            if g is None:
                bad.append((tag, k, "None"))
                continue
            if not np.array_equal(np.isnan(g), np.isnan(rg[k])):
                bad.append((tag, k, "NaN pattern"))
                continue
            if not np.isfinite(rg[k]).any():
                continue  # all NaN: the pattern is the whole comparison
            e = rel_err(g, rg[k])
            kind = "grad_kl" if k.endswith(("_mu", "_logvar")) else "grad"
            worst[kind] = max(worst[kind], e)
            worst["grad:" + tag_of(obj)] = max(worst.get("grad:" + tag_of(obj), 0.0), e)
            if e > GRAD_RTOL:
                bad.append((tag, k, e))

    every = tuple(GRADS) if rkind != "rfrozen" else tuple(GRADS[:6])
    for obj in SUBSETS:
        one(obj, every)
    if (L, z, B, S, d) in NEED_SHAPES:
        for obj in NEED_SUBSETS:
            if rkind != "rfrozen":
                one(obj, ONLY_R)
            one(obj, ONLY_FX)
    record(f"lattice_{L}_{z}_{B}_{S}_{rkind}_{gemm}", worst)
    assert not bad, bad


# ------------------------------------------------------------------- shards
# (objective, live mask, whether its d r_sqrt_sigma is finite: every batch has
# degenerate rows, so dR is all NaN as soon as a ranking term is live)
SHARD_LIVE = [(("total",), 0b000001, False), (("c",), 0b001000, False),
              (tuple(OUTS), 0b111111, False), (("nll", "nll_x"), 0b000110, True),
              (("indiv_prob", "indiv_prob_label"), 0b000000, True)]


@pytest.mark.parametrize("gemm", ["f16x3", "f32"])
@pytest.mark.parametrize("L,z,B,S,d", [(38, 38, 4, 37, 8), (200, 64, 4, 40, 8)])
def test_shards_against_oracle(L, z, B, S, d, gemm):
    """Two S-shards (S_local < S_total, s_offset > 0) at the edges of
    pe.elbo_forward(shards=2), on explicit noise: the eight outputs of
    combine_bstats + finalize and of finalize_slots against the oracle, the two
    combined bstat bit for bit, then backward_local per shard with the combined
    bstat, the packed [d fe_out | d fx_out | dR] buffers summed, against
    pe.elbo_backward of the whole: with total, {c} and all eight live, where
    the degenerate rows make dR all NaN (the pattern is what is compared), and
    with {nll, nll_x} and the two indiv_prob gradients alone, where every dR
    entry is finite and held to GRAD_RTOL.  Dead gscal slots hold a value the
    kernels must not read; an entry where the reference has no finite nonzero
    value is compared exactly and not recorded."""
    inp, noise, g_I, g_IL = lattice_inputs(L, z, B, S, d, L * 7 + S + 1)
    pos = [inp[k] for k in KEYS]
    fwd = pe.elbo_forward(*pos, inp["r_sqrt_sigma"], noise, NLL_COEFF, C_COEFF, shards=2)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    mus = [t[k] for k in ("fe_mu", "fe_logvar", "fx_mu", "fx_logvar")]
    noise_t = torch.from_numpy(noise).to(DEV)
    be = HipShardBackend(gemm)
    Rop = be.prepare_R(t["r_sqrt_sigma"])
    parts = []
    for a, b in zip(fwd["_edges"][:-1], fwd["_edges"][1:]):
        a, b = int(a), int(b)
        assert 0 < b - a < S
        shape = be.shape(b - a, S, a, B, L, z)
        eps = be.prepare_noise(noise_t[a:b].contiguous(), shape)
        parts.append((shape, eps, be.forward_local(shape, t["y"], t["fe_out"], t["fx_out"], Rop,
                                                   eps, keep_T=True)))
    shape0 = parts[0][0]
    colsum = parts[0][2]["colsum"] + parts[1][2]["colsum"]
    slots = torch.zeros((2, 6, B), device=DEV, dtype=torch.float32)
    for i, (_, _, loc) in enumerate(parts):
        slots[i] = loc["bstat"]
    bstat = be.combine_bstats(torch.stack([loc["bstat"] for _, _, loc in parts]))
    outs = be.finalize(shape0, bstat, colsum, *mus, NLL_COEFF, C_COEFF)
    bstat2, outs2 = be.finalize_slots(shape0, slots, colsum, *mus, NLL_COEFF, C_COEFF)
    assert torch.equal(bstat, bstat2)
    errs = {}
    for how, oo in (("combine", outs), ("slots", outs2)):
        for k, o in zip(OUTS, oo):
            errs[f"{k}_{how}"] = rel_err(o.cpu().double().numpy(), fwd[k])
    n = B * L
    gI_t, gIL_t = torch.from_numpy(g_I).to(DEV), torch.from_numpy(g_IL).to(DEV)
    for obj, live, finite_dR in SHARD_LIVE:
        gscal = torch.tensor([W[k] if k in obj else 123.0 for k in SCALARS], device=DEV)
        with_ind = "indiv_prob" in obj
        flat = None
        for shape, eps, loc in parts:
            saved = dict(y=t["y"], fe_out=t["fe_out"], fx_out=t["fx_out"], eps=eps,
                         T=loc["T"].clone(), rowstat=loc["rowstat"], bstat=bstat)
            part, _, _ = be.backward_local(shape, saved, gscal, live, gI_t if with_ind else None,
                                           gIL_t if with_ind else None, NLL_COEFF, C_COEFF, True)
            flat = part if flat is None else flat + part
        flat = flat.cpu().double().numpy()
        rg = pe.elbo_backward(fwd, *pos, noise, NLL_COEFF, C_COEFF,
                              **oracle_upstream(obj, g_I, g_IL))
        for k, got in (("fe_out", flat[:n].reshape(B, L)), ("fx_out", flat[n:2 * n].reshape(B, L)),
                       ("r_sqrt_sigma", flat[2 * n:].reshape(L, z))):
            same_nan = np.array_equal(np.isnan(got), np.isnan(rg[k]))
            assert same_nan, (tag_of(obj), k, "NaN pattern")
            fin = np.isfinite(rg[k])
            if k == "r_sqrt_sigma":
                assert bool(fin.all()) == finite_dR and bool(fin.any()) == finite_dR, tag_of(obj)
            if not rg[k][fin].any():  # nothing finite, or an exactly zero reference
                assert not got[fin].any(), (tag_of(obj), k, "the reference is zero")
                continue
            errs[f"d{k}_{tag_of(obj)}"] = rel_err(got, rg[k])
    record(f"shards_{L}_{z}_{B}_{S}_{gemm}", errs)
    for k, e in errs.items():
        assert e <= (GRAD_RTOL if k.startswith("d") else FWD_RTOL), (k, e)


# ---------------------------------------------------------- forward tile walks
def fwd_tiles_per_workgroup(L, B, S, cus):
    """plan_fwd's rule for the 3xf16 tiles (csrc/probit_fwd.hip): s-chunks until
    the grid is one workgroup per CU; tps sample tiles per workgroup."""
    cdiv = lambda a, b: -(-a // b)
    if L <= 48:
        BM, BN = 256, 48
    elif L <= 96:
        BM, BN = 128, 96
    elif L <= 128:
        BM, BN = 128, 128
    else:
        BM, BN = (128, 256) if S < 256 else (256, 256)
    nNt, nSt = cdiv(L, BN), cdiv(S, BM)
    want = min(max(cdiv(cus, B * nNt), 1), nSt)
    return cdiv(nSt, want), S - (nSt - 1) * BM


@pytest.mark.parametrize("L,z,B,S,d,last", [
    (100, 37, 130, 257, 8, 1),    # 128x128 tile: 3 sample tiles, the second s-chunk one sample
    (260, 64, 128, 130, 8, 2),    # 256x128 tile: last tile 2 samples, last label tile 4 labels
    (260, 64, 128, 300, 8, 44),   # 256x256 tile walking into a ragged last tile
])
def test_forward_tile_walks(L, z, B, S, d, last):
    """fwd16_tiles with tps > 1 against the oracle, forward and backward."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tps, tail = fwd_tiles_per_workgroup(L, B, S, cus)
    assert tps >= 2 and tail == last, (tps, tail, cus)
    ferr, gerr = _against_oracle(L, z, B, S, d, "f16x3", NLL_COEFF, C_COEFF, L * 7 + S,
                                 with_gI=True, shards=4)
    record(f"tile_walk_{L}_{z}_{B}_{S}", {**ferr, **{"d" + k: v for k, v in gerr.items()}})
    for k, e in ferr.items():
        assert e <= FWD_RTOL, (k, e)
    for k, e in gerr.items():
        assert e <= GRAD_RTOL, (k, e)
