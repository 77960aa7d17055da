"""The kernels that walk the batch axis B and the latent axis d, at the sizes
where their loops take a second pass or another path, against fp64 references
(tests/batch_axis_cases.py: cases, references, elementwise metrics in
u = 2^-24, and the rule that a device value may sit at most 4 x max(the torch
CPU fp32 evaluation's own error, 1 u) from fp64).  L = 3, z = 2, S = 2, explicit
noise, both GEMM modes wherever a case runs the forward; every batch has
y[:, 0] = 1, y[:, 1] = 0 and a last row with logits of four times the scale.

Which case reaches which path (batch_axis_cases.paths(): arithmetic on
kFinalThreads = 1024, kCoefThreads = 512, bwd_coef's 256 KL workgroups and
mpv_kl_bwd's 4096 x 256 threads; tests/test_batch_axis_host.py holds those
constants to the source and the cases to their paths, without a GPU):

  finalize_scalars, b loop, 2nd pass      (1025, 4), (1025, 129), (1028, 128);
                                          three passes (2049, 1); the combine
                                          rows of finalize_shards at B = 1025
  finalize_scalars, 16-B KL loop          (1025, 4) two passes, (1028, 128) 33
  finalize_scalars, scalar KL loop        B d % 4 != 0: (1025, 129), (2049, 1),
                                          (513, 257); misaligned pointers:
                                          test_misaligned_mu_logvar (1028, 128)
  bwd_coef's fused KL, stride loop        B d > 131 072: (1025, 129), (1028, 128),
                                          (513, 257) (B < 1024)
  kl_bwd_kernel (only mu / logvar need    test_standalone_kl_bwd; its stride
  a gradient)                             loop B d > 1 048 576: (1025, 1024)
  kl_bwd_range / klt, exp large, tiny,    profile "wide" at (1025, 129) and
  against the 1e-6                        (1025, 1024); "overflow" (inf pattern)
  bstat_combine_kernel, finalize_shards   test_bstat_combine: B = 1, 255, 257,
                                          1025 x R = 1, 2, 8 x maxima near / 200
                                          apart / tied
  reparam_fwd_kernel, reparam_bwd_kernel  test_reparam: n_e != n_x, a block
                                          across both encoders, n_e = 0, n_x = 0,
                                          gz NULL per encoder, every mix of the
                                          four *_add_* pointers, SingleReparam,
                                          wide and overflowing logvar

Measured on the MI355X (profiles/batch_axis_errs.jsonl, recorded by these tests
with MPVAE_RECORD_ERRS set), largest figures in u, the torch-fp32 evaluation's
own figure on the same inputs in brackets:

  KL gradients, fused (a)        g_*_mu 4.9 (4.5), g_fe_logvar 1.6 (1.6),
                                 g_fx_logvar 6.0 (6.0)
  KL gradients, standalone (b)   g_*_mu 5.4 (5.3), g_fe_logvar 2.5 (2.5),
                                 g_fx_logvar 6.4 (6.4); wide no worse than tame
  misaligned (c)                 g_*_mu 4.9 (4.4), g_fx_logvar 5.8 (5.8)
  KL scalar                      1.05 (0.88)
  combined Z (d)                 near 2.6 (3.0), tied 3.1 (3.3), 200 apart 0 (0);
                                 ranking sums 2.9 at R = 8 (bound R)
  reparam (e)                    z 2.0 (2.5), gmu 1.0 (1.0), glv 2.75 (2.75)
  forward outputs 3.3e-7 (FWD_RTOL 2e-6); d fe_out / d fx_out / dR 6.1e-7
  (GRAD_RTOL 5e-5)

Every inf / NaN pattern of the overflow profile equals torch fp32's.  Wrong
builds these tests were seen to fail on: finalize's b loop stopped after one
pass (every case with B > 1024 of a-d); bwd_coef's KL stride one block too
long (the fused cases with B d > 131 072 of a, b's bit comparison, c);
reparam's x branch indexed by i (restated on the CPU, as the build itself
indexes out of bounds: every shape with both encoders non-empty).
"""
import argparse
import itertools

import numpy as np
import pytest
import torch

import batch_axis_cases as bc
import mpvae
from golden_io import OUTS
from live_io import GRADS
from mpvae_ops import FusedReparam, HipShardBackend, SingleReparam
from oracle import probit_elbo as pe
from tolerances import FWD_RTOL, GRAD_RTOL, record, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEMMS = ["f16x3", "f32"]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _dev_inputs(inp, misalign=False):
    """The case's tensors on the device; misalign: each mu / logvar a contiguous
    view at storage offset 1 of a larger buffer (4 bytes past a 16-B boundary)."""
    t = {}
    for k in bc.KEYS + ["r_sqrt_sigma"]:
        a = torch.from_numpy(np.array(inp[k]))
        if misalign and k in bc.MU_KEYS:
            buf = torch.empty(a.numel() + 4, dtype=torch.float32, device=DEV)
            v = buf[1:1 + a.numel()].view(a.shape)
            v.copy_(a)
            assert v.is_contiguous() and v.storage_offset() == 1 and v.data_ptr() % 16 == 4
            t[k] = v
        else:
            t[k] = a.to(DEV)
            assert t[k].data_ptr() % 16 == 0
    return t


def _run(inp, need, gemm, objective, misalign=False):
    """compute_loss + backward of the objective; (outputs, gradients) as numpy."""
    t = _dev_inputs(inp, misalign)
    for k in need:
        t[k].requires_grad_(True)
    args = argparse.Namespace(label_dim=bc.L, z_dim=bc.Z, n_train_sample=bc.S, n_test_sample=bc.S,
                              mode="train", nll_coeff=bc.NLL_COEFF, c_coeff=bc.C_COEFF,
                              mpvae_noise=torch.from_numpy(np.array(inp["noise"])),
                              mpvae_gemm=gemm)
    out = mpvae.compute_loss(*[t[k] for k in bc.KEYS], t["r_sqrt_sigma"], args)
    sum(out[OUTS.index(k[2:])] * w for k, w in bc.OBJECTIVES[objective].items()).backward()
    outs = {k: o.detach().cpu().numpy() for k, o in zip(OUTS, out)}
    grads = {k: None if t[k].grad is None else t[k].grad.cpu().numpy() for k in GRADS}
    # what goes back to the caching allocator holds NaN: a later call that skips
    # an element cannot find this call's value for it in its fresh buffer
    for x in list(out) + [t[k].grad for k in GRADS if t[k].grad is not None]:
        x.detach().fill_(float("nan"))
    return outs, grads


def _forward_errs(outs, B, d, profile, inp):
    """FWD_RTOL figures of the eight outputs (kl and total left to the inf
    check of kl_scalar_errs where fp32 overflows) and the KL scalar's own."""
    ref = bc.elbo_ref(B, d, profile)
    errs = bc.kl_scalar_errs(float(outs["kl"]), inp)
    for k in OUTS:
        if profile == "overflow" and k in ("kl", "total"):
            assert np.isposinf(outs[k]), k
            continue
        errs["out_" + k] = rel_err(outs[k].astype(np.float64), ref[k])
    return errs


def _assert_forward(errs):
    for k, e in errs.items():
        if k.startswith("out_"):
            assert e <= FWD_RTOL, (k, e)


# --------------------------------------------------- a. whole compute_loss
A_CASES = [(1025, 4, "tame"), (1025, 129, "tame"), (1025, 129, "wide"), (1028, 128, "tame"),
           (2049, 1, "tame"), (513, 257, "tame")]


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("B,d,profile", A_CASES)
def test_compute_loss_batch_axis(B, d, profile, gemm):
    """Every input requires a gradient (the KL backward rides on bwd_coef);
    objective 0.75 total.  Outputs FWD_RTOL, d fe_out / d fx_out / dR GRAD_RTOL,
    the KL scalar and the four mu / logvar gradients by the elementwise rule."""
    inp = bc.elbo_case(B, d, profile)
    outs, grads = _run(inp, GRADS, gemm, "total")
    errs = _forward_errs(outs, B, d, profile, inp)
    rg = bc.elbo_ref_grads(B, d, profile, "total")
    for k in ("fe_out", "fx_out", "r_sqrt_sigma"):
        errs["d" + k] = rel_err(grads[k].astype(np.float64), rg[k])
    errs.update(bc.kl_grad_errs({k: grads[k] for k in bc.MU_KEYS}, inp,
                                **bc.OBJECTIVES["total"]))
    record(f"loss_{B}_{d}_{profile}_{gemm}", errs)
    _assert_forward(errs)
    for k in ("fe_out", "fx_out", "r_sqrt_sigma"):
        assert errs["d" + k] <= GRAD_RTOL, (k, errs["d" + k])
    assert not bc.within_ref_rule(errs), (bc.within_ref_rule(errs), errs)


# ------------------------------------------------ b. the standalone KL backward
B_CASES = [(1025, 129, "tame"), (1025, 129, "wide"), (1025, 129, "overflow"),
           (1025, 1024, "tame"), (1025, 1024, "wide")]


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("objective", sorted(bc.OBJECTIVES))
@pytest.mark.parametrize("B,d,profile", B_CASES)
def test_standalone_kl_bwd(B, d, profile, objective, gemm):
    """Only the four mu / logvar tensors require a gradient: mpv_kl_bwd's own
    launch.  Against fp64 by the elementwise rule; at (1025, 129) bit for bit
    the gradients of the fused path (every input requiring a gradient), since
    both run kl_bwd_range."""
    inp = bc.elbo_case(B, d, profile)
    outs, grads = _run(inp, bc.MU_KEYS, gemm, objective)
    for k in ("fe_out", "fx_out", "r_sqrt_sigma"):
        assert grads[k] is None, k
    errs = _forward_errs(outs, B, d, profile, inp)
    errs.update(bc.kl_grad_errs({k: grads[k] for k in bc.MU_KEYS}, inp,
                                **bc.OBJECTIVES[objective]))
    record(f"klbwd_{B}_{d}_{profile}_{objective}_{gemm}", errs)
    _assert_forward(errs)
    assert not bc.within_ref_rule(errs), (bc.within_ref_rule(errs), errs)
    if profile == "overflow":
        assert np.isinf(grads["fe_logvar"]).sum() == 5 and np.isinf(grads["fx_logvar"]).sum() == 5
    if (B, d) == (1025, 129):
        _, fused = _run(inp, GRADS, gemm, objective)
        for k in bc.MU_KEYS:
            assert np.array_equal(_bits(grads[k]), _bits(fused[k])), (k, "fused != standalone")


# ------------------------------------------------------ c. misaligned mu / logvar
@pytest.mark.parametrize("gemm", GEMMS)
def test_misaligned_mu_logvar(gemm):
    """(1028, 128): B d % 4 == 0, so only the pointers' alignment sends
    finalize to its scalar KL loop.  Against the oracle; every output but kl
    and total (another summation order) and the KL gradients bit-equal to the
    aligned run."""
    B, d, profile = 1028, 128, "tame"
    inp = bc.elbo_case(B, d, profile)
    a_outs, a_grads = _run(inp, GRADS, gemm, "total")
    outs, grads = _run(inp, GRADS, gemm, "total", misalign=True)
    errs = _forward_errs(outs, B, d, profile, inp)
    rg = bc.elbo_ref_grads(B, d, profile, "total")
    for k in ("fe_out", "fx_out", "r_sqrt_sigma"):
        errs["d" + k] = rel_err(grads[k].astype(np.float64), rg[k])
    errs.update(bc.kl_grad_errs({k: grads[k] for k in bc.MU_KEYS}, inp,
                                **bc.OBJECTIVES["total"]))
    record(f"misaligned_{B}_{d}_{gemm}", errs)
    _assert_forward(errs)
    for k in ("fe_out", "fx_out", "r_sqrt_sigma"):
        assert errs["d" + k] <= GRAD_RTOL, (k, errs["d" + k])
    assert not bc.within_ref_rule(errs), (bc.within_ref_rule(errs), errs)
    for k in OUTS:
        if k not in ("kl", "total"):
            assert np.array_equal(_bits(outs[k]), _bits(a_outs[k])), k
    for k in bc.MU_KEYS:
        assert np.array_equal(_bits(grads[k]), _bits(a_grads[k])), k


# ------------------------------------------------------- d. cross-shard combine
@pytest.mark.parametrize("kind", bc.BSTAT_KINDS)
@pytest.mark.parametrize("B", bc.BSTAT_B)
@pytest.mark.parametrize("R", bc.BSTAT_R)
def test_bstat_combine(R, B, kind):
    """HipShardBackend.combine_bstats against oracle.probit_elbo.combine_bstats
    in fp64: M exact, Z by the reference-fp32 rule, the sums within R u of
    sum |terms|.  At B = 1025 finalize_slots on the same buffer returns that
    bstat bit for bit and the outputs of finalize(combine_bstats(...)) bit for
    bit, the four loss terms within FWD_RTOL of the oracle's finalize."""
    g = bc.bstat_case(R, B, kind)
    gt = torch.from_numpy(g).to(DEV)
    be = HipShardBackend()
    comb = be.combine_bstats(gt)
    got = comb.cpu().numpy()
    errs = bc.bstat_errs(got, g)
    if kind == "far" and R > 1:   # every shard below the maximum vanishes: Z is the top one's
        top = g[:, 0].argmax(0)
        assert np.array_equal(got[1], g[top, 1, np.arange(B)])
    if B == 1025:
        colsum, mus = bc.finalize_inputs(B)
        colsum_t = torch.from_numpy(colsum).to(DEV)
        mus_t = [torch.from_numpy(mus[k]).to(DEV) for k in bc.MU_KEYS]
        shape = be.shape(bc.S, bc.S * R, 0, B, bc.L, bc.Z)
        bstat2, outs2 = be.finalize_slots(shape, gt, colsum_t, *mus_t, bc.NLL_COEFF, bc.C_COEFF)
        outs1 = be.finalize(shape, comb, colsum_t, *mus_t, bc.NLL_COEFF, bc.C_COEFF)
        assert np.array_equal(_bits(bstat2.cpu().numpy()), _bits(got))
        for k, o1, o2 in zip(OUTS, outs1, outs2):
            assert np.array_equal(_bits(o1.cpu().numpy()), _bits(o2.cpu().numpy())), k
        ref = pe.finalize(pe.combine_bstats([g[r].astype(np.float64) for r in range(R)]),
                          colsum.astype(np.float64), bc.S * R,
                          pe.kl_term(*[mus[k] for k in bc.MU_KEYS]), bc.NLL_COEFF, bc.C_COEFF)
        for k, o in zip(OUTS, outs2):
            errs["out_" + k] = rel_err(o.cpu().numpy().astype(np.float64), ref[k])
    record(f"bstat_{R}_{B}_{kind}", errs)
    _assert_forward(errs)
    assert not bc.within_ref_rule(errs), (bc.within_ref_rule(errs), errs)


# ----------------------------------------------------------- e. reparameterisation
# which of the four pass-through outputs (mu_e, lv_e, mu_x, lv_x) receive a gradient
PASS_SETS = [(), (0, 1, 2, 3), (0, 1, 3), (2,)]
GZ_SETS = [("e", "x"), ("e",), ("x",)]


def _reparam_backward(r, leaves, c, gz_set, pass_set):
    """Gradients of the four leaves for one choice of upstream gradients."""
    outs, gouts = [], []
    for i, name in enumerate(bc.REPARAM_OUTS):
        live = (name[2:] in gz_set) if i < 2 else (i - 2 in pass_set)
        if live:
            outs.append(r[i])
            gouts.append(torch.from_numpy(c["g_" + name]).to(DEV))
    got = torch.autograd.grad(outs, leaves, gouts, retain_graph=True, allow_unused=True)
    res = [g.cpu().numpy() for g in got]
    for g in got:   # freed holding NaN, not values the next variant could find again
        g.fill_(float("nan"))
    return res


@pytest.mark.parametrize("profile", bc.PROFILES)
@pytest.mark.parametrize("shape_e,shape_x", bc.REPARAM_SHAPES)
def test_reparam(shape_e, shape_x, profile):
    """FusedReparam forward and backward against the fp64 formulas
    z = mu + eps exp(lv / 2), gmu = gz + add, glv = gz eps exp(lv / 2) / 2 + add,
    over every choice of which z receives a gradient and which pass-through
    outputs do; the mu / logvar copies bit-equal to their inputs; SingleReparam
    bit-equal to FusedReparam with the other encoder empty."""
    c = bc.reparam_case(shape_e, shape_x, profile)
    names = ("mu_e", "lv_e", "eps_e", "mu_x", "lv_x", "eps_x")
    t = {k: torch.from_numpy(c[k]).to(DEV) for k in names}
    leaves = [t[k].requires_grad_(True) for k in ("mu_e", "lv_e", "mu_x", "lv_x")]
    r = FusedReparam.apply(*[t[k] for k in names])
    errs = {}
    for e, z_dev in (("e", r[0]), ("x", r[1])):
        z, scale = bc.reparam_fwd_ref(c["mu_" + e], c["lv_" + e], c["eps_" + e])
        z32 = bc.reparam_fwd_f32(c["mu_" + e], c["lv_" + e], c["eps_" + e])
        assert z_dev.shape == z.shape
        bc.reparam_errs(z_dev.detach().cpu().numpy(), z, scale, z32, "z", errs)
    for i, k in enumerate(("mu_e", "lv_e", "mu_x", "lv_x")):
        assert np.array_equal(_bits(r[2 + i].detach().cpu().numpy()), _bits(c[k])), k
    if profile == "overflow":
        for e, shape in (("e", shape_e), ("x", shape_x)):
            if np.prod(shape):
                z_np = r[0 if e == "e" else 1].detach().cpu().numpy().reshape(-1)
                assert np.isnan(z_np[0]) and np.isinf(z_np[1]) and np.isfinite(z_np[2:]).all()
    for gz_set, pass_set in itertools.product(GZ_SETS, PASS_SETS):
        got = _reparam_backward(r, leaves, c, gz_set, pass_set)
        for j, e in enumerate(("e", "x")):
            gz = c["g_z_" + e] if e in gz_set else None
            add_mu = c["g_mu_" + e] if 2 * j in pass_set else None
            add_lv = c["g_lv_" + e] if 2 * j + 1 in pass_set else None
            gmu, glv, smu, slv = bc.reparam_bwd_ref(gz, c["lv_" + e], c["eps_" + e], add_mu, add_lv)
            gmu32, glv32 = bc.reparam_bwd_f32(gz, c["lv_" + e], c["eps_" + e], add_mu, add_lv)
            bc.reparam_errs(got[2 * j], gmu, smu, gmu32, "gmu", errs)
            bc.reparam_errs(got[2 * j + 1], glv, slv, glv32, "glv", errs)
    # SingleReparam: the encoder alone, against the fused launch bit for bit
    for e, z_fused, (mu, lv) in (("e", r[0], leaves[:2]), ("x", r[1], leaves[2:])):
        if mu.numel() == 0:
            continue
        z1 = SingleReparam.apply(mu, lv, t["eps_" + e])
        assert np.array_equal(_bits(z1.detach().cpu().numpy()), _bits(z_fused.detach().cpu().numpy()))
        gz = torch.from_numpy(c["g_z_" + e]).to(DEV)
        g1 = torch.autograd.grad([z1], [mu, lv], [gz])
        gf = torch.autograd.grad([z_fused], [mu, lv], [gz], retain_graph=True)
        for a, b in zip(g1, gf):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())), e
    tag = "x".join(map(str, shape_e)) + "_" + "x".join(map(str, shape_x))
    record(f"reparam_{tag}_{profile}", errs)
    assert not bc.within_ref_rule(errs), (bc.within_ref_rule(errs), errs)
