"""dR16s_kernel (the 256 x 256 dR GEMM tile) at the edges of its stage loops.

The kernel walks a split-K chunk in stages of 32 sample rows.  Its stage loops
are unrolled by the parity of the LDS stage image, the odd stage is peeled at
the front, and the stage that streams a chunk's last stage (the only one that
can hold rows past B*S, where noise rows are clamped) is peeled at the end.  So
what can go wrong depends on a chunk's number of stages: 1 (prologue DMA only),
2 (the peeled end alone), 3 (the peeled odd front + the end), >= 4 even / odd
(the steady loop from either parity), and on a ragged last stage.

Shapes: L = 130, z = 260 dispatch dR16s (pick_dr_tile: not both <= 128) with
one partial label tile and two z tiles, the second one partial (4 columns).
B and S, from plan_bwd (csrc/probit_bwd.hip; dr_stages below restates it; rows
= B*S, 2 tiles, an MI355X's 256 CUs, so the split-K target of 128 chunks is
capped by kc_max = cdiv(rows, 256) at every size here):

  kc   = min(128, cdiv(rows, 256))
  rpc  = cdiv(cdiv(rows, kc), 32) * 32        rows per chunk
  nKc  = cdiv(rows, rpc)                      chunks launched
  chunk k has cdiv(min(rows_pad, (k+1) rpc) - k rpc, 32) stages

  B  S    rows  rpc  stages per chunk      real rows of the last stage
  3  8      24   32  [1]                   24
  2  20     40   64  [2]                    8
  3  25     75   96  [3]                   11
  4  70    280  160  [5, 4]                24
  4  195   780  224  [7, 7, 7, 4]          12
  8  225  1800  256  [8 x 7, 1]             8
  6  265  1590  256  [8 x 6, 2]            22
  6  225  1350  256  [8 x 5, 3]             6

rows <= 256 gives one chunk (kc_max = 1), the only way to a chunk of 1, 2 or 3
stages that is also the first; above 256 rows rpc lies in {160, 192, 224, 256},
so full chunks have 5 to 8 stages and only the last chunk is short.  A chunk of
0 stages cannot be launched: nKc = cdiv(rows, rpc) leaves no chunk empty.  Every
case ends in a ragged stage (real rows not a multiple of 32).  The test checks
the table against the device's CU count before it runs a case.

Each case checks d r_sqrt_sigma of compute_loss + backward in f16x3 mode
  * against the fp64 oracle (oracle.probit_elbo) within GRAD_RTOL,
  * against the exact-fp32 mode (mpvae_gemm="f32") within GRAD_RTOL,
and two forward_local + backward_local calls on NaN-poisoned buffers
(HipShardBackend(poison=True)) for finite, bitwise equal gradients.

Measured on the MI355X (the test prints each figure): against fp64 2.0e-6 to
1.05e-5, against the fp32 mode 1.8e-6 to 2.6e-5 (B 8, S 225), GRAD_RTOL 5e-5.
"""
import argparse

import numpy as np
import pytest
import torch

import mpvae
from golden_io import DIFF
from mpvae_ops import HipShardBackend
from oracle import probit_elbo as pe
from tolerances import GRAD_RTOL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, Z, D = 130, 260, 8
NLL_COEFF, C_COEFF = 0.5, 10.0
KEYS = ["y", "fe_out", "fe_mu", "fe_logvar", "fx_out", "fx_mu", "fx_logvar"]

# B, S, stages per split-K chunk, real rows of the last stage
CASES = [
    (3, 8, [1], 24),
    (2, 20, [2], 8),
    (3, 25, [3], 11),
    (4, 70, [5, 4], 24),
    (4, 195, [7, 7, 7, 4], 12),
    (8, 225, [8] * 7 + [1], 8),
    (6, 265, [8] * 6 + [2], 22),
    (6, 225, [8] * 5 + [3], 6),
]


def dr_stages(rows, cus):
    """plan_bwd's split-K plan of the 256 tile: (stages per chunk, real rows of
    the last stage)."""
    cdiv = lambda a, b: -(-a // b)
    tiles = cdiv(L, 256) * cdiv(Z, 256)
    kc = max(cdiv(cus, tiles), cdiv(rows, 131072))
    kc = max(min(kc, cdiv(rows, 256)), 1)
    rpc = cdiv(cdiv(rows, kc), 32) * 32
    rows_pad = cdiv(rows, 32) * 32
    stages = [cdiv(min(rows_pad, (k + 1) * rpc) - k * rpc, 32) for k in range(cdiv(rows, rpc))]
    return stages, rows - (rows_pad - 32)


def case_inputs(B, S):
    rng = np.random.default_rng(L * 7 + B * S)
    y = (rng.random((B, L)) < 0.25).astype(np.float32)
    y[:, 0], y[:, 1] = 1, 0  # every row has a positive and a negative label: dR finite
    f32 = lambda a: a.astype(np.float32)
    inp = dict(y=y, fe_out=f32(rng.standard_normal((B, L))), fx_out=f32(rng.standard_normal((B, L))),
               fe_mu=f32(rng.standard_normal((B, D))), fe_logvar=f32(0.3 * rng.standard_normal((B, D))),
               fx_mu=f32(rng.standard_normal((B, D))), fx_logvar=f32(0.3 * rng.standard_normal((B, D))),
               r_sqrt_sigma=rng.uniform(-1, 1, (L, Z)) * np.sqrt(6.0 / (L + Z)))
    return inp, f32(rng.standard_normal((S, B, Z)))


def dR_of_compute_loss(inp, noise, S, gemm):
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    for k in DIFF + ["r_sqrt_sigma"]:
        t[k].requires_grad_(True)
    args = argparse.Namespace(label_dim=L, z_dim=Z, n_train_sample=S, n_test_sample=S,
                              mode="train", nll_coeff=NLL_COEFF, c_coeff=C_COEFF,
                              mpvae_noise=torch.from_numpy(noise), mpvae_gemm=gemm)
    out = mpvae.compute_loss(*[t[k] for k in KEYS], t["r_sqrt_sigma"], args)
    out[0].backward()
    return t["r_sqrt_sigma"].grad.cpu().double().numpy()


def poisoned_twice(inp, noise, B, S):
    """The packed [d fe_out | d fx_out | dR] of two launches on NaN-filled buffers."""
    be = HipShardBackend("f16x3", poison=True)
    shape = be.shape(S, S, 0, B, L, Z)
    y, fe, fx = (torch.from_numpy(inp[k]).to(DEV) for k in ("y", "fe_out", "fx_out"))
    Rop = be.prepare_R(torch.from_numpy(inp["r_sqrt_sigma"]).to(DEV))
    eps = be.prepare_noise(torch.from_numpy(noise).to(DEV), shape)
    gscal = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, 0.0], device=DEV)
    flats = []
    for _ in range(2):
        loc = be.forward_local(shape, y, fe, fx, Rop, eps, keep_T=True)
        saved = dict(y=y, fe_out=fe, fx_out=fx, eps=eps, T=loc["T"], rowstat=loc["rowstat"],
                     bstat=loc["bstat"])
        flat, _, _ = be.backward_local(shape, saved, gscal, 0b000001, None, None, NLL_COEFF,
                                       C_COEFF, True)
        flats.append(flat.clone())
    return flats


@pytest.mark.parametrize("B,S,stages,last_rows", CASES,
                         ids=[f"B{B}_S{S}" for B, S, _, _ in CASES])
def test_dr16s_stage_edges(B, S, stages, last_rows):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert dr_stages(B * S, cus) == (stages, last_rows), (dr_stages(B * S, cus), cus)
    assert last_rows % 32 != 0
    inp, noise = case_inputs(B, S)
    pos = [inp[k] for k in KEYS]
    fwd = pe.elbo_forward(*pos, inp["r_sqrt_sigma"], noise, NLL_COEFF, C_COEFF)
    ref = pe.elbo_backward(fwd, *pos, noise, NLL_COEFF, C_COEFF, g_total=1.0)["r_sqrt_sigma"]
    assert np.isfinite(ref).all() and ref.any()
    d16 = dR_of_compute_loss(inp, noise, S, "f16x3")
    d32 = dR_of_compute_loss(inp, noise, S, "f32")
    a, b = poisoned_twice(inp, noise, B, S)
    e_ref, e_32 = rel_err(d16, ref), rel_err(d16, d32)
    n_diff = int((a != b).sum())
    n_nan = int((~torch.isfinite(a)).sum() + (~torch.isfinite(b)).sum())
    print(f"dr_edges B={B} S={S} stages={stages}: vs fp64 {e_ref:.3g}, vs f32 mode {e_32:.3g}, "
          f"poisoned repeat: {n_diff} differ, {n_nan} not finite")
    assert d16.shape == (L, Z)
    assert e_ref <= GRAD_RTOL, e_ref
    assert e_32 <= GRAD_RTOL, e_32
    assert n_nan == 0 and n_diff == 0, (n_nan, n_diff)
    # the poisoned launches computed the same dR as the autograd path
    dR_p = a[2 * B * L:].reshape(L, Z).cpu().double().numpy()
    assert rel_err(dR_p, ref) <= GRAD_RTOL
