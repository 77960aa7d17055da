"""Guard bands round every kernel's outputs and workspaces (tests/guarded_alloc.py).

The rest of the GPU suite pins values.  Nothing there sees a store a kernel
should not make: one past the end of an output or a workspace, or one over an
input.  It does not fault (the caching allocator packs blocks and rounds each
to 512 B) and does not change the value under test.  Here every product call
runs twice: plainly, and with the wrapper module's ``torch`` swapped for a
GuardedTorch, so that each buffer the wrapper allocates (outputs, workspaces,
split planes, gradient buffers) is the 0xFF-poisoned body of its own arena with
256 KiB of 0xA5 in front and 2 MiB behind, and the test's own inputs sit in such
arenas too.  Every case asserts

  1. no guard byte changed and no input changed (``check()``);
  2. every result is bitwise the plain call's (NaN at the same places, the
     same bits elsewhere) -- a kernel that *reads* a neighbour's bytes finds
     0xA5 / 0xFF there instead of the allocator's leftovers;
  3. at least the stated number of buffers was guarded (the literal in the
     case table, read off the wrapper's allocations), so that a case cannot
     pass by guarding nothing.

No tolerance: the kernels reduce in a fixed order and the suite holds them to
bitwise repeatability elsewhere.  The shapes, inputs and tables are the other
GPU tests' own (imported), each the smallest that selects its kernel path.

Measured on the MI355X: 146 cases in 6.5 s (the slowest 0.8 s), every one with
0 bad bytes and exactly the stated number of guarded buffers.  What the guards
were seen to report on wrong builds (run under guards only, never plainly):
lin_gemm_kernel without its j < N store mask, linear forward + backward at
(33, 17, 65): 252 bytes behind y (33, 65) from offset 8580, the end of its
body, and 72 bytes behind the 16 384-byte workspace; the host library's
finalize writing one row too many at L = 38 (tests/test_guarded_alloc.py's
path): 304 bytes, the first at offset 1216 of an (8, 38) fp32 output.
"""
import argparse

import numpy as np
import pytest
import torch

import batch_axis_cases as bc
import fair_cases as fc
import mpvae
import mpvae_fair
import mpvae_linear
import mpvae_ops
import mpvae_step
from golden_io import OUTS
from guarded_alloc import guard, same_bits
from live_io import GRADS, KEYS, SCALARS
from mpvae_ops import FusedReparam, HipShardBackend
from test_gpu_bwd_lattice import LATTICE_SHAPES, W, lattice_inputs
from test_gpu_calib import BY as CALIB_GOLDEN, EDGES as CALIB_EDGES, _edge_case
from test_gpu_curves import _seeded
from test_gpu_dr_edges import CASES as DR_CASES, case_inputs as dr_case_inputs, dr_stages
from test_gpu_eval import make_case as eval_case
from test_gpu_predict import SHAPES as PREDICT_SHAPES, _args as predict_args, _case as predict_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NLL_COEFF, C_COEFF = 0.5, 10.0


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _plain(t, role="input"):
    """What alloc_like is to the guarded run: a private copy."""
    return t.detach().clone()


def _both(monkeypatch, modules, run, min_buffers, what):
    """run(alloc) -> {name: tensor or None}: once plainly, once with `modules`
    guarded and alloc = GuardedTorch.alloc_like; the three assertions."""
    plain = run(_plain)
    torch.cuda.synchronize()
    g = guard(monkeypatch, *modules, device=DEV)
    got = run(g.alloc_like)
    rep = g.check()
    n_product = sum(1 for r in g.records if not r.own)
    print(f"{what}: {rep.n_buffers} arenas ({n_product} the wrapper's), "
          f"{rep.n_bad_bytes} bad bytes, first {rep.first}")
    assert rep.n_bad_bytes == 0, (what, rep)
    assert n_product >= min_buffers, (what, n_product, min_buffers)
    assert set(got) == set(plain)
    diff = [k for k in got if not same_bits(got[k], plain[k])]
    assert not diff, (what, "differs from the plain call", diff)
    return g, got


# ====================================================================== ELBO
# the wrapper's allocations of compute_loss + backward on explicit noise:
#   f16x3: noise planes 2 + split ws 1, R planes 2 + split ws 1; f32: R -> fp32 1 (fp64 R only)
#   forward_local T, rowstat, bstat, colsum, ws 5; finalize 6 scalars + 2 = 8
#   backward: the zero of gscal 1, flat 1, ws 1, the four KL gradients 4, dR64 1 (fp64 R only)
ELBO_MIN = {("f16x3", "r64"): 27, ("f16x3", "r32"): 26, ("f32", "r64"): 22, ("f32", "r32"): 20}


def _upstream(B, L, seed):
    rng = np.random.default_rng([seed, B, L, 99])
    return (rng.standard_normal((B, L)).astype(np.float32),
            rng.standard_normal((B, L)).astype(np.float32))


def _elbo_run(inp, noise, S, gemm, rkind, g_I, g_IL, mode="train", seed=None):
    """compute_loss (+ backward of all eight outputs under non-unit upstream
    gradients) as a run(alloc) for _both.  seed: Philox noise from a device key
    that the finalize launch advances."""
    L, z = inp["r_sqrt_sigma"].shape

    def run(alloc):
        t = {k: alloc(_dev(inp[k])) for k in KEYS}
        t["r_sqrt_sigma"] = alloc(_dev(inp["r_sqrt_sigma"],
                                       torch.float32 if rkind == "r32" else torch.float64))
        if mode == "train":
            for k in GRADS:
                t[k].requires_grad_(True)
        args = argparse.Namespace(label_dim=L, z_dim=z, n_train_sample=S, n_test_sample=S,
                                  mode=mode, nll_coeff=NLL_COEFF, c_coeff=C_COEFF,
                                  mpvae_gemm=gemm)
        key = None
        if seed is None:
            args.mpvae_noise = alloc(_dev(noise))
        else:
            key = alloc(torch.tensor([seed], dtype=torch.int64, device=DEV), role="output")
            args.mpvae_noise, args.mpvae_seed, args.mpvae_seed_advance = "philox", key, True
        out = mpvae.compute_loss(*[t[k] for k in KEYS], t["r_sqrt_sigma"], args)
        res = {"out_" + k: o.detach() for k, o in zip(OUTS, out)}
        if mode == "train":
            ups = {k: alloc(torch.tensor(W[k], dtype=torch.float32, device=DEV)) for k in SCALARS}
            gi, gil = alloc(_dev(g_I)), alloc(_dev(g_IL))
            (sum(out[OUTS.index(k)] * ups[k] for k in SCALARS) + (out[6] * gi).sum()
             + (out[7] * gil).sum()).backward()
            for k in GRADS:
                assert t[k].grad is not None and t[k].grad.dtype == t[k].dtype, k
                res["d_" + k] = t[k].grad
        if key is not None:
            res["seed"] = key
        return res
    return run


# L, z, B, S, d: the three shapes of test_forward_tile_walks (tps > 1)
TILE_WALKS = [(100, 37, 130, 257, 8), (260, 64, 128, 130, 8), (260, 64, 128, 300, 8)]


@pytest.mark.parametrize("gemm", ["f16x3", "f32"])
@pytest.mark.parametrize("rkind", ["r64", "r32"])
@pytest.mark.parametrize("L,z,B,S,d", LATTICE_SHAPES)
def test_elbo_lattice_shapes(L, z, B, S, d, rkind, gemm, monkeypatch):
    """One forward tile, element pass and dR tile each (LATTICE_SHAPES); fp64
    r_sqrt_sigma: dR in its own fp64 buffer, fp32: packed behind d fe_out |
    d fx_out."""
    inp, noise, g_I, g_IL = lattice_inputs(L, z, B, S, d, L * 7 + S)
    _both(monkeypatch, [mpvae_ops], _elbo_run(inp, noise, S, gemm, rkind, g_I, g_IL),
          ELBO_MIN[gemm, rkind], f"lattice {L}/{z}/{B}/{S} {rkind} {gemm}")


@pytest.mark.parametrize("rkind", ["r64", "r32"])
@pytest.mark.parametrize("L,z,B,S,d", TILE_WALKS)
def test_elbo_tile_walks(L, z, B, S, d, rkind, monkeypatch):
    inp, noise, g_I, g_IL = lattice_inputs(L, z, B, S, d, L * 7 + S)
    _both(monkeypatch, [mpvae_ops], _elbo_run(inp, noise, S, "f16x3", rkind, g_I, g_IL),
          ELBO_MIN["f16x3", rkind], f"tile walk {L}/{z}/{B}/{S} {rkind}")


@pytest.mark.parametrize("rkind", ["r64", "r32"])
@pytest.mark.parametrize("B,S,stages,last_rows", DR_CASES,
                         ids=[f"B{B}_S{S}" for B, S, _, _ in DR_CASES])
def test_elbo_dr_stage_edges(B, S, stages, last_rows, rkind, monkeypatch):
    """dR16s at L 130, z 260: one to eight stages per split-K chunk, a ragged
    last stage (test_gpu_dr_edges.py's table, held to the device's CU count)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert dr_stages(B * S, cus) == (stages, last_rows), (dr_stages(B * S, cus), cus)
    inp, noise = dr_case_inputs(B, S)
    g_I, g_IL = _upstream(B, 130, S)
    _both(monkeypatch, [mpvae_ops], _elbo_run(inp, noise, S, "f16x3", rkind, g_I, g_IL),
          ELBO_MIN["f16x3", rkind], f"dR stages B{B} S{S} {rkind}")


@pytest.mark.parametrize("gemm", ["f16x3", "f32"])
@pytest.mark.parametrize("rkind", ["r64", "r32"])
@pytest.mark.parametrize("d", [4, 129])
def test_elbo_batch_axis(d, rkind, gemm, monkeypatch):
    """B = 1025: finalize's second pass over b, bwd_coef's fused KL (d = 129:
    its stride loop and the scalar KL loop of finalize)."""
    B = 1025
    c = bc.elbo_case(B, d, "tame")
    g_I, g_IL = _upstream(B, bc.L, d)
    _both(monkeypatch, [mpvae_ops],
          _elbo_run(c, c["noise"], bc.S, gemm, rkind, g_I, g_IL), ELBO_MIN[gemm, rkind],
          f"batch axis B{B} d{d} {rkind} {gemm}")


# forward only, mode "test" (keep_T False): the operands as above, forward_local without T 4,
# finalize 8
TEST_MODE_MIN = {"f16x3": 18, "f32": 13}


@pytest.mark.parametrize("gemm", ["f16x3", "f32"])
@pytest.mark.parametrize("L,z,B,S,d", [LATTICE_SHAPES[0], TILE_WALKS[2],
                                       (38, 38, 2, 2000, 8)])  # 8 / 16 s-chunks: column partials
def test_elbo_test_mode_forward(L, z, B, S, d, gemm, monkeypatch):
    inp, noise, g_I, g_IL = lattice_inputs(L, z, B, S, d, L * 7 + S)
    _both(monkeypatch, [mpvae_ops],
          _elbo_run(inp, noise, S, gemm, "r64", g_I, g_IL, mode="test"), TEST_MODE_MIN[gemm],
          f"test mode {L}/{z}/{B}/{S} {gemm}")


# Philox noise made on the device.  f16x3: planes 2 and R planes 2 in one launch when
# L z <= SPLIT_WITH_NOISE = 16384, else planes 2 + (R planes 2 + split ws 1); f32: the fp32 draw 1
# and the fp32 R 1; then forward, finalize and backward as above
@pytest.mark.parametrize("L,z,B,S,d,gemm,one_launch,min_buffers", [
    (38, 38, 4, 37, 8, "f16x3", True, 25),
    (200, 64, 4, 40, 8, "f16x3", True, 25),     # 12 800 elements: still the one launch
    (700, 64, 3, 40, 8, "f16x3", False, 26),    # 44 800: the noise launch, then mpv_split_f16
    (38, 38, 4, 37, 8, "f32", True, 23),        # noise_philox_kernel's fp32 (S, B, z) draw
])
def test_elbo_device_philox_noise(L, z, B, S, d, gemm, one_launch, min_buffers, monkeypatch):
    """The noise kernel (and the R split riding on it) writing the guarded
    planes; the device key is an input the finalize launch is allowed to
    advance: registered as an output, and advanced by exactly 1."""
    assert (L * z <= HipShardBackend.SPLIT_WITH_NOISE) == one_launch
    inp, _, g_I, g_IL = lattice_inputs(L, z, B, S, d, L * 7 + S)
    seed = 0x1234ABCD5678 + L
    _, got = _both(monkeypatch, [mpvae_ops],
                   _elbo_run(inp, None, S, gemm, "r64", g_I, g_IL, seed=seed), min_buffers,
                   f"philox {L}/{z}/{B}/{S} {gemm}")
    assert got["seed"].tolist() == [seed + 1]


# per shard: the packed statistics, rowstat, T, ws 4 and backward's flat, ws 2; the operands
# (f16x3: noise planes 2 + ws 1 per shard, R planes 2 + ws 1; f32: the fp32 R 1); finalize_slots 9
SHARD_MIN = {"f16x3": 2 * 6 + 2 * 3 + 3 + 9, "f32": 2 * 6 + 1 + 9}


@pytest.mark.parametrize("gemm", ["f16x3", "f32"])
@pytest.mark.parametrize("L,z,B,S,d", [(38, 38, 4, 37, 8), (200, 64, 4, 40, 8)])
def test_elbo_two_shards_packed_statistics(L, z, B, S, d, gemm, monkeypatch):
    """Two S-shards as test_shards_against_oracle drives them, with the packed
    [colsum | 2 x bstat] buffer: each shard writes its own slot beside the
    other's (which must stay zero), then finalize_slots and backward_local
    with every upstream gradient live and dR packed behind d fe_out | d fx_out."""
    inp, noise, g_I, g_IL = lattice_inputs(L, z, B, S, d, L * 7 + S + 1)
    edges = [0, S // 2 + 1, S]
    n = 2 * B * L

    def run(alloc):
        t = {k: alloc(_dev(inp[k])) for k in KEYS + ["r_sqrt_sigma"]}
        mus = [t[k] for k in ("fe_mu", "fe_logvar", "fx_mu", "fx_logvar")]
        noise_t = _dev(noise)
        be = HipShardBackend(gemm)
        Rop = be.prepare_R(t["r_sqrt_sigma"])
        parts, res = [], {}
        for slot, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            shape = be.shape(b - a, S, a, B, L, z)
            eps = be.prepare_noise(alloc(noise_t[a:b].contiguous()), shape)
            loc = be.forward_local(shape, t["y"], t["fe_out"], t["fx_out"], Rop, eps, keep_T=True,
                                   stat_slots=(2, slot))
            other = loc["packed"][n + (1 - slot) * 6 * B:n + (2 - slot) * 6 * B]
            assert not other.any(), "the other shard's slot is not zero"
            parts.append((shape, eps, loc))
            res[f"packed{slot}"], res[f"rowstat{slot}"] = loc["packed"].clone(), loc["rowstat"]
        packed = parts[0][2]["packed"] + parts[1][2]["packed"]        # the all_reduce(SUM)
        bstat, outs = be.finalize_slots(parts[0][0], packed[n:].view(2, 6, B),
                                        packed[:n].view(2, B, L), *mus, NLL_COEFF, C_COEFF)
        res["bstat"] = bstat
        res.update({"out_" + k: o for k, o in zip(OUTS, outs)})
        gscal = alloc(torch.tensor([W[k] for k in SCALARS], dtype=torch.float32, device=DEV))
        gi, gil = alloc(_dev(g_I)), alloc(_dev(g_IL))
        for slot, (shape, eps, loc) in enumerate(parts):
            saved = dict(y=t["y"], fe_out=t["fe_out"], fx_out=t["fx_out"], eps=eps, T=loc["T"],
                         rowstat=loc["rowstat"], bstat=bstat)
            flat, _, dR = be.backward_local(shape, saved, gscal, 0b111111, gi, gil, NLL_COEFF,
                                            C_COEFF, True)
            assert dR.data_ptr() == flat.data_ptr() + 4 * n
            res[f"flat{slot}"] = flat
        torch.cuda.synchronize()
        return res

    _both(monkeypatch, [mpvae_ops], run, SHARD_MIN[gemm], f"shards {L}/{z}/{B}/{S} {gemm}")


# ================================================================ prediction
# f16x3: noise planes 2 + ws 1, R planes 2 + ws 1, colsum, indiv_prob, ws; f32: the fp32 R 1 + 3
PREDICT_MIN = {"f16x3": 9, "f32": 4}


@pytest.mark.parametrize("gemm", ["f16x3", "f32"])
@pytest.mark.parametrize("i", [0, 4, 6, 7])
def test_predict_proba(i, gemm, monkeypatch):
    shape = PREDICT_SHAPES[i]
    t, eps, _ = predict_case(shape)

    def run(alloc):
        p = mpvae.predict_proba(alloc(t["fx_out"]), alloc(t["r_sqrt_sigma"]),
                                predict_args(shape, mpvae_noise=alloc(eps), mpvae_gemm=gemm))
        return {"indiv_prob": p}

    _both(monkeypatch, [mpvae_ops], run, PREDICT_MIN[gemm], f"predict {shape} {gemm}")


# ==================================================== reparameterisation, KL
@pytest.mark.parametrize("shape_e,shape_x", bc.REPARAM_SHAPES)
def test_fused_reparam(shape_e, shape_x, monkeypatch):
    """Forward (z of both encoders and the four mu / logvar copies: 6 buffers)
    and backward with all four pass-through gradients (4 buffers)."""
    c = bc.reparam_case(shape_e, shape_x, "tame")
    names = ("mu_e", "lv_e", "eps_e", "mu_x", "lv_x", "eps_x")

    def run(alloc):
        t = {k: alloc(_dev(c[k])) for k in names}
        leaves = [t[k].requires_grad_(True) for k in ("mu_e", "lv_e", "mu_x", "lv_x")]
        r = FusedReparam.apply(*[t[k] for k in names])
        gouts = [alloc(_dev(c["g_" + k])) for k in bc.REPARAM_OUTS]
        grads = torch.autograd.grad(r, leaves, gouts)
        res = {k: o.detach() for k, o in zip(bc.REPARAM_OUTS, r)}
        res.update({"g" + str(j): g for j, g in enumerate(grads)})
        return res

    _both(monkeypatch, [mpvae_ops], run, 10, f"reparam {shape_e} {shape_x}")


def test_standalone_kl_backward(monkeypatch):
    B, d = 1025, 129
    c = bc.elbo_case(B, d, "tame")

    def run(alloc):
        mus = [alloc(_dev(c[k])) for k in bc.MU_KEYS]
        gscal = alloc(torch.tensor([W[k] for k in SCALARS], dtype=torch.float32, device=DEV))
        outs = HipShardBackend().kl_backward(*mus, gscal)
        return dict(zip(bc.MU_KEYS, outs))

    _both(monkeypatch, [mpvae_ops], run, 4, f"kl_backward B{B} d{d}")


# ============================================================= linear layers
def _guarded_layer(alloc, K, N, seed):
    torch.manual_seed(seed)
    layer = torch.nn.Linear(K, N).to(DEV)
    layer.weight.data, layer.bias.data = alloc(layer.weight), alloc(layer.bias)
    return layer


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _layer_grads(res, tag, layer):
    res["dW" + tag], res["db" + tag] = layer.weight.grad, layer.bias.grad
    assert layer.weight.grad is not None and layer.bias.grad is not None


# forward: y, ws; backward: dx, dW, db, ws
@pytest.mark.parametrize("relu,alpha", [(True, 1.0), (False, 1.7)])
@pytest.mark.parametrize("M,K,N", [(1, 1, 1), (33, 17, 65), (257, 129, 3),
                                   (5, 2100, 70),       # 66 reduction chunks, a ragged last one
                                   (128, 1038, 512)])   # dW with the ones column, a 3-way split
def test_linear(M, K, N, relu, alpha, monkeypatch):
    def run(alloc):
        layer = _guarded_layer(alloc, K, N, 0)
        x = alloc(_randn((M, K), M * 7 + K + N)).requires_grad_(True)
        y = mpvae_linear.linear(x, layer, relu, alpha)
        y.backward(alloc(_randn((M, N), M + 1)))
        res = {"y": y.detach(), "dx": x.grad}
        _layer_grads(res, "", layer)
        return res

    _both(monkeypatch, [mpvae_linear], run, 6, f"linear {M}x{K}x{N} relu={relu}")


def test_linear_with_dropout(monkeypatch):
    M, K, N = 33, 17, 65

    def run(alloc):
        layer = _guarded_layer(alloc, K, N, 7)
        x = alloc(_randn((M, K), 3)).requires_grad_(True)
        torch.cuda.manual_seed(123)     # torch's dropout kernel: the same masks in both runs
        y = mpvae_linear.linear(x, layer, True, 1.0, 0.5)
        y.backward(alloc(_randn((M, N), 4)))
        res = {"y": y.detach(), "dx": x.grad}
        _layer_grads(res, "", layer)
        return res

    _both(monkeypatch, [mpvae_linear], run, 6, "linear 33x17x65 drop_p=0.5")


# forward: two y, ws; backward: dx, two (dW, db), ws
@pytest.mark.parametrize("M,K,Na,Nb", [(7, 20, 6, 3),
                                       (128, 256, 50, 50)])  # segment 2 starts mid-stage
def test_linear_heads(M, K, Na, Nb, monkeypatch):
    def run(alloc):
        la, lb = _guarded_layer(alloc, K, Na, M + K), _guarded_layer(alloc, K, Nb, M + K + 1)
        x = alloc(_randn((M, K), 5)).requires_grad_(True)
        ya, yb = mpvae_linear.heads(x, la, lb, 1.3)
        torch.autograd.backward((ya, yb), (alloc(_randn((M, Na), 6)), alloc(_randn((M, Nb), 7))))
        res = {"ya": ya.detach(), "yb": yb.detach(), "dx": x.grad}
        _layer_grads(res, "a", la), _layer_grads(res, "b", lb)
        return res

    _both(monkeypatch, [mpvae_linear], run, 9, f"heads {M}x{K}x{Na}+{Nb}")


@pytest.mark.parametrize("M,n_a,K,Na,Nb", [(7, 3, 20, 5, 4), (64, 0, 33, 6, 6), (64, 64, 33, 6, 6)])
def test_linear_row_heads(M, n_a, K, Na, Nb, monkeypatch):
    """n_a = 0 and n_a = M: an empty problem inside the batch."""
    def run(alloc):
        la, lb = _guarded_layer(alloc, K, Na, M + n_a), _guarded_layer(alloc, K, Nb, M + n_a + 1)
        h = alloc(_randn((M, K), 8)).requires_grad_(True)
        ya, yb = mpvae_linear.row_heads(h, la, lb, n_a)
        torch.autograd.backward((ya, yb), (alloc(_randn((n_a, Na), 9)),
                                           alloc(_randn((M - n_a, Nb), 10))))
        res = {"ya": ya.detach(), "yb": yb.detach(), "dh": h.grad}
        _layer_grads(res, "a", la), _layer_grads(res, "b", lb)
        return res

    _both(monkeypatch, [mpvae_linear], run, 9, f"row_heads {M}/{n_a}x{K}x{Na}+{Nb}")


# ======================================== fairness, metrics, validation, calibration
def _tables(alloc, dists, L):
    """LabelDistanceTables whose device arrays are the test's inputs too."""
    tables = [mpvae_fair.LabelDistanceTable(d, L, DEV) for d in dists]
    for tab in tables:
        tab.keys, tab.vals, tab.used = alloc(tab.keys), alloc(tab.vals), alloc(tab.used)
    return tables


# label_weights w, count 2; sensitive_groups counts, goff 2; fair_fwd ws, out 2; fair_bwd 2 grads
@pytest.mark.parametrize("norm", fc.FP_NORMS)
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("L", [255, 256, 257, 513])
def test_fairness_penalty(L, B, norm, monkeypatch):
    c = fc.penalty_case(L, B, 3, "all", norm)

    def run(alloc):
        tables = _tables(alloc, c["dists"], L)
        lz = alloc(_dev(c["label_z"])).requires_grad_(True)
        fz = alloc(_dev(c["feat_z"])).requires_grad_(True)
        loss, count = mpvae_fair.fairness_penalty(lz, fz, alloc(_dev(c["labels"])),
                                                  alloc(_dev(c["sensitive"])), tables, norm,
                                                  c["coeff"], max_groups=c["max_groups"])
        (2.5 * loss).backward()
        return {"loss": loss.detach(), "count": count, "g_label_z": lz.grad, "g_feat_z": fz.grad}

    _both(monkeypatch, [mpvae_fair], run, 8, f"fair penalty L{L} B{B} {norm}")


@pytest.mark.parametrize("batched", [False, True], ids=["per_table", "one_launch"])
@pytest.mark.parametrize("L", [63, 64, 65, 4095])
def test_label_weights_three_tables(L, batched, monkeypatch):
    B = 9
    c = fc.weight_pair_case(L, B)
    rng = np.random.default_rng([43, L])
    keys = [fc.key_of(r) for r in c["labels"]]
    dists = c["dists"] + [{k: np.float64(rng.uniform(0.1, 1)) for k in keys[1::2]},
                          {keys[4]: 0.75}]
    fn = mpvae_fair.label_weights_batch if batched else mpvae_fair.label_weights

    def run(alloc):
        w, count = fn(alloc(_dev(c["labels"])), _tables(alloc, dists, L))
        assert w.shape == (3, B) and int(count) > 0
        return {"w": w, "count": count}

    _both(monkeypatch, [mpvae_fair], run, 2, f"label weights L{L} batched={batched}")


def test_device_group_ids(monkeypatch):
    """mpv_group_rows on every input of fair_cases.group_inputs(): gid, order,
    goff and the overflow flag are 4 guarded buffers per call."""
    inputs = fc.group_inputs()
    picks = [(X, (None, 3)[n % 2]) for n, X in enumerate(inputs)]

    def run(alloc):
        res = {}
        for n, (X, mg) in enumerate(picks):
            gid, order, goff, G, overflow = mpvae_fair.group_rows(alloc(X.to(DEV)), mg)
            res.update({f"gid{n}": gid, f"order{n}": order, f"goff{n}": goff, f"over{n}": overflow})
        return res

    _both(monkeypatch, [mpvae_fair], run, 4 * len(picks), "group_rows")
    assert len(picks) == 402


@pytest.mark.parametrize("L", [1, 5, 255, 256, 257, 513])
def test_train_metrics(L, monkeypatch):
    p, t = fc.metrics_case(L, 5)

    def run(alloc):
        res = mpvae_fair.compute_metrics(alloc(_dev(p)), alloc(_dev(t)), 0.5)
        return {k: res[k] for k in mpvae_fair.METRIC_KEYS}

    _both(monkeypatch, [mpvae_fair], run, 2, f"train metrics L{L}")   # ws, out


@pytest.mark.parametrize("N,L,chunk", [(mpvae_fair.CURVE_CHUNK + 1, 3, 0), (96, 130, 0),
                                       (96, 130, 64), (300, 9, 64)])
def test_curve_metrics(N, L, chunk, monkeypatch):
    """Sort keys and merge runs in the workspace: the LDS path, the global
    merge passes (chunk 64) with a ragged tail and a run without a partner."""
    p, t = _seeded(N, L, 32, 7 * N + L)

    def run(alloc):
        res = mpvae_fair.curve_metrics(alloc(_dev(p)), alloc(_dev(t)), chunk)
        return {k: v for k, v in res.items()}

    _both(monkeypatch, [mpvae_fair], run, 3, f"curves N{N} L{L} chunk{chunk}")  # ws, per, agg


@pytest.mark.parametrize("n_thr", [1, 64, 70])
@pytest.mark.parametrize("N,L", [(1, 1), (130, 65), (261, 257)])
def test_threshold_sweep(N, L, n_thr, monkeypatch):
    p, t = _seeded(N, L, 32, 7 * N + L)
    thr = [0.37] if n_thr == 1 else [float(x) for x in
                                     np.linspace(-0.05, 1.05, n_thr).astype(np.float32)]

    def run(alloc):
        return {"table": mpvae_fair.threshold_sweep_metrics(alloc(_dev(p)), alloc(_dev(t)), thr)}

    # out, and a workspace per slice of 64 thresholds
    _both(monkeypatch, [mpvae_fair], run, 3 if n_thr > 64 else 2, f"sweep N{N} L{L} x{n_thr}")


def _calib_cases():
    cases = {}
    for name, (B, L, T, G, empty, ll, R, small) in CALIB_EDGES.items():
        cases[name] = (lambda name=name, a=(B, L, T, G, empty, ll), small=small:
                       _edge_case(*a, seed=len(name), small_group=small), R, T)
    gold = CALIB_GOLDEN["c7_l257"]
    cases["golden_c7_l257"] = (lambda: gold, 2, len(gold["dists"]))
    return cases


CALIB = _calib_cases()


@pytest.mark.parametrize("name", CALIB)
def test_calibration(name, monkeypatch):
    """calibration_loss forward + backward (d threshold and d indiv_prob).
    Buffers: label_weights w, count 2 (count alone without tables), the group
    layout's counts, goff 2, calib_fwd ws, out, cal_prob 3, backward's zero, gx,
    gp 3."""
    build, R, T = CALIB[name]
    f = build()
    L = f["labels"].shape[1]

    def run(alloc):
        p = alloc(_dev(f["p"])).requires_grad_(True)
        x = alloc(_dev(f["threshold"])).requires_grad_(True)
        bce, fair, cal, active, contributed = mpvae_fair.calibration_loss(
            p, x, alloc(_dev(f["labels"])), alloc(_dev(f["sensitive"])),
            alloc(_dev(f["centroids"])), _tables(alloc, f["dists"], L), f["learn_logit"], slices=R)
        (0.75 * bce + 1.5 * fair).backward()
        return {"bce": bce.detach(), "fair": fair.detach(), "cal_prob": cal, "active": active,
                "contributed": contributed, "g_threshold": x.grad, "g_p": p.grad}

    _both(monkeypatch, [mpvae_fair], run, 10 if T else 9, f"calibration {name}")


# counts, out, terms, ws; with definitions out_defs too
@pytest.mark.parametrize("D", [None, 2], ids=["one_definition", "two_definitions"])
def test_split_eval(D, monkeypatch):
    """mpv_split_eval and mpv_split_eval_defs at N 24, L 257, G 3, R 2 with 5
    targets a definition (past the register tile of 4): every piece of the
    workspace is non-empty."""
    c = eval_case(L=257, N=24, G=3, T=5 * (D or 1), R=2)

    def run(alloc):
        order, goff = mpvae_fair._group_layout(_dev(c["gid"].astype(np.int32)), c["G"])
        res = mpvae_fair._split_eval(alloc(_dev(c["pred"])), alloc(_dev(c["y"])),
                                     alloc(_dev(c["w"])), alloc(order), alloc(goff), c["G"],
                                     c["R"], D)
        return dict(zip(("counts", "out", "terms", "out_defs"), res))

    _both(monkeypatch, [mpvae_fair], run, 4 if D is None else 5, f"split eval D={D}")


# ====================================================================== Adam
def _adam_case(n_tensors, numels, steps, inf_step, monkeypatch, what):
    """mpvae_step.adam_step on guarded parameters, gradients and (zeros_like)
    state against torch's fused capturable Adam + host StepLR, driven as
    test_native_adam_matches_torch_fused_adam drives them: two param groups
    with their own lr and weight decay (one 0), StepLR(step_size 2), a skipped
    (found_inf) update at `inf_step`."""
    g = guard(monkeypatch, mpvae_step, device=DEV)
    gen = torch.Generator().manual_seed(11 + n_tensors)
    shapes = [((numels[i % len(numels)],), torch.float64 if i % 5 == 4 else torch.float32)
              for i in range(n_tensors)]
    init = [torch.randn(s, dtype=dt, generator=gen).to(DEV) for s, dt in shapes]
    ps = [torch.nn.Parameter(v.clone()) for v in init]
    qs = [torch.nn.Parameter(g.alloc_like(v, role="output")) for v in init]
    half = n_tensors // 2
    groups = lambda xs: [dict(params=xs[:half], lr=7.5e-4, weight_decay=1e-5),
                         dict(params=xs[half:], lr=3e-4, weight_decay=0.0)]
    ref = torch.optim.Adam(groups(ps), fused=True, capturable=True)
    mine = torch.optim.Adam(groups(qs), fused=True, capturable=True)
    assert mpvae_step._native_adam(mine)
    sref = torch.optim.lr_scheduler.StepLR(ref, 2, 0.3)
    dsched = mpvae_step.DeviceStepLR(torch.optim.lr_scheduler.StepLR(mine, 2, 0.3), mine)
    dsched.lr = g.alloc_like(dsched.lr, role="output")
    dsched.last_epoch = g.alloc_like(dsched.last_epoch, role="output")
    updates = g.alloc_like(torch.zeros((), dtype=torch.int64, device=DEV), role="output")
    applied = 0
    for it in range(steps):
        found = g.alloc_like(torch.full((), 1.0 if it == inf_step else 0.0, device=DEV))
        for p, q in zip(ps, qs):
            grad = (torch.randn(p.shape, dtype=p.dtype, generator=gen)
                    * (10.0 if it == 0 else 1.0)).to(DEV)
            p.grad, q.grad = grad.clone(), g.alloc_like(grad)
        ref.found_inf = found
        ref.step()
        del ref.found_inf
        if it != inf_step:
            sref.step()
            applied += 1
        mpvae_step.adam_step(mine, found, updates=updates, sched=dsched)
        # once per optimizer step, not once per finish launch
        assert int(updates) == applied and int(dsched.last_epoch) == sref.last_epoch == applied, it
        assert dsched.lr.tolist() == [gr["lr"] for gr in ref.param_groups], it
        for i, (p, q) in enumerate(zip(ps, qs)):
            sp, sq = ref.state[p], mine.state[q]
            assert torch.equal(sp["step"], sq["step"]), (it, i, sp["step"], sq["step"])
            assert torch.equal(p, q), (it, i, "param")
            assert torch.equal(sp["exp_avg"], sq["exp_avg"]), (it, i, "exp_avg")
            assert torch.equal(sp["exp_avg_sq"], sq["exp_avg_sq"]), (it, i, "exp_avg_sq")
    assert [gr["lr"] for gr in ref.param_groups] != [7.5e-4, 3e-4]     # the decay happened
    rep = g.check()
    n_product = sum(1 for r in g.records if not r.own)
    print(f"{what}: {rep.n_buffers} arenas ({n_product} the wrapper's), {rep.n_bad_bytes} bad bytes,"
          f" first {rep.first}")
    assert rep.n_bad_bytes == 0, rep          # guards, the gradients and found_inf
    assert n_product >= 3 * n_tensors         # step, exp_avg, exp_avg_sq of every parameter


def test_adam_ragged_blocks_two_groups(monkeypatch):
    """70 tensors, 35 per group: the > 32 tensors chunk loop of adam_step in
    both groups, 2048-element blocks over ragged fp32 and fp64 tensors."""
    _adam_case(70, [1, 7, 2047, 2048, 2049, 4097], 5, 2, monkeypatch, "adam 70 tensors")


def test_adam_two_finish_launches(monkeypatch):
    """300 one-element tensors: 300 step counters > 256, two mpv_adam_finish
    launches, of which only the first may count the update and step the lr."""
    _adam_case(300, [1], 3, None, monkeypatch, "adam 300 tensors")
