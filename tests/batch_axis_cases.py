"""Seeded cases, fp64 references and elementwise error metrics of the batch (B)
and latent (d) axis tests: tests/test_gpu_batch_axis.py on the GPU,
tests/test_batch_axis_host.py on the host library.  Imports no GPU code.

References: oracle.probit_elbo (combine_bstats, kl_term, kl_backward, finalize,
elbo_forward / elbo_backward).  The reparameterisation has no oracle; its fp64
formulas are stated here (reparam_fwd_ref / reparam_bwd_ref).

Logvar profiles (PROFILES): "tame" 0.3 N(0,1); "wide" 8 N(0,1) clipped to +-30
with planted pairs lve - lvx in {+-60, +-80} and lvx in {-30, -13.8, +30};
"overflow" tame with a few elements lve = 0, lvx = -100 (lve - lvx = +100:
fp32 exp overflows, 11 above its threshold 88.7; e^lvx = e^-100 is an fp32
subnormal, but it only ever meets the 1e-6 beside it, 10^38 times larger, so
neither its last bits nor a flush to zero can reach a result).

Metric: elementwise, in units of u = 2^-24, each difference from the fp64 value
divided by a scale that models one fp32 evaluation of the formula (|x| u for an
exp of a rounded argument x); a scale is floored at 2^-125, since below the
normal range fp32 is spaced by 2^-149 = 2^-125 u whatever the value.  Bound
(within_ref_rule): the same formulas evaluated in torch CPU fp32 on the same
inputs are measured in the same metric, and the value under test may sit at
most REF_FACTOR = 4 times the larger of that figure and 1 u from fp64 (another
expf, another division, another summation order).  Where the torch fp32 value
is not finite, the value under test must be the same inf / NaN, and is not
measured.
"""
import functools
import math

import numpy as np
import torch

from oracle import probit_elbo as pe
from tolerances import BATCH_AXIS_REF_FACTOR as REF_FACTOR

U = 2.0 ** -24
SCALE_FLOOR = 2.0 ** -125
F32 = np.float32
L, Z, S = 3, 2, 2
NLL_COEFF, C_COEFF = 0.5, 10.0
PROFILES = ("tame", "wide", "overflow")
MU_KEYS = ("fe_mu", "fe_logvar", "fx_mu", "fx_logvar")
KEYS = ["y", "fe_out", "fe_mu", "fe_logvar", "fx_out", "fx_mu", "fx_logvar"]
# non-unit upstream gradients of total and kl, per objective (fp32 values: the
# fp64 references are given exactly what the kernels are given)
OBJECTIVES = {"total": dict(g_total=0.75), "kl": dict(g_kl=1.375),
              "total+kl": dict(g_total=0.75, g_kl=1.375)}

# ------------------------------------------------------------ path arithmetic
# The constants of the kernels' launches (tests/test_batch_axis_host.py checks
# them against the source text).
K_FINAL_THREADS = 1024        # csrc/probit_fwd.hip kFinalThreads: finalize's one block
K_COEF_THREADS = 512          # csrc/probit_bwd.hip kCoefThreads
K_COEF_KL_BLOCKS = 256        # bwd_coef's KL workgroups: min(cdiv(B d, 512), 256)
K_KL_THREADS, K_KL_BLOCKS = 256, 4096   # csrc/util.hip mpv_kl_bwd's grid cap
K_ROW_THREADS = 256           # bstat_combine / reparam: cdiv(n, 256) blocks


def cdiv(a, b):
    return -(-a // b)


def paths(B, d, aligned=True):
    """Loop passes each kernel makes over (B, d), from the launch constants."""
    n = B * d
    vec = n % 4 == 0 and aligned
    return dict(
        final_b_passes=cdiv(B, K_FINAL_THREADS),
        final_vec=vec,
        final_kl_passes=cdiv(n, K_FINAL_THREADS * (4 if vec else 1)),
        coef_kl_passes=cdiv(n, min(cdiv(n, K_COEF_THREADS), K_COEF_KL_BLOCKS) * K_COEF_THREADS),
        kl_bwd_passes=cdiv(n, min(cdiv(n, K_KL_THREADS), K_KL_BLOCKS) * K_KL_THREADS))


# ----------------------------------------------------------------- generators
def _plant_idx(n, k):
    """k distinct flat indices spread over [0, n): the first and the last
    element among them (the last lies in every loop's final pass)."""
    return np.unique(np.linspace(0, n - 1, k).astype(np.int64)) if n else np.zeros(0, np.int64)


def logvar_pair(rng, B, d, profile):
    """(fe_logvar, fx_logvar) fp32 (B, d) of one profile."""
    n = B * d
    if profile == "wide":
        lve = np.clip(8.0 * rng.standard_normal(n), -30, 30).astype(F32)
        lvx = np.clip(8.0 * rng.standard_normal(n), -30, 30).astype(F32)
        plants = [(30, -30), (-30, 30), (40, -40), (-40, 40), (None, -30), (None, -13.8),
                  (None, 30)]
        idx = _plant_idx(n, len(plants))
        assert len(idx) == len(plants)
        for i, (e, x) in zip(idx, plants):
            if e is not None:
                lve[i] = e
            lvx[i] = x
    else:
        lve = (0.3 * rng.standard_normal(n)).astype(F32)
        lvx = (0.3 * rng.standard_normal(n)).astype(F32)
        if profile == "overflow":
            idx = _plant_idx(n, 5)
            lve[idx], lvx[idx] = 0.0, -100.0
    return lve.reshape(B, d), lvx.reshape(B, d)


@functools.lru_cache(maxsize=None)
def elbo_case(B, d, profile, seed=0):
    """Inputs of one compute_loss call at (B, d), L = 3, z = 2, S = 2: labels
    with y[:, 0] = 1, y[:, 1] = 0 (no degenerate row), row B - 1 with logits
    four times the scale of the others (losing that row moves nll by orders
    more than FWD_RTOL), explicit noise.  Read-only arrays, shared."""
    rng = np.random.default_rng([B, d, PROFILES.index(profile), seed])
    n32 = lambda *s: rng.standard_normal(s).astype(F32)
    y = (rng.random((B, L)) < 0.5).astype(F32)
    y[:, 0], y[:, 1] = 1, 0
    fe_out, fx_out = n32(B, L), n32(B, L)
    fe_out[B - 1] *= 4
    fx_out[B - 1] *= 4
    lve, lvx = logvar_pair(rng, B, d, profile)
    inp = dict(y=y, fe_out=fe_out, fe_mu=n32(B, d), fe_logvar=lve, fx_out=fx_out,
               fx_mu=n32(B, d), fx_logvar=lvx,
               r_sqrt_sigma=rng.uniform(-1, 1, (L, Z)) * np.sqrt(6.0 / (L + Z)),
               noise=n32(S, B, Z))
    for v in inp.values():
        v.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def elbo_ref(B, d, profile, seed=0):
    """oracle.probit_elbo.elbo_forward of elbo_case (computed once)."""
    inp = elbo_case(B, d, profile, seed)
    with np.errstate(over="ignore"):
        return pe.elbo_forward(*[inp[k] for k in KEYS], inp["r_sqrt_sigma"], inp["noise"],
                               NLL_COEFF, C_COEFF)


@functools.lru_cache(maxsize=None)
def elbo_ref_grads(B, d, profile, objective, seed=0):
    inp = elbo_case(B, d, profile, seed)
    return pe.elbo_backward(elbo_ref(B, d, profile, seed), *[inp[k] for k in KEYS], inp["noise"],
                            NLL_COEFF, C_COEFF, **OBJECTIVES[objective])


# -------------------------------------------------------------------- metrics
def same_nonfinite(got, ref32):
    """The NaN positions and the signed inf positions of got equal ref32's."""
    got, ref32 = np.asarray(got, np.float64), np.asarray(ref32, np.float64)
    sinf = lambda a: np.where(np.isinf(a), np.sign(a), 0.0)
    return bool(np.array_equal(np.isnan(got), np.isnan(ref32)) and
                np.array_equal(sinf(got), sinf(ref32)))


def elem_err(got, ref, scale, mask=None):
    """max over the masked elements of |got - ref| / max(scale, 2^-125), in u."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.broadcast_to(np.asarray(scale, np.float64), ref.shape)
    mask = np.ones(ref.shape, bool) if mask is None else mask
    if not mask.any():
        return 0.0
    if not np.isfinite(got[mask]).all():
        return float("inf")
    return float(np.max(np.abs(got[mask] - ref[mask]) / np.maximum(scale[mask], SCALE_FLOOR)) / U)


def within_ref_rule(errs):
    """Every figure k of errs within REF_FACTOR x max(errs[k + '_ref32'], 1 u);
    returns the offenders."""
    return [(k, e, errs[k + "_ref32"]) for k, e in errs.items()
            if not k.endswith("_ref32") and k + "_ref32" in errs
            and not e <= REF_FACTOR * max(errs[k + "_ref32"], 1.0)]


# ------------------------------------------------------------------------- KL
def _g(g_total=0.0, g_kl=0.0):
    return g_kl + pe.KL_WEIGHT * g_total


def kl_grads_f32(inp, g_total=0.0, g_kl=0.0):
    """oracle.probit_elbo.kl_backward's formulas in torch CPU fp32."""
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    mue, lve, mux, lvx = (torch.from_numpy(np.array(inp[k], F32)) for k in MU_KEYS)
    s = t(0.5) * (t(g_kl) + t(pe.KL_WEIGHT) * t(g_total)) / t(float(mue.shape[0]))
    ex = torch.exp(lvx)
    den = ex + t(pe.KL_EPS)
    d = mux - mue
    r = torch.exp(lve - lvx)
    out = dict(fe_mu=s * (-2.0 * d / den), fx_mu=s * (2.0 * d / den), fe_logvar=s * (-1.0 + r),
               fx_logvar=s * (1.0 - r - d * d * ex / den ** 2))
    return {k: v.numpy() for k, v in out.items()}


def kl_grad_scales(inp, ref, g):
    mue, lve, mux, lvx = (np.asarray(inp[k], np.float64) for k in MU_KEYS)
    a = abs(0.5 * g / mue.shape[0])
    dm, ex, delta = mux - mue, np.exp(lvx), lve - lvx
    r = np.exp(delta)
    q = dm * dm * ex / (ex + pe.KL_EPS) ** 2
    lvt = a * (1.0 + r * (1.0 + np.abs(delta)))
    return dict(fe_mu=np.abs(ref["fe_mu"]) * (1.0 + np.abs(lvx)),
                fx_mu=np.abs(ref["fx_mu"]) * (1.0 + np.abs(lvx)),
                fe_logvar=lvt, fx_logvar=lvt + a * q * (1.0 + np.abs(lvx)))


def kl_grad_errs(got, inp, g_total=0.0, g_kl=0.0):
    """got: the four KL gradients by MU_KEYS name.  Asserts the torch-fp32
    inf / NaN pattern; returns the elementwise errors (u) of got and of the
    torch-fp32 evaluation ('<key>_ref32') over the elements finite in fp32."""
    g = _g(g_total, g_kl)
    ref = pe.kl_backward(*[inp[k] for k in MU_KEYS], g)
    ref32 = kl_grads_f32(inp, g_total, g_kl)
    scales = kl_grad_scales(inp, ref, g)
    errs = {}
    for k in MU_KEYS:
        assert same_nonfinite(got[k], ref32[k]), (k, "inf / NaN pattern differs from fp32")
        fin = np.isfinite(ref32[k])
        errs[k] = elem_err(got[k], ref[k], scales[k], fin)
        errs[k + "_ref32"] = elem_err(ref32[k], ref[k], scales[k], fin)
    return errs


def kl_scalar_f32(inp):
    """The reference's own KL expression in torch CPU fp32."""
    fe_mu, fe_logvar, fx_mu, fx_logvar = (torch.from_numpy(np.array(inp[k], F32)) for k in MU_KEYS)
    return float(torch.mean(0.5 * torch.sum((fx_logvar - fe_logvar) - 1 + torch.exp(
        fe_logvar - fx_logvar) + torch.square(fx_mu - fe_mu) / (torch.exp(fx_logvar) + 1e-6), dim=1)))


def kl_scalar_errs(got, inp):
    """{'kl', 'kl_ref32'}: |kl - fp64| over 0.5 / B * sum |addends|, in u; where
    fp32 overflows, got must be that same inf (both figures then 0)."""
    mue, lve, mux, lvx = (np.asarray(inp[k], np.float64) for k in MU_KEYS)
    ref32 = kl_scalar_f32(inp)
    if not math.isfinite(ref32):
        assert float(got) == ref32, (float(got), ref32)
        return dict(kl=0.0, kl_ref32=0.0)
    ref = pe.kl_term(mue, lve, mux, lvx)
    absum = (np.abs(lvx - lve) + 1.0 + np.exp(lve - lvx) +
             (mux - mue) ** 2 / (np.exp(lvx) + pe.KL_EPS)).sum()
    scale = 0.5 / mue.shape[0] * absum
    return dict(kl=elem_err(float(got), ref, scale), kl_ref32=elem_err(ref32, ref, scale))


# ---------------------------------------------------------- cross-shard combine
BSTAT_R, BSTAT_B = (1, 2, 8), (1, 255, 257, 1025)
BSTAT_KINDS = ("near", "far", "tie")


def bstat_case(R, B, kind, seed=0):
    """Gathered per-shard statistics (R, 6, B) fp32 = [m_e, Z_e, m_x, Z_x,
    csum_e, csum_x] per shard.  Maxima: 'near' within 1 of each other; 'far'
    200 apart (fp32 and fp64 exp(-200 k) is 0 or 1e-87: the shard holding the
    maximum, another one on every row, alone decides Z); 'tie' shard 0 holds
    the maximum of every row, shard 1 ties with it on the even rows."""
    rng = np.random.default_rng([R, B, BSTAT_KINDS.index(kind), seed])
    base = -20.0 + 5.0 * rng.standard_normal((2, 1, B))
    r, b = np.arange(R)[:, None], np.arange(B)[None, :]
    if kind == "near":
        off = -rng.random((2, R, B))
    elif kind == "far":
        off = -200.0 * np.stack([(r + b) % R, (r + b + 1) % R])
    else:
        off = -3.0 * rng.random((2, R, B)) - 1e-3
        off[:, 0] = 0.0
        if R > 1:
            off[:, 1, ::2] = 0.0
    m = (base + off).astype(F32)
    g = np.empty((R, 6, B), F32)
    g[:, 0], g[:, 2] = m[0], m[1]
    g[:, 1], g[:, 3] = rng.uniform(0.5, 4.0, (R, B)), rng.uniform(0.5, 4.0, (R, B))
    g[:, 4], g[:, 5] = rng.uniform(0.0, 2.0, (R, B)), rng.uniform(0.0, 2.0, (R, B))
    return g


def bstat_errs(got, g):
    """got (6, B) against oracle.probit_elbo.combine_bstats of g (R, 6, B).
    Asserts M exact and the ranking sums within R u of sum |terms|; returns the
    errors of Z (relative to sum Z_r e^(m_r - M), all terms positive) of got
    and of the torch-fp32 evaluation, and of the sums (in u)."""
    got = np.asarray(got, np.float64)
    R = g.shape[0]
    ref = pe.combine_bstats([g[r].astype(np.float64) for r in range(R)])
    t = torch.from_numpy(g)
    errs = {}
    for tag, mi, zi in (("e", 0, 1), ("x", 2, 3)):
        assert np.array_equal(got[mi], ref[mi]), ("M_" + tag, "not exact")
        M32 = t[:, mi].max(0).values
        Z32 = (t[:, zi] * torch.exp(t[:, mi] - M32)).sum(0).numpy()
        errs["Z_" + tag] = elem_err(got[zi], ref[zi], ref[zi])
        errs["Z_" + tag + "_ref32"] = elem_err(Z32, ref[zi], ref[zi])
    absum = np.abs(g[:, 4:].astype(np.float64)).sum(0)
    errs["csum"] = elem_err(got[4:], ref[4:], absum)
    assert errs["csum"] <= R, ("ranking sums", errs["csum"], R)
    return errs


def finalize_inputs(B, d=4, seed=0):
    """colsum (2, B, L) and the four mu / logvar (B, d) for a finalize call."""
    rng = np.random.default_rng([B, d, seed, 77])
    colsum = rng.uniform(0.0, S, (2, B, L)).astype(F32)
    lve, lvx = logvar_pair(rng, B, d, "tame")
    mus = dict(fe_mu=rng.standard_normal((B, d)).astype(F32), fe_logvar=lve,
               fx_mu=rng.standard_normal((B, d)).astype(F32), fx_logvar=lvx)
    return colsum, mus


# ------------------------------------------------------------ reparameterisation
REPARAM_SHAPES = [((128, 50), (128, 50)),   # the product's own shape
                  ((1, 257), (3, 100)),     # block 1 straddles both encoders
                  ((7, 1), (1025, 3)),      # n_e < one block, n_x over 13 blocks
                  ((5, 50), (0, 50)), ((0, 50), (5, 50))]
REPARAM_OUTS = ("z_e", "z_x", "mu_e", "lv_e", "mu_x", "lv_x")


def logvar_single(rng, shape, profile):
    n = int(np.prod(shape))
    if profile == "wide":
        lv = np.clip(8.0 * rng.standard_normal(n), -30, 30).astype(F32)
        idx = _plant_idx(n, 2)
        lv[idx] = np.array([-30.0, 30.0], F32)[:len(idx)]
    else:
        lv = (0.3 * rng.standard_normal(n)).astype(F32)
    return lv.reshape(shape)


def reparam_case(shape_e, shape_x, profile, seed=0):
    """mu, lv, eps of both encoders, an upstream gradient for each of the six
    outputs ('g_<out>').  'overflow': lv = +200 at the first two elements of an
    encoder (exp(100) = inf in fp32), eps == 0 at the first (0 inf = NaN), and
    lv = -200 at the last (exp(-100): an fp32 subnormal)."""
    rng = np.random.default_rng([*shape_e, *shape_x, PROFILES.index(profile), seed, 5])
    c = {}
    for e, shape in (("e", shape_e), ("x", shape_x)):
        n = int(np.prod(shape))
        mu = rng.standard_normal(shape).astype(F32)
        lv = logvar_single(rng, shape, profile)
        eps = rng.standard_normal(shape).astype(F32)
        if profile == "overflow" and n >= 3:
            lv.reshape(-1)[[0, 1, n - 1]] = (200.0, 200.0, -200.0)
            eps.reshape(-1)[0] = 0.0
        c.update({"mu_" + e: mu, "lv_" + e: lv, "eps_" + e: eps})
        for k in ("z_", "mu_", "lv_"):
            c["g_" + k + e] = rng.standard_normal(shape).astype(F32)
    return c


def reparam_fwd_ref(mu, lv, eps):
    mu, lv, eps = (np.asarray(a, np.float64) for a in (mu, lv, eps))
    z = mu + eps * np.exp(lv / 2)
    return z, np.abs(mu) + np.abs(eps) * np.exp(lv / 2)          # value, scale


def reparam_fwd_f32(mu, lv, eps):
    mu, lv, eps = (torch.from_numpy(np.array(a, F32)) for a in (mu, lv, eps))
    return (mu + eps * torch.exp(0.5 * lv)).numpy()


def reparam_bwd_ref(gz, lv, eps, add_mu, add_lv):
    """(gmu, glv, scale of gmu, scale of glv) in fp64; gz / add_* None: no
    gradient arrives there (gz counts as 0)."""
    lv, eps = np.asarray(lv, np.float64), np.asarray(eps, np.float64)
    z0 = np.zeros(lv.shape)
    gz, add_mu, add_lv = (z0 if a is None else np.asarray(a, np.float64)
                          for a in (gz, add_mu, add_lv))
    t = 0.5 * np.exp(lv / 2)
    return (gz + add_mu, gz * eps * t + add_lv, np.abs(gz) + np.abs(add_mu),
            np.abs(gz * eps) * t + np.abs(add_lv))


def reparam_bwd_f32(gz, lv, eps, add_mu, add_lv):
    lv, eps = torch.from_numpy(np.array(lv, F32)), torch.from_numpy(np.array(eps, F32))
    tt = lambda a: None if a is None else torch.from_numpy(np.array(a, F32))
    gz, add_mu, add_lv = tt(gz), tt(add_mu), tt(add_lv)
    g = torch.zeros_like(lv) if gz is None else gz
    gmu = g if add_mu is None else g + add_mu
    glv = g * eps * 0.5 * torch.exp(0.5 * lv)
    glv = glv if add_lv is None else glv + add_lv
    return gmu.numpy(), glv.numpy()


def reparam_errs(got, ref, scale, ref32, name, errs):
    """Pattern against torch fp32 asserted; the errors of got and of torch fp32
    over the elements finite in fp32 are max-folded into errs[name(+_ref32)]."""
    assert same_nonfinite(got, ref32), (name, "inf / NaN pattern differs from fp32")
    fin = np.isfinite(ref32)
    errs[name] = max(errs.get(name, 0.0), elem_err(got, ref, scale, fin))
    errs[name + "_ref32"] = max(errs.get(name + "_ref32", 0.0), elem_err(ref32, ref, scale, fin))
