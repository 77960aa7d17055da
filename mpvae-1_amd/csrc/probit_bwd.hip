// Backward of the MPVAE probit ELBO for one S-shard: the gradients PyTorch
// autograd takes through reference mpvae.py:165-210, written out analytically.
//
//   bwd_coef_kernel  per (s,b): alpha = -g_nll * softmax_s(logp)/B and the
//                    ranking coefficients betaP = g_c N/(n S B), betaN = g_c P/(n S B)
//                    (NaN for a degenerate row whose ranking term is live,
//                    reproducing the 0/0 of mpvae.py:118 under autograd); per
//                    batch row also an upper bound of |G| (3xf16 scale).
//   bwd_elem_kernel  streams T once: recomputes E, E_x, forms
//                    dE = alpha (y/E - (1-y)/(1-E)) - [y=1] betaP e^{-5E}
//                         + [y=0] betaN e^{5E} + g_indiv/S,
//                    du = dE (1-1e-6) phi(u); column sums over s give d fe_out /
//                    d fx_out; writes G = du + du_x (fp32 over T, or 3xf16 planes).
//                    bwd_elem_ring_kernel is the same pass through a per-wave
//                    LDS ring (planes, more than 512 columns).  Shared:
//                    elem_coef_load, d_elem2x4, poison_row, elem_colsum_store.
//   dR16_kernel,     dR[l][k] = sum_{s,b} G[s,b,l] eps[s,b,k], 3xf16 operands on
//   dR16s_kernel     the f16 matrix cores; the rows (the K axis) are the LDS
//                    rows, fragments come from ds_read_b64_tr_b16 transposed
//                    reads; split-K over the S*B rows into slabs reduced in a
//                    fixed order (deterministic).  dR16_kernel takes the 64 and
//                    128 tiles (L, z <= 64 / <= 128), dR16s_kernel, two wave
//                    groups one phase apart, the 256 tile.
//   dR_gemm_kernel   the same on exact fp32 MFMA (MPV_GEMM_F32), 128 tile.
//                    Shared by the three: Dr16Tile (geometry), dr_ctx (what a
//                    workgroup and its lanes own), dr_mfma on a DrFrag (3xf16)
//                    filled by dr_read (dR16_kernel) or, from constant per-lane
//                    bases, by drs_read (dR16s_kernel: DrsAddr), dr_store_slab.
// Host: pick_dr_tile chooses the DrTile descriptor (edge, split-K target,
// threads, kernel); plan_bwd derives the grids and the workspace layout from it.
#include <type_traits>

#include "abi_util.h"
#include "mpv_common.h"


namespace mpv {

// Upper bounds used for the G scale (3xf16): for E = Phi(u)(1-1e-6)+0.5e-6,
// sup_u phi(u) |y/E - (1-y)/(1-E)| < 4.5 (inverse Mills ratio capped by the
// 0.5e-6 floor), phi(u) e^{-5E} <= 0.4, phi(u) e^{5E} <= 0.4 e^5 < 60.  Only the
// order of magnitude matters: the split keeps full precision for anything
// within 2^10 of the bound.
constexpr float kBoundDl = 4.5f, kBoundPos = 0.4f, kBoundNeg = 60.0f, kBoundInd = 0.4f;

// --------------------------------------------------------------- coefficients
// bwd_coef: one workgroup per batch row of 512 threads (1024: C2 +1.3 us, C3
// +-0, round 6; 256: C2 +1.7, C3 +2, C4 +3 us against 512, round 3)
constexpr int kCoefThreads = 512;

__global__ __launch_bounds__(kCoefThreads) void bwd_coef_kernel(
    const float* __restrict__ y, const float* __restrict__ rowstat, const float* __restrict__ bstat,
    const float* __restrict__ gscal, const float* __restrict__ gI, const float* __restrict__ gIL,
    float* __restrict__ coef, float* __restrict__ gbound, int S, int B, int L, float S_total,
    float nll_coeff, float c_coeff, int live, mpv_kl_bwd_args kl, int kl_blocks) {
  __shared__ float red[48];
  if ((int)blockIdx.x >= B) {  // the extra workgroups: the KL backward (mpv_bwd_args.kl)
    kl_bwd_range(kl, (int64_t)(blockIdx.x - B) * blockDim.x + threadIdx.x,
                 (int64_t)kl_blocks * blockDim.x);
    return;
  }
  const int b = blockIdx.x, tid = threadIdx.x;
  float np = 0.f, nn = 0.f, gi = 0.f;
  for (int l = tid; l < L; l += blockDim.x) {
    const int64_t o = (int64_t)b * L + l;
    const float v = y[o];
    np += (v == 1.0f) ? 1.0f : 0.0f;
    nn += (v == 0.0f) ? 1.0f : 0.0f;
    gi = fmaxf(gi, (gI ? fabsf(gI[o]) : 0.0f) + (gIL ? fabsf(gIL[o]) : 0.0f));
  }
  {  // the two counts and the max with one barrier pair (block_reduce's orders)
    const int lane = tid & 63, wid = tid >> 6, nw = (blockDim.x + 63) >> 6;
    np = wave_sum(np);
    nn = wave_sum(nn);
    gi = wave_max(gi);
    __syncthreads();
    if (lane == 0) red[wid] = np, red[16 + wid] = nn, red[32 + wid] = gi;
    __syncthreads();
    np = nn = 0.0f;
    gi = -INFINITY;
    for (int i = 0; i < nw; ++i) {
      np += red[i];
      nn += red[16 + i];
      gi = fmaxf(gi, red[32 + i]);
    }
  }
  const float nrm = np * nn;
  // only live slots are read (gscal may hold just the TOTAL slot)
  auto gs = [&](int k) { return (live & MPV_LIVE(k)) ? gscal[k] : 0.0f; };
  const float gt = gs(MPV_G_TOTAL);
  const float gn[2] = {gs(MPV_G_NLL) + nll_coeff * gt, gs(MPV_G_NLL_X) + nll_coeff * gt};
  const float gc[2] = {gs(MPV_G_C) + c_coeff * gt, gs(MPV_G_C_X) + c_coeff * gt};
  const bool clive[2] = {(live & (MPV_LIVE(MPV_G_TOTAL) | MPV_LIVE(MPV_G_C))) != 0,
                         (live & (MPV_LIVE(MPV_G_TOTAL) | MPV_LIVE(MPV_G_C_X))) != 0};
  const float inv_B = 1.0f / (float)B;
  float bound = kBoundInd * gi / S_total;
  float bmaxb[2];
#pragma unroll
  for (int br = 0; br < 2; ++br) {
    const float M = bstat[(2 * br) * B + b], Z = bstat[(2 * br + 1) * B + b];
    const bool dead = !(nrm > 0.0f) && clive[br];
    const float cs = gc[br] / (nrm * S_total * (float)B);
    float bmax = 0.0f;
    // one sample's coefficients (stored times dE/du's constant kPhiK: the
    // element pass then multiplies by exp(-u^2/2) alone)
    auto one = [&](float lp, float P, float N, float& ca, float& cp, float& cn) {
      float alpha = -gn[br] * (expf(lp - M) / Z) * inv_B;
      float bP = nrm > 0.0f ? cs * N : 0.0f;
      float bN = nrm > 0.0f ? cs * P : 0.0f;
      bmax = fmaxf(bmax, kBoundDl * fabsf(alpha) + kBoundPos * fabsf(bP) + kBoundNeg * fabsf(bN));
      if (dead) alpha = bP = bN = __builtin_nanf("");
      ca = alpha * kPhiK;
      cp = bP * kPhiK;
      cn = bN * kPhiK;
    };
    const float* rl = rowstat + ((int64_t)br * B + b) * S;
    const float* rp = rowstat + ((int64_t)(2 + 2 * br) * B + b) * S;
    const float* rn = rowstat + ((int64_t)(3 + 2 * br) * B + b) * S;
    float* ca = coef + ((int64_t)(3 * br + 0) * B + b) * S;
    float* cp = coef + ((int64_t)(3 * br + 1) * B + b) * S;
    float* cn = coef + ((int64_t)(3 * br + 2) * B + b) * S;
    if ((S & 3) == 0) {  // four consecutive samples per thread, 16-B accesses (same values)
      for (int s = 4 * tid; s < S; s += 4 * (int)blockDim.x) {
        const f32x4 lp = *reinterpret_cast<const f32x4*>(rl + s);
        const f32x4 P = *reinterpret_cast<const f32x4*>(rp + s);
        const f32x4 N = *reinterpret_cast<const f32x4*>(rn + s);
        float a[4], p[4], n[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) one(lp[j], P[j], N[j], a[j], p[j], n[j]);
        *reinterpret_cast<f32x4*>(ca + s) = f32x4{a[0], a[1], a[2], a[3]};
        *reinterpret_cast<f32x4*>(cp + s) = f32x4{p[0], p[1], p[2], p[3]};
        *reinterpret_cast<f32x4*>(cn + s) = f32x4{n[0], n[1], n[2], n[3]};
      }
    } else {
      for (int s = tid; s < S; s += blockDim.x) one(rl[s], rp[s], rn[s], ca[s], cp[s], cn[s]);
    }
    bmaxb[br] = bmax;
  }
  block_reduce2<true>(bmaxb[0], bmaxb[1], red);
  bound += bmaxb[0];
  bound += bmaxb[1];
  if (tid == 0 && gbound) gbound[b] = bound;
}

// ------------------------------------------------------------ element pass
struct ElemParams {
  const float* y;
  const float* fe;
  const float* fx;
  const float* gI;   // (B,L) grad of indiv_prob (feature branch) or NULL
  const float* gIL;  // (B,L) grad of indiv_prob_label (label branch) or NULL
  const float* coef;
  float* T;          // (B*S, ldT)
  uint16_t* g;       // chunked 3xf16 output planes (B*S rows of gld halves), or NULL: fp32 G over T
  const float* g_bound;  // (B) per-row bounds of |G|: the planes' scale (wave_pow2_scale)
  int64_t gld;
  float* colpart;  // [nSc][2][B][L]
  int S, B, L, Lc;  // Lc: columns covered (L rounded up to 4 for planes: pads get G = 0)
  int ldT;          // t_cols(L)
  int TPR, RPI, rows_per_chunk;
  float inv_S;
};

// dL/dt of one element for the label (.x) and feature (.y) branches at once
// (packed fp32): u = t + base, E = probit(u),
//   dE = alpha (y/E - (1-y)/(1-E)) + [y=1](-betaP) e^{-5E} + [y=0] betaN e^{5E} + g_ind
// (mpvae.py:110-117, 184-185 differentiated), dL/dt = dE (1-1e-6) phi(u).
// Per-column constants of the element pass (the lane's four label columns).
struct ElemCol {
  f32x2 base[4];  // fe_out, fx_out, in the probit's argument units (x kZq)
  f32x2 gind[4];  // g(indiv_prob_label), g(indiv_prob), / S_total, x kPhiK
  float y[4];
  bool soft[4];
  float qm[4];  // d = E + qm: E - 1 for y = 0 (the sign of d logp/dE folded in), E otherwise
  float sga[4];   // e^{-5E} (y = 1) or e^{5E} as exp2(sga w) e^{-+5 C0}
  float wp[4], wn[4];  // [y = 1], [y = 0] (1 or 0)
  bool pos[4];         // y = 1
  float kp, kn;        // e^{-5 C0}, e^{5 C0}: the row's ranking coefficients
                       // rkp = kp (-bP), rkn = kn bN carry them
};

// A degenerate row poisons every label, whatever its value (reference
// autograd); rkp is NaN exactly when betaP is.
MPV_DEV void poison_row(f32x2 (&out)[4], f32x2 rkp) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (rkp.x != rkp.x) out[q].x = rkp.x;
    if (rkp.y != rkp.y) out[q].y = rkp.y;
  }
}

// Four elements (columns) of one row at once, step-major so that the
// dependent packed ops of one element interleave with the others'.
// SOFT: the block may hold soft (non 0/1) labels (a per-column branch; false:
// no branch at all, so the four columns' chains interleave in one basic
// block).  NANCHK: poison the row here when bP is NaN (false: the caller does
// it with a wave-uniform test).  SOFT_RCP: a soft label's y/E - (1-y)/(1-E)
// by hardware reciprocals (1 ulp) instead of IEEE divisions, whose
// registers would spill the LDS-ring kernel.
// rkp, rkn: the row's ranking coefficients of a positive / negative label,
// kp (-betaP) and kn betaN (a binary block picks one per column instead of
// forming wn rkn + wp rkp; elem_rank_coefs).
// rkq: the four columns' ranking coefficients already picked (the LDS-ring
// loop reads each from its own address), or null.
template <bool SOFT = true, bool NANCHK = true, bool SOFT_RCP = false>
MPV_DEV void d_elem2x4(const float (&t)[4], const ElemCol& c, f32x2 alpha, f32x2 rkp, f32x2 rkn,
                       f32x2 (&out)[4], const f32x2* rkq = nullptr, const f32x2* qc1 = nullptr) {
  f32x2 zq[4], w[4], ez[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) zq[q] = pk_fma(splat2(t[q]), splat2(kZq), c.base[q]);
  probit_dw2xN_zq<4>(zq, w, ez, qc1);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    // E in the reference's rounding order (mpvae.py:171-180: cdf = 0.5 (1 +
    // erf) exact from w = 1 + erf, then cdf (1 - eps1) and + eps1/2 each
    // rounded in fp32), so that near E -> 1, where one fp32 ulp of E is ~6 %
    // of 1 - E and 1/(1 - E) weights the gradient, E is the reference's E
    // bit for bit whenever w is (a single fma(w, kEh, C0) rounds once and
    // moved such gradients by ~1e-3: DESIGN.md section 4, "Full C4")
    f32x2 E;
    {
#pragma clang fp contract(off)
      E = w[q] * kEh + splat2(kC0);
    }
    // d logp / dE = y/E - (1-y)/(1-E): one reciprocal of E (y = 1) or of
    // E - 1 (y = 0, the sign folded in; exact for E >= 0.5)
    const f32x2 d = E + splat2(c.qm[q]);
    const f32x2 r = f32x2{fast_rcp(d.x), fast_rcp(d.y)};
    f32x2 dE;
    if (SOFT && c.soft[q]) {
      const f32x2 omE = splat2(1.0f) - E;
      const f32x2 dl = SOFT_RCP ? splat2(c.y[q]) * f32x2{fast_rcp(E.x), fast_rcp(E.y)} -
                                      splat2(1.0f - c.y[q]) * f32x2{fast_rcp(omE.x), fast_rcp(omE.y)}
                                : splat2(c.y[q]) / E - splat2(1.0f - c.y[q]) / omE;
      dE = pk_fma(alpha, dl, c.gind[q]);
    } else {
      dE = pk_fma(alpha, r, c.gind[q]);
    }
    // ranking term: pos -> -betaP e^{-5E}, neg -> +betaN e^{5E}
    const f32x2 rk = rkq   ? rkq[q]
                     : SOFT ? pk_fma(splat2(c.wn[q]), rkn, splat2(c.wp[q]) * rkp)
                            : (c.pos[q] ? rkp : rkn);
    const f32x2 a = w[q] * c.sga[q];
    dE = pk_fma(rk, f32x2{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)}, dE);
    out[q] = dE * ez[q];  // the coefficients carry kPhiK
  }
  if (NANCHK && (rkp.x != rkp.x || rkp.y != rkp.y)) poison_row(out, rkp);
}

// The ranking coefficients of one row from its betaP, betaN (label, feature).
MPV_DEV void elem_rank_coefs(const ElemCol& c, f32x2 bP, f32x2 bN, f32x2& rkp, f32x2& rkn) {
  rkp = splat2(c.kp) * -bP;
  rkn = splat2(c.kn) * bN;
}

// Inputs of one row s of the element pass: its six coefficients (label .x,
// feature .y) and the lane's four t values.
struct ElemRow {
  f32x2 alpha, bP, bN;
  float t[4];
};

// The six coefficients of sample row o = b*S + s (coef is [k][b][s]) as
// (label, feature) pairs.
MPV_DEV void elem_coef_load(const ElemParams& p, int64_t o, f32x2& alpha, f32x2& bP, f32x2& bN) {
  const int64_t BS = (int64_t)p.B * p.S;
  alpha = f32x2{p.coef[0 * BS + o], p.coef[3 * BS + o]};
  bP = f32x2{p.coef[1 * BS + o], p.coef[4 * BS + o]};
  bN = f32x2{p.coef[2 * BS + o], p.coef[5 * BS + o]};
}

MPV_DEV void elem_row_load(ElemRow& r, const ElemParams& p, int b, int s, int c0,
                           const bool (&ok)[4]) {
  const int64_t cb = (int64_t)b * p.S + s;
  elem_coef_load(p, cb, r.alpha, r.bP, r.bN);
  const float* row = p.T + cb * p.ldT;
  if (c0 < p.L) {  // t_cols rows: the pad columns are readable
    // nontemporal T loads and G-plane stores: element pass -5 %
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row + c0));
    r.t[0] = v[0]; r.t[1] = v[1]; r.t[2] = v[2]; r.t[3] = v[3];
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) r.t[q] = ok[q] ? row[c0 + q] : 0.0f;
  }
}

// The lane's four label columns c0 .. c0+3 of batch row b: validity and the
// per-column constants of the element math (ElemCol).
MPV_DEV void elem_col_setup(const ElemParams& p, int b, int c0, bool active, bool (&ok)[4],
                            ElemCol& ec) {
  const int L = p.L;
  ec.kp = exp2f((-5.0f * 1.4426950408889634f) * kC0);
  ec.kn = exp2f((5.0f * 1.4426950408889634f) * kC0);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = c0 + q;
    ok[q] = active && c < L;
    const int64_t o = (int64_t)b * L + (ok[q] ? c : 0);
    const float yv = ok[q] ? p.y[o] : 0.0f;
    const float fe = ok[q] ? p.fe[o] : 0.0f;
    const float fx = ok[q] ? p.fx[o] : 0.0f;
    const float gi = (ok[q] && p.gI) ? p.gI[o] * p.inv_S : 0.0f;
    const float gil = (ok[q] && p.gIL) ? p.gIL[o] * p.inv_S : 0.0f;
    ec.base[q] = f32x2{fe, fx} * kZq;
    ec.gind[q] = f32x2{gil, gi} * kPhiK;
    ec.y[q] = yv;
    ec.soft[q] = !(yv == 0.0f || yv == 1.0f);
    ec.qm[q] = yv == 0.0f ? -1.0f : 0.0f;  // E - 1 = -(1 - E), or E
    const float sgx = (yv == 1.0f ? -5.0f : 5.0f) * 1.4426950408889634f;
    ec.sga[q] = sgx * kEh;
    // the constant factor e^{-+5 C0} of e^{-+5E} rides on the label weights
    ec.wp[q] = yv == 1.0f ? 1.0f : 0.0f;
    ec.wn[q] = yv == 0.0f ? 1.0f : 0.0f;
    ec.pos[q] = yv == 1.0f;
  }
}

// Column sums of a block's rows -> colpart[sc][2][b][.]: every thread stages
// its sg2 into cred (256 x 8 floats of LDS, free by now), then each of the
// block's 4 TPR columns adds its RPI row-lanes in a fixed order.
MPV_DEV void elem_colsum_store(const ElemParams& p, const f32x2 (&sg2)[4], float* cred, int TPR,
                               int RPI) {
  const int b = blockIdx.x, sc = blockIdx.y, tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    cred[tid * 8 + q] = sg2[q].x;
    cred[tid * 8 + 4 + q] = sg2[q].y;
  }
  __syncthreads();
  for (int j = tid; j < TPR * 4; j += blockDim.x) {
    const int cqq = j >> 2, q = j & 3;
    const int c = blockIdx.z * 1024 + j;
    if (c < p.L) {
      float e = 0.f, x = 0.f;
      for (int r = 0; r < RPI; ++r) {
        e += cred[(r * TPR + cqq) * 8 + q];
        x += cred[(r * TPR + cqq) * 8 + 4 + q];
      }
      p.colpart[(((int64_t)sc * 2 + 0) * p.B + b) * p.L + c] = e;
      p.colpart[(((int64_t)sc * 2 + 1) * p.B + b) * p.L + c] = x;
    }
  }
}

// Rows of T in flight per thread beyond the one computing (kElemLookahead).
// The row index and the six per-row coefficients are per-lane (a block row
// holds RPI rows of TPR threads), 12 more VGPRs than fit in 128: the kernel
// runs at 3 waves per SIMD instead of spilling (4 waves per SIMD: slower,
// profiles/r06_elem_occ4_ab.json).
constexpr int kElemLookahead = 1;  // 2, 3: C3 element pass 0.111 -> 0.120 ms (r06_la_ab.json)
constexpr int kElemMinRows = 16;   // minimum T rows per thread (C2 -6 %)
template <bool PLANES>
__global__ __launch_bounds__(256, 3) void bwd_elem_kernel(ElemParams p) {
  constexpr int LA = kElemLookahead;
  __shared__ float cred[256 * 8];
  const int b = blockIdx.x, sc = blockIdx.y;
  const int tid = threadIdx.x;
  const int rsub = tid / p.TPR, cq = tid % p.TPR;
  const bool active = rsub < p.RPI;
  const int c0 = blockIdx.z * 1024 + cq * 4;
  const int S = p.S, L = p.L;
  const float gs = PLANES ? wave_pow2_scale(p.g_bound, p.B) : 1.0f;

  bool ok[4];
  ElemCol ec;
  elem_col_setup(p, b, c0, active, ok, ec);
  f32x2 sg2[4] = {splat2(0.f), splat2(0.f), splat2(0.f), splat2(0.f)};  // (label, feature)
  const int s_begin = sc * p.rows_per_chunk;
  const int s_end = min(S, s_begin + p.rows_per_chunk);
  if (active && c0 < p.Lc) {
    // LA rows of lookahead: rows s+RPI .. s+LA*RPI are in flight while row s
    // computes (the element math and the T stream overlap)
    const int s0 = s_begin + rsub, R = p.RPI;
    ElemRow buf[LA + 1];
#pragma unroll
    for (int j = 0; j < LA; ++j)
      if (s0 + j * R < s_end) elem_row_load(buf[j], p, b, s0 + j * R, c0, ok);
    for (int s = s0; s < s_end; s += R) {
      if (s + LA * R < s_end) elem_row_load(buf[LA], p, b, s + LA * R, c0, ok);
      const ElemRow& cur = buf[0];
      const int64_t cb = (int64_t)b * S + s;
      float G[4];
      f32x2 g2[4];
      f32x2 rkp, rkn;
      elem_rank_coefs(ec, cur.bP, cur.bN, rkp, rkn);
      d_elem2x4(cur.t, ec, cur.alpha, rkp, rkn, g2);
      // column sums: pad columns (finite, never published) need no mask
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sg2[q] = sg2[q] + g2[q];
        G[q] = ok[q] ? g2[q].x + g2[q].y : 0.0f;
      }
      if (PLANES) {
        // (split2_f16 / add_f32 here, as in elem_ring_rows: C3 element pass
        // +4 %, the per-column branches leave the asm blocks unscheduled)
        uint16_t h[4], l[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) split_f16(G[q], gs, h[q], l[q]);
        // rows b*S + s (the noise planes' row order), chunked like mpv_split16
        const int64_t o = chunked_index(cb, p.gld, c0);
        const s16x4 hv{(short)h[0], (short)h[1], (short)h[2], (short)h[3]};
        const s16x4 lv{(short)l[0], (short)l[1], (short)l[2], (short)l[3]};
        __builtin_nontemporal_store(hv, reinterpret_cast<s16x4*>(p.g + o));
        __builtin_nontemporal_store(lv, reinterpret_cast<s16x4*>(p.g + o + kLoOff));
      } else {
        float* row = p.T + cb * p.ldT;
        if (c0 < L) {  // pad columns get G = 0
          *reinterpret_cast<f32x4*>(row + c0) = f32x4{G[0], G[1], G[2], G[3]};
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (ok[q]) row[c0 + q] = G[q];
        }
      }
#pragma unroll
      for (int j = 0; j < LA; ++j) buf[j] = buf[j + 1];
    }
  }
  elem_colsum_store(p, sg2, cred, p.TPR, p.RPI);
}

// The element pass for 3xf16 planes when one thread row of a block covers a
// whole label row (plan_bwd: TPR = cdiv(Lc, 4), so Lc > 512: C4, C5 and any
// 512 < L < 1024, whose surplus waves are masked).  T rows stream through a per-wave LDS ring by LDS-DMA
// (global_load_lds_dwordx4: a wave moves the 1 KB of a row its own 256
// columns need, so no wave reads another's slot and the ring needs no
// barrier); the row's six coefficients come from an LDS copy of the block's
// chunk.  The loop then issues no register load that hipcc must wait for --
// its only vector-memory ops are the DMA (counted here, lds_dma16) and the two
// G-plane stores per row -- and with SOFT false it has no divergent branch,
// so the four columns' element math interleaves in one basic block.  (The
// register-lookahead kernel above serialises each column's dependent packed
// ops behind s_nop: its per-column soft-label branches split the row into
// basic blocks the scheduler cannot interleave across, and without them hipcc
// drains its lookahead loads every row: DESIGN.md section 3.)
constexpr int kElemRing = 8;       // T rows in flight per wave (1 KB each; 8: 3 waves per SIMD)
constexpr int kElemRingRows = 256;  // rows per sub-chunk (the coefficient copy)
constexpr int kElemRingMinRows = 128;  // rows per block at least (plan_bwd; 64: +0.3 % at S 512)
// The rows of one sub-chunk [sb, sb + nrows) for one wave; SOFT: the block
// holds soft labels (block-uniform, so either loop is one basic block).
// MASK: some lane of the wave has columns past L or past the planes (their G is
// zeroed, their stores skipped).  NANCHK: some row of the sub-chunk is
// degenerate (its NaN poisons every label of that row).  The loop is bound by
// VALU issue (~95 % busy at C4, profiles/r05_elem_valu_pmc.json), so the row
// sums and the f16 split are one instruction each (asm: hipcc's SLP
// vectoriser otherwise packs the sums through register moves and splits by
// convert / convert back / subtract), the coefficients sit in LDS as the
// (label, feature) pairs the packed math takes, and the checks that do not
// apply to a wave or a sub-chunk are compiled out.
template <bool SOFT, bool MASK, bool NANCHK>
MPV_DEV void elem_ring_rows(const ElemParams& p, const ElemCol& ec, const bool (&ok)[4], bool live,
                            int b, int sb, int nrows, int c0, float gs, uint32_t voff,
                            float* myring, const float (*cf)[8], f32x2 (&sg2)[4]) {
  constexpr int NR = kElemRing;
  const int lane = threadIdx.x & 63;
  const int64_t rowb = (int64_t)b * p.S + sb;
  const char* tbase = reinterpret_cast<const char*>(p.T + rowb * p.ldT);
  const int64_t rstride = (int64_t)p.ldT * 4;
  auto issue = [&](int r) {  // LDS-DMA of row r (sub-chunk-relative) into its slot
    lds_dma16(tbase + r * rstride, voff, lds_addr(myring + (r % NR) * 256));
  };
  const int pro = min(NR, nrows);
  for (int r = 0; r < pro; ++r) issue(r);
  // each column's ranking coefficient read from its own cf address (rkp at
  // byte 0 of a row, rkn at 16; alpha at 8 and 24, so 8 past either): no
  // per-row select
  uint32_t rsel[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) rsel[q] = ec.pos[q] ? 0u : 16u;
  // the lane's plane offset in a row (bytes); the row base is wave-uniform
  const uint32_t loffb = live ? 2u * (uint32_t)(((c0 >> 5) << 6) + (c0 & 31)) : 0u;
  f32x2 qc1 = splat2(kErfcxC1);
  asm volatile("" : "+v"(qc1));
  auto row = [&](int r) {
    const f32x4 tv = *reinterpret_cast<const f32x4*>(myring + (r % NR) * 256 + lane * 4);
    const float t[4] = {tv[0], tv[1], tv[2], tv[3]};
    f32x2 g2[4];
    // (the row offset opaque: a scalar, so each address is one add)
    const char* crow =
        reinterpret_cast<const char*>(&cf[0][0]) + __builtin_amdgcn_readfirstlane(r * 32);
    const f32x2 rkp = *reinterpret_cast<const f32x2*>(crow);
    const f32x2 rkn = *reinterpret_cast<const f32x2*>(crow + 16);
    if (SOFT) {
      const f32x2 alpha = *reinterpret_cast<const f32x2*>(crow + 8);
      d_elem2x4<SOFT, false, true>(t, ec, alpha, rkp, rkn, g2);
    } else {
      f32x2 rkq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) rkq[q] = *reinterpret_cast<const f32x2*>(crow + rsel[q]);
      const f32x2 alpha = *reinterpret_cast<const f32x2*>(crow + rsel[0] + 8);
      d_elem2x4<SOFT, false, true>(t, ec, alpha, rkp, rkn, g2, rkq, &qc1);
    }
    // (the row's rkp is wave-uniform)
    if (NANCHK && __builtin_amdgcn_readfirstlane((rkp.x != rkp.x || rkp.y != rkp.y) ? 1 : 0))
      poison_row(g2, rkp);
    float G[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sg2[q] = sg2[q] + g2[q];
      G[q] = add_f32(g2[q].x, g2[q].y);
      if (MASK && !ok[q]) G[q] = 0.0f;
    }
    uint32_t hv[2], lv[2];
    split2_f16(G[0], G[1], gs, hv[0], lv[0]);
    split2_f16(G[2], G[3], gs, hv[1], lv[1]);
    // the row base made opaque so it stays a scalar base (saddr stores with a
    // 32-bit lane offset, no 64-bit address add per row)
    const uint64_t ga = reinterpret_cast<uint64_t>(p.g + (rowb + r) * p.gld);
    // (readfirstlane returns int: each half zero-extended through uint32_t)
    const uint64_t grow =
        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(ga >> 32)) << 32) |
        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)ga);
    if (!MASK || live) {  // nontemporal plane stores (the element pass -2 %, round 2)
      // (asm: hipcc forms a 64-bit lane address per row otherwise; the ring's
      // vmcnt arithmetic counts these two stores as before)
      asm volatile("global_store_dwordx2 %0, %1, %2 nt\n\t"
                   "global_store_dwordx2 %0, %3, %2 offset:%4 nt"
                   :
                   : "v"(loffb), "v"(u32x2{hv[0], hv[1]}), "s"(grow), "v"(u32x2{lv[0], lv[1]}),
                     "i"(2 * kLoOff));
    }
    if (r + NR < nrows) issue(r + NR);  // into the slot row r was just read from
  };
  // Before row r is read, the ops issued after its DMA are the DMAs of rows
  // r+1 .. min(r+NR-1, last) and the two plane stores of each row
  // max(0, r-NR+1) .. r-1 (vector memory ops retire in issue order).  Rows
  // NR-1 .. nrows-NR wait for a constant count; the ramps use the run-time
  // count (an s_waitcnt takes an immediate: a compare ladder).  Only the
  // common loop (binary labels, full waves, no degenerate row) is peeled.
  int r = 0;
  if (!SOFT && !MASK && !NANCHK) {
    for (; r < min(NR - 1, nrows); ++r) {
      wait_vmcnt_dyn(min(NR - 1, nrows - 1 - r) + 2 * r);
      row(r);
    }
    for (; r <= nrows - NR; ++r) {
      wait_vmcnt<3 * (NR - 1)>();
      row(r);
    }
  }
  for (; r < nrows; ++r) {
    wait_vmcnt_dyn(min(NR - 1, nrows - 1 - r) + 2 * min(r, NR - 1));
    row(r);
  }
}

__global__ __launch_bounds__(256, 3) void bwd_elem_ring_kernel(ElemParams p) {
  constexpr int NR = kElemRing, CR = kElemRingRows;
  __shared__ __attribute__((aligned(16))) float ring[4][NR][256];  // [wave][slot][1 KB]
  __shared__ __attribute__((aligned(16))) float cf[CR][8];  // rkp, alpha, rkn, alpha (label, feature)
  const int b = blockIdx.x, sc = blockIdx.y, tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = blockIdx.z * 1024 + tid * 4;
  const int S = p.S, B = p.B, L = p.L;
  const float gs = wave_pow2_scale(p.g_bound, B);
  bool ok[4];
  ElemCol ec;
  elem_col_setup(p, b, c0, true, ok, ec);
  bool my_soft = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) my_soft |= ok[q] && ec.soft[q];
  const bool soft_any = __syncthreads_or(my_soft) != 0;
  // a wave whose first lane is past the planes' columns writes nothing and
  // streams nothing (its lane 0 has the wave's smallest c0); in a live wave
  // every store instruction has a live lane, so it issues (the vmcnt
  // arithmetic of elem_ring_rows counts on that)
  const bool wave_live = (int)(blockIdx.z * 1024 + wid * 256) < p.Lc;
  // every lane's four columns are labels (< L) and in the planes (< Lc)
  const bool wave_full = (int)(blockIdx.z * 1024 + wid * 256 + 256) <= min(L, p.Lc);
  const bool live = c0 < p.Lc;
  const int s_begin = sc * p.rows_per_chunk;
  const int s_end = min(S, s_begin + p.rows_per_chunk);
  // lanes past the row's end (L % 1024 != 0) re-read column 0 and are masked
  const uint32_t voff = (uint32_t)((c0 < L ? c0 : 0) * 4);
  f32x2 sg2[4] = {splat2(0.f), splat2(0.f), splat2(0.f), splat2(0.f)};
  for (int sb = s_begin; sb < s_end; sb += CR) {  // sub-chunks of <= CR rows
    const int nrows = min(CR, s_end - sb);
    __syncthreads();  // the previous sub-chunk's cf reads are done
    // cf[row] = rkp, alpha, rkn, alpha as (label, feature) pairs (alpha 8
    // bytes past either ranking coefficient: elem_ring_rows)
    bool nan_row = false;
    for (int r = tid; r < nrows; r += 256) {
      f32x2 alpha, bP, bN, rkp, rkn;
      elem_coef_load(p, (int64_t)b * S + sb + r, alpha, bP, bN);
      elem_rank_coefs(ec, bP, bN, rkp, rkn);
      nan_row |= bP.x != bP.x || bP.y != bP.y;
      *reinterpret_cast<f32x4*>(&cf[r][0]) = f32x4{rkp.x, rkp.y, alpha.x, alpha.y};
      *reinterpret_cast<f32x4*>(&cf[r][4]) = f32x4{rkn.x, rkn.y, alpha.x, alpha.y};
    }
    const bool nan_any = __syncthreads_or(nan_row) != 0;
    if (!wave_live) continue;
    float* myring = &ring[wid][0][0];
    if (soft_any || !wave_full || nan_any) {
      if (soft_any)
        elem_ring_rows<true, true, true>(p, ec, ok, live, b, sb, nrows, c0, gs, voff, myring, cf, sg2);
      else
        elem_ring_rows<false, true, true>(p, ec, ok, live, b, sb, nrows, c0, gs, voff, myring, cf, sg2);
    } else {
      elem_ring_rows<false, false, false>(p, ec, ok, live, b, sb, nrows, c0, gs, voff, myring, cf,
                                          sg2);
    }
  }
  // the ring is free now: its first 8 KB serve as cred
  __syncthreads();
  elem_colsum_store(p, sg2, &ring[0][0][0], 256, 1);
}

// ---------------------------------------------------------------- dR GEMMs
// What every dR GEMM kernel (3xf16 or fp32) takes: the split-K grid and its output.
struct DrCommon {
  float* slab;  // [nKc][L][z]
  int S, B, L, z;
  int nLt, nZt, nKc, rows_per_chunk;
};

// ------------------------------------------------------------ 3xf16 dR GEMM
// K axis = the S*B sample rows q = b*S + s: the noise planes' own row order, in
// which the element pass also writes the G planes, so a K row is one address
// for both operands.  The rows stream in stages of 32 through a ring of LDS
// stage images (LDS-DMA, one barrier per stage).  Both operands are chunked
// (mpv_split16), so the 128 columns of a tile are 512 contiguous bytes per row
// holding hi and lo; a stage image is [G rows | E rows], 32 rows x 512 B each
// (the 256 tile keeps the operands' images apart: DrsAddr),
// and one DMA wave-instruction moves two whole rows.  The 32-B unit U of row r
// (units 4k, 4k+1: hi of columns 32k..32k+31; 4k+2, 4k+3: their lo) sits at
// position U ^ (r & 7).  An MFMA fragment (8 K rows of one column per lane) is
// two ds_read_b64_tr_b16; lane group g reads rows 4g..4g+3 and 16+4g..16+4g+3,
// so a 32-lane half of one transposed read touches rows 8j..8j+7 at 8 distinct
// positions mod 256 B, all 64 banks once: conflict-free (checked).
// Element j of lane group g holds K row (j < 4 ? 4g + j : 16 + 4g + j - 4), the
// same for A and B.
// (k sits where its fields always were: the kernels' argument layout is unchanged)
struct Dr16Params {
  const uint16_t* g;    // chunked G planes, rows b*S + s, gld halves per row
  const float* g_bound;  // (B) per-row bounds of |G|: the planes' scale (wave_pow2_scale)
  int64_t gld;
  mpv_split16 eps16;    // rows b*S + s
  DrCommon k;
  int rows_pad;
};

constexpr int kDrKR = 32;     // K rows per stage (one MFMA k-step)

// Geometry of a 3xf16 dR tile: WM x WN waves, each TM x TN MFMA tiles of 16 x 16.
template <int WM_, int WN_, int TM_, int TN_>
struct Dr16Tile {
  static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_;
  static constexpr int NW = WM * WN;
  static constexpr int BL = WM * TM * 16, BZ = WN * TN * 16;
  static_assert(BL == BZ, "square tile: one LDS row layout for both operands");
  static constexpr int ROWB = BL * 4;          // bytes per LDS row: BL columns, hi + lo
  static constexpr int IMG = kDrKR * ROWB;     // per operand
  static constexpr int STAGE = 2 * IMG;
  static constexpr int PIECES = STAGE / 1024;  // 1-KB wave-instructions per stage
  static constexpr int RPP = 1024 / ROWB;      // rows per piece
  static_assert(RPP >= 1 && RPP * ROWB == 1024, "a 1-KB DMA piece is whole rows");
};

// base: a generic pointer into LDS or an LDS-typed one (lds_cptr)
using lds_cptr = const __attribute__((address_space(3))) char*;
template <class Ptr>
MPV_DEV s16x4 tr_read(Ptr base, int off) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(base + off));
}

// block id -> (kc, tile): all tiles of one K chunk share rows -> ids equal mod 8
MPV_DEV void decode_kc_tile(int id, int K, int nT, int& kc, int& tile) {
  const int full = (K / 8) * 8 * nT;
  if (id < full) {
    const int q = id / (8 * nT), r = id % (8 * nT);
    tile = r / 8;
    kc = q * 8 + (r % 8);
  } else {
    const int r = id - full, Kr = K % 8;
    tile = r / Kr;
    kc = (K / 8) * 8 + (r % Kr);
  }
}

// What a dR workgroup and its waves and lanes own, fixed for its life.
struct DrCtx {
  int kc, tile, l0, z0;      // K chunk, output tile and its first label / latent column
  int wid, wm, wn;           // wave (uniform) and its place in the WM x WN grid
  int lane, lr, lg;          // lane, lane & 15, lane >> 4
  int rows;                  // sample rows B*S
  int q_begin, q_end;        // the chunk's K rows
  int r0, r1, sw, tp;        // transposed reads: the lane's two LDS rows, r0 & 7, 16-B part
};

// q_limit: where the last chunk ends (the 3xf16 kernels run over the padded rows).
template <int BL, int BZ, int WN>
MPV_DEV DrCtx dr_ctx(const DrCommon& p, int q_limit) {
  DrCtx c;
  decode_kc_tile(blockIdx.x, p.nKc, p.nLt * p.nZt, c.kc, c.tile);
  c.l0 = (c.tile / p.nZt) * BL, c.z0 = (c.tile % p.nZt) * BZ;
  c.lane = threadIdx.x & 63;
  c.wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  c.wm = c.wid / WN, c.wn = c.wid % WN;
  c.lr = c.lane & 15, c.lg = c.lane >> 4;
  c.rows = p.B * p.S;
  c.q_begin = c.kc * p.rows_per_chunk;
  c.q_end = min(q_limit, c.q_begin + p.rows_per_chunk);
  // lane 4q+p of its 16-lane group
  const int tq = c.lr >> 2;
  c.tp = c.lr & 3;
  c.r0 = c.lg * 4 + tq, c.r1 = c.r0 + 16, c.sw = c.r0 & 7;
  return c;
}

// The workgroup's tile of slab kc.  D[i = l][j = z]: row = lg*4 + reg, col = lr.
// SCALED false (fp32 operands): the accumulators as they are.
template <bool SCALED = true, int TM, int TN>
MPV_DEV void dr_store_slab(const f32x4 (&acc)[TM][TN], const DrCtx& c, const DrCommon& k,
                           float inv = 1.0f) {
  const int L = k.L, z = k.z;
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int l = c.l0 + (c.wm * TM + m) * 16 + c.lg * 4 + i;
        const int zc = c.z0 + (c.wn * TN + n) * 16 + c.lr;
        if (l < L && zc < z)
          k.slab[((int64_t)c.kc * L + l) * z + zc] = SCALED ? acc[m][n][i] * inv : acc[m][n][i];
      }
}

// 1 / (the G planes' scale x the noise planes' scale): the 3xf16 slabs' factor
MPV_DEV float dr16_inv_scale(const Dr16Params& p) {
  return 1.0f / (wave_pow2_scale(p.g_bound, p.k.B) * *p.eps16.scale);
}

// Fragments of one dR stage (per wave: TM A tiles and TN B tiles, hi and lo).
template <int TM, int TN>
struct DrFrag {
  s16x8 ah[TM], al[TM], bh[TN], bl[TN];
};

template <class T, class Ptr>
MPV_DEV void dr_read(DrFrag<T::TM, T::TN>& f, Ptr base, const DrCtx& c) {
  constexpr int TM = T::TM, TN = T::TN, ROWB = T::ROWB, IMG = T::IMG;
  const int r0 = c.r0, r1 = c.r1, sw = c.sw, tp = c.tp;
#pragma unroll
  for (int m = 0; m < TM; ++m) {
    const int t = c.wm * TM + m, uh = (t >> 1) * 4 + (t & 1);
    const int ch = ((uh ^ sw) << 5) + tp * 8, cl = (((uh + 2) ^ sw) << 5) + tp * 8;
    f.ah[m] = __builtin_shufflevector(tr_read(base, r0 * ROWB + ch), tr_read(base, r1 * ROWB + ch),
                                      0, 1, 2, 3, 4, 5, 6, 7);
    f.al[m] = __builtin_shufflevector(tr_read(base, r0 * ROWB + cl), tr_read(base, r1 * ROWB + cl),
                                      0, 1, 2, 3, 4, 5, 6, 7);
  }
#pragma unroll
  for (int n = 0; n < TN; ++n) {
    const int t = c.wn * TN + n, uh = (t >> 1) * 4 + (t & 1);
    const int ch = ((uh ^ sw) << 5) + tp * 8, cl = (((uh + 2) ^ sw) << 5) + tp * 8;
    f.bh[n] = __builtin_shufflevector(tr_read(base + IMG, r0 * ROWB + ch),
                                      tr_read(base + IMG, r1 * ROWB + ch), 0, 1, 2, 3, 4, 5, 6, 7);
    f.bl[n] = __builtin_shufflevector(tr_read(base + IMG, r0 * ROWB + cl),
                                      tr_read(base + IMG, r1 * ROWB + cl), 0, 1, 2, 3, 4, 5, 6, 7);
  }
}

// The stage's 3xf16 products: hi hi, hi lo, lo hi.
template <int TM, int TN>
MPV_DEV void dr_mfma(f32x4 (&acc)[TM][TN], const DrFrag<TM, TN>& f) {
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n) {
      acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_f16x8(f.ah[m]), as_f16x8(f.bh[n]),
                                                         acc[m][n], 0, 0, 0);
      acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_f16x8(f.ah[m]), as_f16x8(f.bl[n]),
                                                         acc[m][n], 0, 0, 0);
      acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_f16x8(f.al[m]), as_f16x8(f.bh[n]),
                                                         acc[m][n], 0, 0, 0);
    }
}

// One stage's LDS-DMA for this wave: PER_WAVE 1-KB pieces of RPP whole rows.
// Wave w moves pieces w*PER_WAVE ..; the first PIECES/2 are G rows, the rest E.
// The global base address is the piece's first row (wave-uniform: it goes in
// an SGPR pair); with RPP > 1 a lane's row within the piece is in its offset.
template <int PER_WAVE, int PIECES, int RPP>
MPV_DEV void dr_issue(const Dr16Params& p, char* dst, int q0, int rows, int wid,
                      const int (&dma_off)[PER_WAVE]) {
  const int lrow = RPP == 1 ? 0 : (int)(threadIdx.x & 63) / (64 / RPP);
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int pc = wid * PER_WAVE + i;
    const int q = q0 + (pc % (PIECES / 2)) * RPP;
    const uint16_t* src;
    int off = dma_off[i];
    if (pc < PIECES / 2) {  // G rows >= rows are zero
      src = p.g + (int64_t)q * p.gld;
      off += lrow * p.gld * 2;
    } else {  // E rows >= rows: repeat the last real row (finite, times a zero G row)
      const int qb = min(q, rows - 1);
      src = p.eps16.data + (int64_t)qb * p.eps16.ld;
      off += (min(q + lrow, rows - 1) - qb) * (int)p.eps16.ld * 2;
    }
    lds_dma16(src, (uint32_t)off, lds_addr(dst + pc * 1024));
  }
}

// The 64 and 128 tiles: every wave streams its share of stage ci+1 (a burst of
// LDS-DMA) and then reads and multiplies stage ci; two stage images, one
// barrier per stage.
template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(WM* WN * 64, 1) void dR16_kernel(Dr16Params p) {
  using T = Dr16Tile<WM, WN, TM, TN>;
  constexpr int STAGE = T::STAGE, PIECES = T::PIECES, RPP = T::RPP;
  static_assert(PIECES % T::NW == 0, "DMA pieces must split over waves");
  constexpr int PER_WAVE = PIECES / T::NW;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const DrCtx c = dr_ctx<T::BL, T::BZ, WN>(p.k, p.rows_pad);
  // DMA lane mapping: RPP rows per 1-KB wave-instruction; wave w moves pieces
  // w*PER_WAVE ..; the first PIECES/2 are G rows, the rest E rows.  Per-lane
  // byte offsets (without the stage's first row) of my pieces:
  int dma_off[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int pc = c.wid * PER_WAVE + i;
    const int pr = pc % (PIECES / 2);
    const int lrow = c.lane / (64 / RPP), lpos = c.lane % (64 / RPP);  // 16-B slot within the row
    const int r = pr * RPP + lrow;  // K row within the stage
    const int u_lds = lpos >> 1, half = lpos & 1;
    const int u_src = u_lds ^ (r & 7);
    // (chunked planes: 4 B per column)
    dma_off[i] = 4 * (pc < PIECES / 2 ? c.l0 : c.z0) + u_src * 32 + half * 16;
  }

  // (The zeroing loops and the stage count stay written out here and in
  // dR16s_kernel, in this order: with the count a DrCtx field, the accumulators
  // zeroed by an initialiser, or both in a helper, hipcc allocates
  // dR16s_kernel's registers differently and it runs 1.4-2 % slower at C4.)
  f32x4 acc[TM][TN];
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nst = (c.q_end - c.q_begin + kDrKR - 1) / kDrKR;
  // (a loop of one pass, not an if: after an if hipcc waits for all of a
  // stage's fragment reads before its first MFMA instead of read by read)
  for (int j = 0; j < 1 && j < nst; ++j)
    dr_issue<PER_WAVE, PIECES, RPP>(p, smem + j * STAGE, c.q_begin + j * kDrKR, c.rows, c.wid,
                                    dma_off);
  for (int ci = 0; ci < nst; ++ci) {
    wait_vmcnt<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    barrier_raw();  // stage ci landed for every wave; all waves are done reading ci-1
    if (ci + 1 < nst)
      dr_issue<PER_WAVE, PIECES, RPP>(p, smem + ((ci + 1) % 2) * STAGE,
                                      c.q_begin + (ci + 1) * kDrKR, c.rows, c.wid, dma_off);
    DrFrag<TM, TN> f;
    // (an LDS-typed base: through a generic pointer hipcc adds the lane's row
    // offset again at every read, 15 more VALU instructions per stage of the
    // 128 tile)
    dr_read<T>(f, (lds_cptr)(smem + (ci % 2) * STAGE), c);
    dr_mfma(acc, f);
  }
  dr_store_slab(acc, c, p.k, dr16_inv_scale(p));
}

// ---- the 256 tile's ring, fragment addresses and stage DMA (dR16s_kernel) ----
// Its ring holds the two stage images operand by operand,
//   [G stage 0 | G stage 1 | E stage 0 | E stage 1],  IMG bytes each,
// so both parities of an operand lie within 64 KB of one base and a transposed
// read's whole stage / row / unit-group displacement fits ds_read's 16-bit
// offset field.  A lane reads  r*ROWB + ((uh ^ sw) << 5) + tp*8  of an image,
// uh = (t>>1)*4 + (t&1) (+2 for a lo unit) and t = w*TT + i the wave's i-th
// tile; with TT a multiple of 4, uh = w*2*TT + uhi and only uhi & 7 meets the
// 3-bit sw.  So eight bases per operand, one per value of (uhi & 7) ^ sw with
// r0*ROWB, tp*8 and the wave's w*TT*64 folded in, and everything else is an
// immediate: (uhi >> 3)*256, row r1 = r0 + 16 at +16*ROWB, stage parity at
// +IMG.  16 address VGPRs, fixed for the kernel's life; no address arithmetic
// in the stage loops (the [G|E][G|E] ring with a run-time stage base took
// 48-79 VALU per stage to rebuild these addresses from the parity).
template <class T>
struct DrsAddr {
  static_assert(T::TM % 4 == 0 && T::TN % 4 == 0, "a wave's units start at a multiple of 8");
  static_assert(T::IMG + 16 * T::ROWB + ((2 * (T::TM > T::TN ? T::TM : T::TN) - 1) >> 3) * 256 < 65536,
                "the displacements fit ds_read's offset field");
  lds_cptr a[8], b[8];
  MPV_DEV void init(lds_cptr ring, const DrCtx& c) {
    const int lane_b = c.r0 * T::ROWB + c.tp * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = ring + (c.wm * T::TM * 64 + lane_b + ((j ^ c.sw) << 5));
      b[j] = ring + (2 * T::IMG + c.wn * T::TN * 64 + lane_b + ((j ^ c.sw) << 5));
      // opaque from here on: hipcc otherwise keeps sw and rebuilds them per stage
      asm volatile("" : "+v"(a[j]));
      asm volatile("" : "+v"(b[j]));
    }
  }
};

// hi (LO = 0) or lo (LO = 2) fragment of the wave's I-th tile, stage parity PAR
template <class T, int PAR, int I, int LO>
MPV_DEV s16x8 drs_frag(const lds_cptr (&base)[8]) {
  constexpr int uhi = (I >> 1) * 4 + (I & 1) + LO;
  constexpr int off = PAR * T::IMG + (uhi >> 3) * 256;
  return __builtin_shufflevector(tr_read(base[uhi & 7], off),
                                 tr_read(base[uhi & 7], off + 16 * T::ROWB), 0, 1, 2, 3, 4, 5, 6, 7);
}

// Step K of a stage's reads: the hi and lo fragments of one tile, A tiles first
// (the order of dr_read).
template <class T, int PAR, int K>
MPV_DEV void drs_read_step(DrFrag<T::TM, T::TN>& f, const DrsAddr<T>& ad) {
  if constexpr (K < T::TM) {
    f.ah[K] = drs_frag<T, PAR, K, 0>(ad.a);
    f.al[K] = drs_frag<T, PAR, K, 2>(ad.a);
  } else {
    f.bh[K - T::TM] = drs_frag<T, PAR, K - T::TM, 0>(ad.b);
    f.bl[K - T::TM] = drs_frag<T, PAR, K - T::TM, 2>(ad.b);
  }
}

template <class T, int PAR, int K = 0>
MPV_DEV void drs_read(DrFrag<T::TM, T::TN>& f, const DrsAddr<T>& ad) {
  if constexpr (K < T::TM + T::TN) {
    drs_read_step<T, PAR, K>(f, ad);
    drs_read<T, PAR, K + 1>(f, ad);
  }
}

// lds_dma16 to LDS byte lds_base + OFF, with M0 set by one scalar add and left
// there: nothing else in dR16s_kernel reads or sets M0 (gfx950's ds_read needs
// none; checked in its assembly).  M0 is reserved to hipcc, which sets it right
// at each use of its own, so it cannot be named as a clobber.
template <int OFF>
MPV_DEV void lds_dma16_at(const void* saddr, uint32_t voff, uint32_t lds_base) {
  asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               :
               : "v"(voff), "s"(saddr), "s"(lds_base), "n"(OFF)
               : "memory", "scc");
}

// Pieces pc0 .. pc0+COUNT-1 of one stage's LDS-DMA (one row each: the first
// PIECES/2 are G rows into dst_g, the rest E rows into dst_e).
template <int COUNT, int PIECES>
MPV_DEV void drs_issue_range(const Dr16Params& p, char* dst_g, char* dst_e, int q0, int rows,
                             int pc0, int l0, int z0, int lane_u, int lane_h) {
#pragma unroll
  for (int i = 0; i < COUNT; ++i) {
    const int pc = pc0 + i;  // wave-uniform
    const bool is_g = pc < PIECES / 2;
    const int r = is_g ? pc : pc - PIECES / 2;
    const int q = q0 + r;
    const char* src = is_g ? reinterpret_cast<const char*>(p.g + (int64_t)q * p.gld + 2 * l0)
                           : reinterpret_cast<const char*>(p.eps16.data +
                                                           (int64_t)min(q, rows - 1) * p.eps16.ld +
                                                           2 * z0);
    lds_dma16(src, (uint32_t)(((lane_u ^ (r & 7)) << 5) + lane_h),
              lds_addr((is_g ? dst_g : dst_e) + r * 1024));
  }
}

// A group-0 wave's share of every stage's LDS-DMA: PER_WAVE consecutive rows
// of one operand (the first WN/2 waves G rows, the others noise rows), walked
// by 64-bit pointer increments -- two SALU per row instead of the ~14 of a
// row * ld product and clamp per piece (round 5: the stage's DMA block 325 ->
// 139 instructions, dR -1.5 %, profiles/r05_dr_dma_ab.json).
template <int PER_WAVE, int PIECES, int WN>
struct DrsDma {
  const char* src;    // first row of this wave's share of the next stage
  int64_t row_b;      // bytes per source row
  int r_first;        // that row's place in the stage
  uint32_t lds_base;  // LDS byte address of the share in its operand's stage-0 image
  bool is_g;
  MPV_DEV void init(const Dr16Params& p, int q_begin, int wn, int l0, int z0, uint32_t ring,
                    int img) {
    static_assert(PIECES / 2 == (WN / 2) * PER_WAVE, "G rows on the first half of the waves");
    static_assert(PER_WAVE % 8 == 0, "the source swizzle (row & 7) restarts with every share");
    const int pc = wn * PER_WAVE;
    is_g = pc < PIECES / 2;
    r_first = is_g ? pc : pc - PIECES / 2;
    lds_base = ring + (is_g ? 0 : 2 * img) + r_first * 1024;
    const int q = q_begin + kDrKR + r_first;  // the first stage it streams is stage 1
    row_b = is_g ? p.gld * 2 : p.eps16.ld * 2;
    src = is_g ? reinterpret_cast<const char*>(p.g + (int64_t)q * p.gld + 2 * l0)
               : reinterpret_cast<const char*>(p.eps16.data + (int64_t)q * p.eps16.ld + 2 * z0);
  }
};

// drs_read of stage parity PAR with a group-0 wave's share of the next stage's
// LDS-DMA (into the images of parity 1 - PAR) woven in: one or two 1-KB pieces
// after each tile's four transposed reads, so the CU's load path (the DMA) and
// the LDS (the reads) work side by side instead of the reads queueing behind
// the whole DMA burst (profiles/r05_dr_ab.json: DMA issue 1060 + reads 960
// ticks, serial, against 1650 for the other group's MFMAs).  A piece is a
// pointer step (2 SALU), the M0 add, a wait state and the DMA, its lanes'
// source swizzle voff ^ (row & 7) << 5 being loop-invariant.  TAIL: the stage streamed is the chunk's last and may be the padded
// one (q_next = its first row of this share): noise rows past the last real
// one repeat that row, as drs_issue_range clamps them; G rows there are zero
// in the planes (rows_pad).  Only that stage pays the compare and selects.
// pieces I .. END-1 of the share
template <class T, int PAR, bool TAIL, int I, int END, class Dma>
MPV_DEV void drs_pieces(const Dma& dma, const char*& sp, int nvalid, uint32_t voff) {
  if constexpr (I < END) {
    lds_dma16_at<(1 - PAR) * T::IMG + I * 1024>(sp, voff ^ ((I & 7) << 5), dma.lds_base);
    if constexpr (TAIL) sp += (I + 1 < nvalid) ? dma.row_b : 0;
    else sp += dma.row_b;
    drs_pieces<T, PAR, TAIL, I + 1, END>(dma, sp, nvalid, voff);
  }
}

template <class T, int PER_WAVE, int PAR, bool TAIL, int K = 0, class Dma>
MPV_DEV void drs_read_dma_steps(DrFrag<T::TM, T::TN>& f, const DrsAddr<T>& ad, const Dma& dma,
                                const char*& sp, int nvalid, uint32_t voff) {
  constexpr int STEPS = T::TM + T::TN;
  if constexpr (K < STEPS) {
    drs_read_step<T, PAR, K>(f, ad);
    __builtin_amdgcn_sched_barrier(0);
    drs_pieces<T, PAR, TAIL, K * PER_WAVE / STEPS, (K + 1) * PER_WAVE / STEPS>(dma, sp, nvalid, voff);
    __builtin_amdgcn_sched_barrier(0);
    drs_read_dma_steps<T, PER_WAVE, PAR, TAIL, K + 1>(f, ad, dma, sp, nvalid, voff);
  }
}

template <class T, int PER_WAVE, int PAR, bool TAIL, class Dma>
MPV_DEV void drs_read_dma(DrFrag<T::TM, T::TN>& f, const DrsAddr<T>& ad, Dma& dma, int q_next,
                          int rows, uint32_t voff) {
  const char* sp = dma.src;
  int nvalid = PER_WAVE;
  if (TAIL && !dma.is_g) {
    const int over = q_next - (rows - 1);
    if (over > 0) sp -= over * dma.row_b;
    nvalid = max(1, min(PER_WAVE, rows - q_next));
  }
  drs_read_dma_steps<T, PER_WAVE, PAR, TAIL>(f, ad, dma, sp, nvalid, voff);
  dma.src += kDrKR * dma.row_b;  // on to the next stage
}

// Staggered schedule: the waves of row wm = 0 (group 0) and wm = 1 (group 1)
// share the SIMDs pairwise and run one phase apart, so on every SIMD one wave
// issues MFMAs while the other streams/reads.  Time is cut into slots ended by
// one barrier each; group 0 does mem(i) in slot 2i and mma(i) in slot 2i+1,
// group 1 does mem(i) in slot 2i+1 and mma(i) in slot 2i+2.
//   mem(i): fragment reads of stage i; group 0 weaves the LDS-DMA of stage i+1
//           into the other parity's images (read by group 1 in slot 2i-1, so
//           free) into them (drs_read_dma).
//   mma(i): 96 MFMAs; group 0 then waits for its stage i+1 DMA, so stage i+1
//           is visible to both groups after the slot's barrier.
// Two 64-KB stage images (laid out operand by operand: DrsAddr); DMA latency
// budget = one slot pair.  Round 5
// (the slot-timing study in profiles/r05_dr_ab.json): with the DMA as a burst ahead
// of the reads, group 0's mem slot (1060 + 960 ticks) outlasted the other
// group's MFMAs (1650) every slot; woven, dR -4.2 %.  Measured slower: group 1
// issuing the stream between its own MFMAs (+2.3 %), half of it in each
// group's read slot (+12 % woven, +0.8 % with group 1's half ahead of its
// reads).
template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(WM* WN * 64, 1) void dR16s_kernel(Dr16Params p) {
  static_assert(WM == 2, "two wave groups");
  using T = Dr16Tile<WM, WN, TM, TN>;
  constexpr int IMG = T::IMG, PIECES = T::PIECES;
  constexpr int PER_WAVE = PIECES / WN;  // pieces per group-0 wave (group 1 issues none)
  static_assert(PIECES % WN == 0, "DMA pieces must split over the waves");
  static_assert(T::RPP == 1, "one 1-KB row per DMA piece");
  // [G stage 0 | G stage 1 | E stage 0 | E stage 1] (DrsAddr)
  __shared__ __attribute__((aligned(1024))) char smem[4 * IMG];

  const DrCtx c = dr_ctx<T::BL, T::BZ, WN>(p.k, p.rows_pad);
  const int grp = c.wm, wn = c.wn;
  // per-lane part of a piece's source offset: 16-B slot `lane` of the row
  // (32-B unit lane/2, swizzled by the row's r & 7, which cycles with the piece)
  const int lane_u = c.lane >> 1, lane_h = (c.lane & 1) * 16;

  // (written out, in this order: the note in dR16_kernel)
  f32x4 acc[TM][TN];
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nst = (c.q_end - c.q_begin + kDrKR - 1) / kDrKR;
  // Stage i lives in the images of parity (i + p0) & 1, p0 = nst & 1: the last
  // stage always has parity 1 and the one before it parity 0, so the peeled
  // end of the chunk is one code path and the odd stage is peeled at the front.
  const int p0 = nst & 1;
  if (grp == 0 && nst > 0) {
    drs_issue_range<PER_WAVE, PIECES>(p, smem + p0 * IMG, smem + (2 + p0) * IMG, c.q_begin, c.rows,
                                      wn * PER_WAVE, c.l0, c.z0, lane_u, lane_h);
    wait_vmcnt<0>();
  }
  DrFrag<TM, TN> f;
  DrsAddr<T> ad;
  ad.init((lds_cptr)smem, c);
  barrier_raw();
  // the second slot of a stage: its 96 MFMAs
  auto mma = [&]() {
    lds_barrier();
    __builtin_amdgcn_s_setprio(1);
    dr_mfma(acc, f);
    __builtin_amdgcn_s_setprio(0);
  };
  // The stage loops are unrolled by parity, so every LDS displacement is an
  // immediate; a chunk with an odd number of stages skips the first pair's
  // parity-0 half.  The two groups run the same number of barriers: 2*nst + 1
  bool skip = p0;
  if (grp == 0) {
    DrsDma<PER_WAVE, PIECES, WN> dma;
    dma.init(p, c.q_begin, wn, c.l0, c.z0, lds_addr(smem), IMG);
    // (a piece's swizzle is written as an xor next to its DMA; hipcc hoists the
    // eight values out of the loops on its own, registers permitting: forced
    // into registers beside the 16 read bases they spilled the accumulators)
    const uint32_t voff = (uint32_t)((lane_u << 5) + lane_h);
    // slot 2i: read stage i with stage i+1's DMA woven in; slot 2i+1: MFMAs
    // of stage i, then stage i+1 landed before the closing barrier
    auto stream = [&](auto par, auto tail) {
      drs_read_dma<T, PER_WAVE, decltype(par)::value, decltype(tail)::value>(
          f, ad, dma, c.q_begin + (nst - 1) * kDrKR + dma.r_first, c.rows, voff);
      mma();
      wait_vmcnt<0>();
      barrier_raw();
    };
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    // the steady state streams the stages before the chunk's last: whole, real rows
#pragma clang loop unroll(disable)
    for (int n = nst - 2 + p0; n > 0; n -= 2) {
      if (!skip) stream(P0{}, std::false_type{});
      skip = false;
      stream(P1{}, std::false_type{});
    }
    if (nst >= 2) stream(P0{}, std::true_type{});  // streams the last stage
    if (nst >= 1) {  // the last stage: nothing to stream
      drs_read<T, 1>(f, ad);
      mma();
      barrier_raw();
    }
    barrier_raw();
  } else {
    barrier_raw();
    // slot 2i+1: read stage i; slot 2i+2: MFMAs of stage i
#pragma clang loop unroll(disable)
    for (int n = nst + p0; n > 0; n -= 2) {
      if (!skip) {
        drs_read<T, 0>(f, ad);
        mma();
        barrier_raw();
      }
      skip = false;
      drs_read<T, 1>(f, ad);
      mma();
      barrier_raw();
    }
  }
  dr_store_slab(acc, c, p.k, dr16_inv_scale(p));
}

// ---------------------------------------------------------------- dR GEMM
struct DrParams {
  const float* G;    // (B*S, ldG): row q = b*S + s  (the T buffer)
  const float* eps;  // (S, B, z)
  DrCommon k;
  int ldG;  // t_cols(L)
};

constexpr int kDrBK = 32;

template <int TM, int TN>
__global__ __launch_bounds__(256) void dR_gemm_kernel(DrParams p) {
  constexpr int WM = 2, WN = 2;
  constexpr int BM = WM * TM * 16;  // l tile
  constexpr int BN = WN * TN * 16;  // z tile
  constexpr int LDG = BM + 16, LDE = BN + 16;  // conflict-free ds_read_b32 (stride = 16 mod 32)
  constexpr int G4 = kDrBK * BM / 4, E4 = kDrBK * BN / 4;
  constexpr int GV = (G4 + 255) / 256, EV = (E4 + 255) / 256;
  __shared__ __attribute__((aligned(16))) float smem[kDrBK * (LDG + LDE)];
  float* Gs = smem;
  float* Es = smem + kDrBK * LDG;

  const DrCtx ctx = dr_ctx<BM, BN, WN>(p.k, p.k.B * p.k.S);  // no pad rows: the tail loads zeros
  const int l0 = ctx.l0, z0 = ctx.z0, wm = ctx.wm, wn = ctx.wn, lr = ctx.lr, lg = ctx.lg;
  const int q_begin = ctx.q_begin, q_end = ctx.q_end;
  const int tid = threadIdx.x;
  const int S = p.k.S, B = p.k.B, L = p.k.L, z = p.k.z;
  const bool evec = (z & 3) == 0;  // (G rows have the t_cols stride: whole float4s)

  f32x4 acc[TM][TN] = {};
  f32x4 rg[GV], re[EV];
  auto load = [&](int q0) {
#pragma unroll
    for (int v = 0; v < GV; ++v) {
      const int idx = tid + v * 256;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (idx < G4) {
        const int r = idx / (BM / 4), c = l0 + (idx % (BM / 4)) * 4;
        const int q = q0 + r;
        if (q < q_end) {
          const float* src = p.G + (int64_t)q * p.ldG;
          if (c < L) x = *reinterpret_cast<const f32x4*>(src + c);  // pads hold G = 0
        }
      }
      rg[v] = x;
    }
#pragma unroll
    for (int v = 0; v < EV; ++v) {
      const int idx = tid + v * 256;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (idx < E4) {
        const int r = idx / (BN / 4), c = z0 + (idx % (BN / 4)) * 4;
        const int q = q0 + r;
        if (q < q_end) {
          const int bb = q / S, s = q - bb * S;
          const float* src = p.eps + ((int64_t)s * B + bb) * z;
          if (evec && c + 3 < z) x = *reinterpret_cast<const f32x4*>(src + c);
          else {
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = (c + k < z) ? src[c + k] : 0.0f;
          }
        }
      }
      re[v] = x;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int v = 0; v < GV; ++v) {
      const int idx = tid + v * 256;
      if (idx < G4)
        *reinterpret_cast<f32x4*>(&Gs[(idx / (BM / 4)) * LDG + (idx % (BM / 4)) * 4]) = rg[v];
    }
#pragma unroll
    for (int v = 0; v < EV; ++v) {
      const int idx = tid + v * 256;
      if (idx < E4)
        *reinterpret_cast<f32x4*>(&Es[(idx / (BN / 4)) * LDE + (idx % (BN / 4)) * 4]) = re[v];
    }
  };

  if (q_begin < q_end) {
    load(q_begin);
    store();
    __syncthreads();
    for (int q0 = q_begin; q0 < q_end; q0 += kDrBK) {
      const bool more = q0 + kDrBK < q_end;
      if (more) load(q0 + kDrBK);
#pragma unroll
      for (int j = 0; j < kDrBK / 4; ++j) {
        float a[TM], bb[TN];
#pragma unroll
        for (int m = 0; m < TM; ++m) a[m] = Gs[(j * 4 + lg) * LDG + wm * TM * 16 + m * 16 + lr];
#pragma unroll
        for (int n = 0; n < TN; ++n) bb[n] = Es[(j * 4 + lg) * LDE + wn * TN * 16 + n * 16 + lr];
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
          for (int n = 0; n < TN; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], bb[n], acc[m][n], 0, 0, 0);
      }
      __syncthreads();
      if (more) {
        store();
        __syncthreads();
      }
    }
  }
  dr_store_slab<false>(acc, ctx, p.k);
}

// ------------------------------------------------------------------- plans
// A dR tile as the host sees it: its geometry, its split-K target and the
// kernel that computes it.
struct DrTile {
  int edge;                      // output tile edge, labels and latent columns alike
  int chunks_per_cu;             // split-K chunks per CU; 0: kDr32Blocks workgroups in all
  int threads;
  void (*kernel16)(Dr16Params);  // the 3xf16 kernel, or
  void (*kernel32)(DrParams);    // the fp32 one
};

constexpr int kDr32Blocks = 1536;            // fp32 dR: workgroups aimed at (several per CU)
constexpr int64_t kDrMaxChunkRows = 131072;  // longest split-K chunk (sample rows)

static DrTile pick_dr_tile(int64_t L, int64_t z, int gemm) {
  // fp32: 128 x 128, 4 waves of 64 x 64
  if (gemm != MPV_GEMM_F16X3) return {128, 0, 256, nullptr, dR_gemm_kernel<4, 4>};
  // Both <= 64 (mirflickr 38, the fairsoft adult-like 25 x 10): a 64 x 64 tile
  // (4 waves of 32 x 32, 2 x 16 KB stages), planes padded to 64 columns: half
  // the G-plane and noise-plane bytes of the 128 tile at L = z = 38.  Two K
  // chunks per CU (4 and 8 measure the same at C2)
  if (L <= 64 && z <= 64) return {64, 2, 256, dR16_kernel<2, 2, 2, 2>, nullptr};
  // Both <= 128 (nuswide 81): a 128 x 128 tile (4 waves of 64 x 64, 2 x 32 KB
  // stages, two workgroups per CU), so the G and noise planes are padded to
  // 128 columns instead of 256
  if (L <= 128 && z <= 128) return {128, 2, 256, dR16_kernel<2, 2, 4, 4>, nullptr};
  // 256 x 256, 8 waves of 128 x 64 in two groups one phase apart, 2 x 64 KB
  // stages: one workgroup per CU in a single wave of equal chunks
  return {256, 1, 512, dR16s_kernel<2, 4, 8, 4>, nullptr};
}

struct BwdPlan {
  DrTile tile;
  int TPR, RPI, nLc, nSc, rows_per_chunk, Lc;   // element pass
  int nLt, nZt, nKc, dr_rows_per_chunk, rows_pad;  // dR GEMM
  int64_t ldg;                                  // G plane columns (3xf16, padded)
  // the workspace's pieces (NULL from the sizing pass)
  float *coef, *colpart, *slab, *gbound;
  uint16_t* g16;  // G planes, chunked: rows_pad rows of 2 * ldg halves; 3xf16 only
};

static BwdPlan plan_bwd(Workspace& ws, const mpv_shape* s, int gemm) {
  BwdPlan pl;
  const int64_t L = s->L, S = s->S_local, B = s->B, z = s->z;
  const bool planes = gemm == MPV_GEMM_F16X3;
  pl.tile = pick_dr_tile(L, z, gemm);
  const int64_t dr_tile = pl.tile.edge;
  pl.ldg = cdiv(L, dr_tile) * dr_tile;
  // columns the element pass covers: L rounded up to whole 4-column lane
  // groups (the pad columns get G = 0).  The G planes' columns beyond are
  // never written: in the dR GEMM a G column l meets only output row l, and
  // rows >= L are not stored (round 5 wrote zeros up to the 32-wide chunk:
  // L = 38 covered 64 columns, 40 now -- C2's element pass does 38 % less)
  const int64_t Lc = planes ? std::min<int64_t>(pl.ldg, cdiv(L, 4) * 4) : L;
  pl.Lc = (int)Lc;
  pl.nLc = (int)cdiv(Lc, 1024);
  pl.TPR = (int)(Lc >= 1024 ? 256 : cdiv(Lc, 4));
  pl.RPI = 256 / pl.TPR;
  // s-chunks: enough blocks for several rounds of resident blocks (short tail)
  int64_t want = cdiv(8192, B * pl.nLc);
  // but at least kElemMinRows rows per thread (block setup amortised; the
  // LDS-ring kernel, with its coefficient staging and ring prologue per block,
  // kElemRingMinRows, which matters at small n_sample: the strong-scaling share)
  const int64_t min_rows = (planes && pl.RPI == 1) ? kElemRingMinRows : kElemMinRows;
  want = std::min<int64_t>(want, cdiv(S, (int64_t)pl.RPI * min_rows));
  // but two blocks per CU at least when a thread still gets kElemMinRows / 2
  // rows (C2: 384 blocks, 1.5 per CU, left half the CUs with one wave per
  // SIMD: element pass 24.9 -> 22.3 us with 512; C3 has 2816 either way)
  const int64_t even = cdiv(2 * (int64_t)num_cus(), B * pl.nLc);
  if (want < even && cdiv(S, even * pl.RPI) >= kElemMinRows / 2) want = even;
  if (want < 1) want = 1;
  const int64_t max_chunks = cdiv(S, pl.RPI);
  if (want > max_chunks) want = max_chunks;
  pl.rows_per_chunk = (int)cdiv(S, want);
  pl.nSc = (int)cdiv(S, pl.rows_per_chunk);
  pl.nLt = (int)cdiv(L, dr_tile);
  pl.nZt = (int)cdiv(z, dr_tile);
  const int64_t rows = B * S;
  const int64_t tiles = (int64_t)pl.nLt * pl.nZt;
  const int64_t kr = 32;  // K rows per stage of either GEMM
  pl.rows_pad = (int)(cdiv(rows, kr) * kr);
  // split-K chunks: the workgroups the tile aims at (pick_dr_tile) over its tiles
  const int cpc = pl.tile.chunks_per_cu;
  int64_t kc = cdiv(cpc ? cpc * (int64_t)num_cus() : kDr32Blocks, tiles);
  // but no K chunk longer than kDrMaxChunkRows: one fp32 accumulator per output
  // over 4.2 M rows (C5 on one GPU: 256 tiles, so one chunk each) drifted 1e-4
  // (normwise) between two shardings of the same sum; chunks of <= 128 K rows
  // keep it at the C4 level (< 1e-5), the chunks summed in a fixed order
  kc = std::max<int64_t>(kc, cdiv(rows, kDrMaxChunkRows));
  const int64_t kc_max = cdiv(rows, 256);
  if (kc > kc_max) kc = kc_max;
  if (kc < 1) kc = 1;
  pl.dr_rows_per_chunk = (int)(cdiv(cdiv(rows, kc), kr) * kr);
  pl.nKc = (int)cdiv(rows, pl.dr_rows_per_chunk);
  pl.coef = ws.take<float>(6, B, S);
  pl.colpart = ws.take<float>(pl.nSc, 2, B, L);
  pl.slab = ws.take<float>(pl.nKc, L, z);
  pl.gbound = ws.take<float>(B + 64);
  pl.g16 = ws.take<uint16_t>(planes ? 2 : 0, pl.rows_pad, pl.ldg);
  return pl;
}

}  // namespace mpv

using namespace mpv;

extern "C" {

int64_t mpv_noise_plane_cols(const mpv_shape* shape) {
  if (check_shape(shape) != MPV_OK) return 0;
  const int64_t t = pick_dr_tile(shape->L, shape->z, MPV_GEMM_F16X3).edge;
  return cdiv(shape->z, t) * t;
}

size_t mpv_bwd_workspace_bytes(const mpv_shape* shape, int gemm) {
  if (check_shape(shape) != MPV_OK) return 0;
  return layout_bytes(plan_bwd, shape, gemm);
}

int mpv_probit_bwd(const mpv_shape* shape, const mpv_bwd_args* a, void* stream) {
  if (int rc = check_shape(shape)) return rc;
  MPV_REQUIRE(a && a->y && a->fe_out && a->fx_out && a->T && a->rowstat && a->bstat &&
                  a->gscal && a->dfe_dfx && a->workspace,
              "NULL pointer in mpv_bwd_args");
  MPV_REQUIRE(a->gemm == MPV_GEMM_F32 || a->gemm == MPV_GEMM_F16X3, "unknown gemm mode %d",
              a->gemm);
  const bool planes = a->gemm == MPV_GEMM_F16X3;
  Workspace carve(a->workspace);
  const BwdPlan pl = plan_bwd(carve, shape, a->gemm);
  MPV_REQUIRE(!(a->dR32 && a->dR64), "dR32 or dR64, not both");
  void* const dR_out = a->dR64 ? (void*)a->dR64 : (void*)a->dR32;
  const int dR_dtype = a->dR64 ? MPV_F64 : MPV_F32;
  if (a->kl) {
    MPV_REQUIRE(a->kl->fe_mu && a->kl->fe_logvar && a->kl->fx_mu && a->kl->fx_logvar &&
                    a->kl->gscal && a->kl->g_fe_mu && a->kl->g_fe_logvar && a->kl->g_fx_mu &&
                    a->kl->g_fx_logvar && a->kl->B > 0 && a->kl->d > 0,
                "bad kl arguments");
  }
  if (dR_out) {
    if (planes) {
      MPV_REQUIRE(a->eps16.data && a->eps16.scale, "eps16 planes are NULL");
      MPV_REQUIRE(a->eps16.ld >= 2 * (int64_t)pl.nZt * pl.tile.edge && a->eps16.ld % 64 == 0 &&
                      a->eps16.rows_pad >= shape->S_local * shape->B,
                  "eps16 planes too small (ld %lld < %lld: mpv_noise_plane_cols)",
                  (long long)a->eps16.ld, 2 * (long long)pl.nZt * pl.tile.edge);
    } else {
      MPV_REQUIRE(a->eps != nullptr, "MPV_GEMM_F32 needs eps");
    }
  }
  MPV_REQUIRE(carve.fits(a->workspace_bytes), "workspace too small: %zu < %zu",
              a->workspace_bytes, carve.bytes());
  hipStream_t st = as_stream(stream);
  const int64_t gld = 2 * pl.ldg;
  const int S = (int)shape->S_local, B = (int)shape->B, L = (int)shape->L, z = (int)shape->z;
  const bool want_planes = planes && dR_out != nullptr;

  mpv_kl_bwd_args kl{};
  int kl_blocks = 0;
  if (a->kl) {
    kl = *a->kl;
    kl_blocks = (int)std::min<int64_t>(cdiv(kl.B * kl.d, kCoefThreads), 256);
  }
  MPV_LAUNCH("bwd_coef", bwd_coef_kernel, dim3(B + kl_blocks), dim3(kCoefThreads), 0, st, a->y, a->rowstat,
             a->bstat, a->gscal, a->g_indiv, a->g_indiv_label, pl.coef,
             want_planes ? pl.gbound : nullptr, S, B, L, (float)shape->S_total, a->nll_coeff,
             a->c_coeff, a->live, kl, kl_blocks);
  if (want_planes) {
    const int64_t pad_rows = (int64_t)pl.rows_pad - (int64_t)B * S;
    if (pad_rows > 0) {
      const size_t off = (size_t)B * S * gld, n = (size_t)pad_rows * gld * sizeof(uint16_t);
      if (hipMemsetAsync(pl.g16 + off, 0, n, st) != hipSuccess)
        return fail(MPV_ELAUNCH, "memset of G pad rows failed");
    }
  }

  const ElemParams ep{a->y, a->fe_out, a->fx_out, a->g_indiv, a->g_indiv_label, pl.coef, a->T,
                      want_planes ? pl.g16 : nullptr, pl.gbound, gld, pl.colpart, S, B, L,
                      want_planes ? pl.Lc : L, (int)t_cols(L), pl.TPR, pl.RPI, pl.rows_per_chunk,
                      1.0f / (float)shape->S_total};
  const dim3 eg(B, pl.nSc, pl.nLc);
  // t_cols rows: 16-B aligned, whole float4 reads
  if (want_planes && pl.RPI == 1)  // L >= 1024: the LDS-ring element pass
    MPV_LAUNCH("bwd_elem", bwd_elem_ring_kernel, eg, dim3(256), 0, st, ep);
  else if (want_planes)
    MPV_LAUNCH("bwd_elem", bwd_elem_kernel<true>, eg, dim3(256), 0, st, ep);
  else
    MPV_LAUNCH("bwd_elem", bwd_elem_kernel<false>, eg, dim3(256), 0, st, ep);
  if (!dR_out) {
    if (int rc = launch_sum_slabs(pl.colpart, pl.nSc, 2 * (int64_t)B * L, a->dfe_dfx, MPV_F32, st))
      return rc;
  }

  if (dR_out) {
    const dim3 grid((unsigned)((int64_t)pl.nLt * pl.nZt * pl.nKc)), block(pl.tile.threads);
    const DrCommon dc{pl.slab, S, B, L, z, pl.nLt, pl.nZt, pl.nKc, pl.dr_rows_per_chunk};
    if (planes) {
      const Dr16Params dp{pl.g16, pl.gbound, gld, a->eps16, dc, pl.rows_pad};
      MPV_LAUNCH("dR_gemm", pl.tile.kernel16, grid, block, 0, st, dp);
    } else {
      const DrParams dp{a->T, a->eps, dc, (int)t_cols(L)};
      MPV_LAUNCH("dR_gemm", pl.tile.kernel32, grid, block, 0, st, dp);
    }
    // the column partials (d fe_out, d fx_out) and the dR slabs in one launch
    if (int rc = launch_sum_slabs_pair(pl.colpart, pl.nSc, 2 * (int64_t)B * L, a->dfe_dfx, MPV_F32,
                                       pl.slab, pl.nKc, (int64_t)L * z, dR_out, dR_dtype, st))
      return rc;
  }
  return MPV_OK;
}

}  // extern "C"
