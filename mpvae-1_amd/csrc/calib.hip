// Post-process threshold calibration (fairsoft_train_postprocess.py): one
// decision threshold per (label, sensitive group) learned on a frozen model.
//
//   calib_fwd_kernel     calibrate_p (:39-49) with the threshold of the row's
//                        group, the BCE of the calibrated probabilities
//                        (:117-126) and the per-slice partial sums behind the
//                        fairness term's weighted means (:128-161);
//   calib_tables_kernel  the weight sums, the group and batch means, the
//                        squared-distance penalty, the number of active
//                        (target, group) terms and the backward's tables;
//   calib_bwd_kernel     d (g_bce bce + g_fair fair) / d threshold_ and, on
//                        request, / d indiv_prob (autograd through the same
//                        lines), the threshold's as per-slice partials;
//   calib_dx_kernel      their sum over the slices.
//
// Grid of the forward and the backward: (label chunk of 256) x (group k) x
// (row slice r of R).  Block (., k, r) walks its share of the positions
// goff[k] .. goff[k+1] of `order`, found on the device, so the grid is host
// knowledge.  fp64 arithmetic from fp32 inputs, in the reference's forms.  No
// floating-point atomics: every sum runs in an order fixed by (B, L, T, G, R,
// goff), so two calls on the same inputs give the same bits.
#include "abi_util.h"
#include "mpv_common.h"

namespace mpv {

constexpr int kCalThreads = 256;
constexpr int kCalTile = 4;       // targets whose sums a thread holds in registers at once
constexpr double kCalEps = 1e-6;  // the reference's 1e-6 (logit, the BCE logs)

// Workspace.
struct CalibWs {
  double* bpart;   // (NLB, G, R)   BCE partials
  double* wpart;   // (T, G, R)     sum of w over the slice's rows
  double* qpart;   // (T, G, R, L)  sum of w q
  double* wsum;    // (T, G + 1)    W_tk, and W_t at k = G
  double* dtab;    // (T, G, L)     2 (m_tk - m_t) / W_tk
  double* etab;    // (T, L)        sum_k 2 (m_tk - m_t) / W_t
  double* dxpart;  // (G, R, L)     d threshold partials
};

static CalibWs calib_ws(Workspace& ws, int64_t L, int64_t T, int64_t G, int64_t R) {
  CalibWs c;
  c.bpart = ws.take<double>(cdiv(L, kCalThreads), G, R);
  c.wpart = ws.take<double>(T, G, R);
  c.qpart = ws.take<double>(T, G, R, L);
  c.wsum = ws.take<double>(T, G + 1);
  c.dtab = ws.take<double>(T, G, L);
  c.etab = ws.take<double>(T, L);
  c.dxpart = ws.take<double>(G, R, L);
  return c;
}

static bool calib_shape_ok(int64_t L, int64_t T, int64_t G) { return L >= 1 && T >= 0 && G >= 1; }

// The threshold of (label l, group k) and what the calibration needs of it:
// c = logit(thr) (:40), and for the backward d c / d threshold_.
struct CalibThr {
  double c, dc;
};
MPV_DEV CalibThr calib_thr(double x, int learn_logit) {
  double thr = x, dthr = 1.0;
  if (learn_logit) {  // sigmoid (:43-44) and its derivative e^-x thr^2
    const double ex = exp(-x);
    thr = 1.0 / (ex + 1.0);
    dthr = ex * thr * thr;
  }
  const double om = 1.0 - thr + kCalEps;
  // outside (0, 1) the log is NaN and stays NaN (the finite gate skips the update)
  return CalibThr{log(thr / om), (1.0 / thr + 1.0 / om) * dthr};
}

// cal_prob = sigmoid(logit(p) - c) (:47-49); e = exp(-(a - c)), so that
// d q / d a = e q^2, the form autograd differentiates.
MPV_DEV double calib_q(double p, double c, double& e) {
  const double a = log(p / (1.0 - p + kCalEps));
  e = exp(-(a - c));
  return 1.0 / (e + 1.0);
}

__global__ __launch_bounds__(kCalThreads) void calib_fwd_kernel(mpv_calib_args a, CalibWs ws) {
  __shared__ double red[kCalThreads / 64];
  const int L = (int)a.L, B = (int)a.B, T = (int)a.T, G = (int)a.G, R = (int)a.R;
  const int k = blockIdx.y, r = blockIdx.z;
  const int l = blockIdx.x * kCalThreads + threadIdx.x;
  int j0, j1;
  group_slice(a.goff, k, r, R, B, j0, j1);
  double bce = 0.0;
  if (l < L) {
    const bool cal = a.threshold != nullptr;  // else p is already calibrated
    const double c = cal ? calib_thr((double)a.threshold[(int64_t)l * G + k], a.learn_logit).c : 0.0;
    // kCalTile targets per pass over the slice; the first pass also stores
    // cal_prob and sums the BCE (T = 0: that pass alone)
    for (int t0 = 0; t0 < max(T, 1); t0 += kCalTile) {
      double acc[kCalTile] = {0.0, 0.0, 0.0, 0.0}, wacc[kCalTile] = {0.0, 0.0, 0.0, 0.0};
      for (int j = j0; j < j1; ++j) {
        const int b = a.order[j];
        if ((unsigned)b >= (unsigned)B) continue;
        const int64_t i = (int64_t)b * L + l;
        double e;
        const double q = cal ? calib_q((double)a.p[i], c, e) : (double)a.p[i];
        if (t0 == 0) {
          if (a.cal_prob != nullptr) a.cal_prob[i] = (float)q;
          if (a.y != nullptr) {
            const double y = (double)a.y[i];
            bce -= y * log(q + kCalEps) + (1.0 - y) * log(1.0 - q + kCalEps);
          }
        }
#pragma unroll
        for (int u = 0; u < kCalTile; ++u) {
          if (t0 + u < T) {
            const double w = a.w[(int64_t)(t0 + u) * B + b];
            acc[u] += w * q;
            wacc[u] += w;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kCalTile; ++u) {
        if (t0 + u < T) {
          const int64_t s = ((int64_t)(t0 + u) * G + k) * R + r;
          ws.qpart[s * L + l] = acc[u];
          if (l == 0) ws.wpart[s] = wacc[u];
        }
      }
    }
  }
  bce = block_sum_f64<kCalThreads / 64>(bce, red);
  if (threadIdx.x == 0) ws.bpart[((int64_t)blockIdx.x * G + k) * R + r] = bce;
}

// One block.  out = [bce, fair, number of active (t, k) terms].
__global__ __launch_bounds__(kCalThreads) void calib_tables_kernel(mpv_calib_args a, CalibWs ws,
                                                                   int nlb) {
  __shared__ double red[kCalThreads / 64];
  const int L = (int)a.L, T = (int)a.T, G = (int)a.G, R = (int)a.R;
  const int tid = threadIdx.x;
  slice_weight_sums(ws.wpart, ws.wsum, T, G, R);
  double pen = 0.0;
  for (int l = tid; l < L; l += kCalThreads) {
    for (int t = 0; t < T; ++t) {
      const double Wt = ws.wsum[t * (G + 1) + G];
      double esum = 0.0;
      if (Wt > 0.0) {  // :147 `if weights.sum() > 0`
        double tot = 0.0;
        for (int i = 0; i < G * R; ++i) tot += ws.qpart[((int64_t)t * G * R + i) * L + l];
        const double mt = tot / Wt;
        for (int k = 0; k < G; ++k) {
          const double Wk = ws.wsum[t * (G + 1) + k];
          double fp = 0.0;
          if (Wk > 0.0) {  // :157 `if weight_sensitive.sum() > 0`
            double s = 0.0;
            for (int r = 0; r < R; ++r) s += ws.qpart[(((int64_t)t * G + k) * R + r) * L + l];
            fp = fair_pair_step(s, Wk, mt, MPV_FAIR_L2, pen, esum);
          }
          ws.dtab[((int64_t)t * G + k) * L + l] = fp;
        }
        esum /= Wt;
      } else {
        for (int k = 0; k < G; ++k) ws.dtab[((int64_t)t * G + k) * L + l] = 0.0;
      }
      ws.etab[(int64_t)t * L + l] = esum;
    }
  }
  pen = block_sum_f64<kCalThreads / 64>(pen, red);
  double bce = 0.0;
  for (int i = tid; i < nlb * G * R; i += kCalThreads) bce += ws.bpart[i];
  bce = block_sum_f64<kCalThreads / 64>(bce, red);
  if (tid == 0) {
    int nterms = 0;
    for (int t = 0; t < T; ++t) {
      if (!(ws.wsum[t * (G + 1) + G] > 0.0)) continue;
      for (int k = 0; k < G; ++k) nterms += ws.wsum[t * (G + 1) + k] > 0.0 ? 1 : 0;
    }
    a.out[0] = bce / (double)a.B;  // :126 `.sum(1).mean()`
    a.out[1] = pen;
    a.out[2] = (double)nterms;
  }
}

__global__ __launch_bounds__(kCalThreads) void calib_bwd_kernel(mpv_calib_args a, CalibWs ws,
                                                                const double* __restrict__ gout,
                                                                float* __restrict__ g_p) {
  const int L = (int)a.L, B = (int)a.B, T = (int)a.T, G = (int)a.G, R = (int)a.R;
  const int k = blockIdx.y, r = blockIdx.z;
  const int l = blockIdx.x * kCalThreads + threadIdx.x;
  if (l >= L) return;
  int j0, j1;
  group_slice(a.goff, k, r, R, B, j0, j1);
  const CalibThr th = calib_thr((double)a.threshold[(int64_t)l * G + k], a.learn_logit);
  const double gb = a.y != nullptr ? gout[0] / (double)B : 0.0, gf = gout[1];
  // D[t, k, l] - E[t, l] of the first kCalTile targets in registers
  double de[kCalTile];
#pragma unroll
  for (int u = 0; u < kCalTile; ++u)
    de[u] = u < T ? ws.dtab[((int64_t)u * G + k) * L + l] - ws.etab[(int64_t)u * L + l] : 0.0;
  double acc = 0.0;
  for (int j = j0; j < j1; ++j) {
    const int b = a.order[j];
    if ((unsigned)b >= (unsigned)B) continue;
    const int64_t i = (int64_t)b * L + l;
    const double p = (double)a.p[i];
    double e;
    const double q = calib_q(p, th.c, e);
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < kCalTile; ++u)
      if (u < T) s += a.w[(int64_t)u * B + b] * de[u];
    for (int t = kCalTile; t < T; ++t)
      s += a.w[(int64_t)t * B + b] *
           (ws.dtab[((int64_t)t * G + k) * L + l] - ws.etab[(int64_t)t * L + l]);
    double dq = gf * s;
    if (a.y != nullptr) {
      const double y = (double)a.y[i];
      dq += gb * (-y / (q + kCalEps) + (1.0 - y) / (1.0 - q + kCalEps));
    }
    const double da = dq * e * q * q;  // d / d logit(p); d / d c is its negative
    acc -= da;
    if (g_p != nullptr) g_p[i] = (float)(da * (1.0 / p + 1.0 / (1.0 - p + kCalEps)));
  }
  // 0 * c: a threshold whose logit is NaN poisons its own gradient entry even
  // when no row used it, as autograd through the reference's full (B, L, G)
  // cal_prob does
  ws.dxpart[((int64_t)k * R + r) * L + l] = acc * th.dc + 0.0 * th.c;
}

// g_threshold[l, k] = sum_r dxpart[k, r, l], r in order.
__global__ void calib_dx_kernel(CalibWs ws, int L, int G, int R, float* __restrict__ g_threshold) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)L * G) return;
  const int l = (int)(i / G), k = (int)(i % G);
  double s = 0.0;
  for (int r = 0; r < R; ++r) s += ws.dxpart[((int64_t)k * R + r) * L + l];
  g_threshold[i] = (float)s;
}

}  // namespace mpv

using namespace mpv;

extern "C" {

size_t mpv_calib_workspace_bytes(int64_t L, int64_t T, int64_t G, int64_t R) {
  if (!calib_shape_ok(L, T, G) || R < 1) return 0;
  return layout_bytes(calib_ws, L, T, G, R);
}

static int calib_check(const mpv_calib_args* a, void* workspace, size_t workspace_bytes,
                       CalibWs* ws) {
  MPV_REQUIRE(a != nullptr, "mpv_calib_args is NULL");
  MPV_REQUIRE(a->p != nullptr, "NULL p in mpv_calib_args");
  MPV_REQUIRE(a->B >= 1 && calib_shape_ok(a->L, a->T, a->G),
              "bad calibration shape B=%lld L=%lld T=%lld G=%lld", (long long)a->B,
              (long long)a->L, (long long)a->T, (long long)a->G);
  MPV_REQUIRE(a->R >= 1, "calibration row slices R must be >= 1 (got %lld)", (long long)a->R);
  MPV_REQUIRE(a->B < (int64_t(1) << 31) && a->L < (int64_t(1) << 31) && a->G <= 65535 &&
                  a->R <= 65535 && a->T * a->G * a->R < (int64_t(1) << 31),
              "calibration shape too large");
  MPV_REQUIRE(a->order && a->goff, "NULL order / goff in mpv_calib_args");
  MPV_REQUIRE(a->T == 0 || a->w != nullptr, "NULL w with T > 0");
  Workspace carve(workspace);
  *ws = calib_ws(carve, a->L, a->T, a->G, a->R);
  MPV_REQUIRE(carve.fits(workspace_bytes), "calibration workspace too small");
  return MPV_OK;
}

int mpv_calib_fwd(const mpv_calib_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  CalibWs ws;
  if (int rc = calib_check(a, workspace, workspace_bytes, &ws)) return rc;
  MPV_REQUIRE(a->out != nullptr, "NULL out in mpv_calib_args");
  hipStream_t st = as_stream(stream);
  const int nlb = (int)cdiv(a->L, kCalThreads);
  MPV_LAUNCH("calib_fwd", calib_fwd_kernel, dim3(nlb, (unsigned)a->G, (unsigned)a->R),
             dim3(kCalThreads), 0, st, *a, ws);
  MPV_LAUNCH("calib_tables", calib_tables_kernel, dim3(1), dim3(kCalThreads), 0, st, *a, ws, nlb);
  return MPV_OK;
}

int mpv_calib_bwd(const mpv_calib_args* a, const double* gout, float* g_threshold, float* g_p,
                  void* workspace, size_t workspace_bytes, void* stream) {
  CalibWs ws;
  if (int rc = calib_check(a, workspace, workspace_bytes, &ws)) return rc;
  MPV_REQUIRE(a->threshold != nullptr, "mpv_calib_bwd needs a threshold");
  MPV_REQUIRE(gout && g_threshold, "NULL gout / g_threshold in mpv_calib_bwd");
  hipStream_t st = as_stream(stream);
  const int nlb = (int)cdiv(a->L, kCalThreads);
  MPV_LAUNCH("calib_bwd", calib_bwd_kernel, dim3(nlb, (unsigned)a->G, (unsigned)a->R),
             dim3(kCalThreads), 0, st, *a, ws, gout, g_p);
  MPV_LAUNCH("calib_bwd", calib_dx_kernel, dim3((unsigned)cdiv(a->L * a->G, 256)), dim3(256), 0, st,
             ws, (int)a->L, (int)a->G, (int)a->R, g_threshold);
  return MPV_OK;
}

}  // extern "C"
