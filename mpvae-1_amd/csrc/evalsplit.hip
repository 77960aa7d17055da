// The evaluation pass over a whole split (fairsoft_evaluate.py:83-121): from the
// (N, L) buffer of indiv_prob, the labels and the row weights of every target,
//
//   split_eval_kernel   the "soft" tp / fp / fn of evals.compute_tp_fp_fn applied
//                       to probabilities (evals.py:61-67) and, per target, the
//                       weight sums and the weighted sums of the probabilities,
//                       all as per-slice partials;
//   split_final_kernel  one workgroup: the partials summed slice by slice, the
//                       counts, miF1 / maF1 (evals.py:99-109), the group and
//                       split means, the squared distance of every active
//                       (target, group) pair and the means of the distances
//                       (:106-121) and of their squares
//                       (fairsoft_train_postprocess.py:444).
//
// mpv_split_eval_defs scores the same buffer under D definitions of the row
// weights (the distance sweep of fairsoft_metric.py): split_eval sees D * T
// targets, split_final takes the two means per definition, each as the call
// on that definition alone takes them; mpv_split_eval is D = 1.
//
// Grid of split_eval: (label chunk) x (group k) x (row slice r of R).  A
// workgroup's 256 lanes are (row, label) pairs: `lp` lanes along the labels
// (the power of two >= L when L <= 32, else one 64-label chunk: a 256-B row
// read per wave) and 256 / lp rows at once, so that a split of 10^4 - 10^5 rows
// at 20 - 40 labels fills the waves.  The rows of a slice are summed per lane,
// then over the lanes of a wave in a fixed shuffle tree, then over the waves
// in order.  fp64 arithmetic from the fp32 inputs; no floating-point atomics:
// every sum runs in an order fixed by (N, L, T, G, R, goff), so two calls on the
// same inputs give the same bits.
//
// Targets are held kEvalTile at a time in registers.  The first tile's pass
// over the slice also makes the counts, so one read of pred and target serves
// everything up to kEvalTile targets; each further tile reads pred (not
// target) and its own weights again.
#include "abi_util.h"
#include "mpv_common.h"

namespace mpv {

constexpr int kEvalThreads = 256;
constexpr int kEvalWaves = kEvalThreads / 64;
constexpr int kEvalTile = 4;                 // targets whose sums a lane holds at once
constexpr int kEvalVals = 3 + 2 * kEvalTile;  // tp, fp, fn, then (sum w p, sum w) per target
constexpr double kEvalEps = 1e-6;            // evals.py:109

// Workspace.
struct EvalWs {
  double* cpart;  // (G, R, 3, L)  tp / fp / fn partials
  double* wpart;  // (T, G, R)     sum of w over the slice's rows
  double* qpart;  // (T, G, R, L)  sum of w p
  double* wsum;   // (T, G + 1)    W_tk, and W_t at k = G
  double* gsum;   // (T, G, L)     sum_r qpart
  double* csum;   // (G, 3, L)     sum_r cpart
  double* mtab;   // (T, L)        m_t
};

static EvalWs eval_ws(Workspace& ws, int64_t L, int64_t T, int64_t G, int64_t R) {
  EvalWs c;
  c.cpart = ws.take<double>(G, R, 3, L);
  c.wpart = ws.take<double>(T, G, R);
  c.qpart = ws.take<double>(T, G, R, L);
  c.wsum = ws.take<double>(T, G + 1);
  c.gsum = ws.take<double>(T, G, L);
  c.csum = ws.take<double>(G, 3, L);
  c.mtab = ws.take<double>(T, L);
  return c;
}

// T targets in each of D >= 1 definitions, at most 2^20 in all.
static bool split_shape_ok(int64_t N, int64_t L, int64_t T, int64_t D, int64_t G) {
  return N > 0 && N < (int64_t(1) << 31) && L > 0 && L <= 4096 && T >= 0 &&
         T <= (int64_t(1) << 20) / D && G >= 1 && G <= 65535;
}
static bool split_slices_ok(int64_t R) { return R >= 1 && R <= 65535; }

// Lanes along the labels: the power of two >= L up to 32, else 64.
static int eval_lanes(int64_t L) {
  if (L > 32) return 64;
  int lp = 1;
  while (lp < L) lp *= 2;
  return lp;
}

// The sums of v[] over the lanes that share a label, in a fixed order: the
// rows of a wave by a shuffle tree, then the waves in order.  Threads
// 0 .. lp - 1 hold the result.
MPV_DEV void eval_block_sum(double (&v)[kEvalVals], int lp, double* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 32; o >= lp; o >>= 1) {
#pragma unroll
    for (int i = 0; i < kEvalVals; ++i) v[i] += __shfl_xor(v[i], o, 64);
  }
  __syncthreads();  // `red` may still be read from the tile before
  if (lane < lp) {
#pragma unroll
    for (int i = 0; i < kEvalVals; ++i) red[(i * kEvalWaves + wv) * 64 + lane] = v[i];
  }
  __syncthreads();
  if ((int)threadIdx.x < lp) {
#pragma unroll
    for (int i = 0; i < kEvalVals; ++i) {
      double s = 0.0;
      for (int w = 0; w < kEvalWaves; ++w) s += red[(i * kEvalWaves + w) * 64 + threadIdx.x];
      v[i] = s;
    }
  }
}

__global__ __launch_bounds__(kEvalThreads) void split_eval_kernel(mpv_split_eval_args a, EvalWs ws,
                                                                  int lp) {
  __shared__ double red[kEvalVals * kEvalWaves * 64];
  const int L = (int)a.L, N = (int)a.N, T = (int)a.T, G = (int)a.G, R = (int)a.R;
  const int k = blockIdx.y, r = blockIdx.z;
  const int tid = threadIdx.x;
  const int l = blockIdx.x * lp + (tid & (lp - 1));
  const int row = tid / lp, rows = kEvalThreads / lp;
  const bool live = l < L;
  int j0, j1;
  group_slice(a.goff, k, r, R, N, j0, j1);
  for (int t0 = 0; t0 < max(T, 1); t0 += kEvalTile) {
    double v[kEvalVals];
#pragma unroll
    for (int i = 0; i < kEvalVals; ++i) v[i] = 0.0;
    for (int j = j0 + row; j < j1; j += rows) {
      const int b = a.order != nullptr ? a.order[j] : j;
      if ((unsigned)b >= (unsigned)N || !live) continue;
      const int64_t i = (int64_t)b * L + l;
      const double p = (double)a.pred[i];
      if (t0 == 0) {
        const double y = (double)a.target[i];
        v[0] += y * p;                          // evals.py:62
        v[1] += (y == 0.0 ? 1.0 : 0.0) * p;     // :63, logical_not of a float
        v[2] += y * (p == 0.0 ? 1.0 : 0.0);     // :65
      }
#pragma unroll
      for (int u = 0; u < kEvalTile; ++u) {
        if (t0 + u < T) {
          const double w = a.w[(int64_t)(t0 + u) * N + b];
          v[3 + 2 * u] += w * p;
          v[4 + 2 * u] += w;
        }
      }
    }
    eval_block_sum(v, lp, red);
    if (tid < lp && live) {
      if (t0 == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ws.cpart[(((int64_t)k * R + r) * 3 + c) * L + l] = v[c];
      }
#pragma unroll
      for (int u = 0; u < kEvalTile; ++u) {
        if (t0 + u < T) {
          const int64_t s = ((int64_t)(t0 + u) * G + k) * R + r;
          ws.qpart[s * L + l] = v[3 + 2 * u];
          if (l == 0) ws.wpart[s] = v[4 + 2 * u];
        }
      }
    }
  }
}

// One block.  The workspace's tables are written and read back by this block
// alone, with a barrier between the phases.
//
// `a.T` targets are D definitions of a.T / D targets each: everything up to
// terms[] is per target, and the means over a definition's (target, group)
// pairs walk them as a call on that definition alone would (thread tid takes
// pairs tid, tid + 256, ... of the definition, then the block sum), so each
// definition's three numbers carry the bits of its own call.  out_defs NULL
// (D = 1): they go to a.out[2..4]; else to out_defs[d * 3 ..], and a.out[2..4]
// hold definition 0's.
__global__ __launch_bounds__(kEvalThreads) void split_final_kernel(mpv_split_eval_args a,
                                                                   EvalWs ws, int D,
                                                                   double* __restrict__ out_defs) {
  __shared__ double red[kEvalWaves];
  const int64_t L = a.L, T = a.T, G = a.G, R = a.R;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  slice_weight_sums(ws.wpart, ws.wsum, T, G, R);
  // the slices of every (t, k, l) and (k, c, l), r in order
  for (int64_t i = tid; i < T * G * L; i += kEvalThreads) {
    const int64_t tk = i / L, l = i % L;
    double s = 0.0;
    for (int64_t r = 0; r < R; ++r) s += ws.qpart[(tk * R + r) * L + l];
    ws.gsum[i] = s;
  }
  for (int64_t i = tid; i < G * 3 * L; i += kEvalThreads) {
    const int64_t k = i / (3 * L), cl = i % (3 * L);
    double s = 0.0;
    for (int64_t r = 0; r < R; ++r) s += ws.cpart[(k * R + r) * 3 * L + cl];
    ws.csum[i] = s;
  }
  __syncthreads();
  // m_t and the counts, k in order
  for (int64_t i = tid; i < T * L; i += kEvalThreads) {
    const int64_t t = i / L, l = i % L;
    double s = 0.0;
    for (int64_t k = 0; k < G; ++k) s += ws.gsum[(t * G + k) * L + l];
    ws.mtab[i] = s / ws.wsum[t * (G + 1) + G];
  }
  for (int64_t i = tid; i < 3 * L; i += kEvalThreads) {
    double s = 0.0;
    for (int64_t k = 0; k < G; ++k) s += ws.csum[k * 3 * L + i];
    a.counts[i] = s;
  }
  __syncthreads();
  // terms[t, k], a wave per pair: fairsoft_evaluate.py:106 `if weights.sum() > 0`,
  // :115 `if weights_sensitive.sum() > 0`
  for (int64_t i = wv; i < T * G; i += kEvalWaves) {
    const int64_t t = i / G, k = i % G;
    const double Wt = ws.wsum[t * (G + 1) + G], Wk = ws.wsum[t * (G + 1) + k];
    double s = 0.0;
    if (Wt > 0.0 && Wk > 0.0) {
      for (int64_t l = lane; l < L; l += 64) {
        const double d = ws.gsum[i * L + l] / Wk - ws.mtab[t * L + l];
        s += d * d;
      }
    }
    s = wave_sum(s);
    if (lane == 0) a.terms[i] = (Wt > 0.0 && Wk > 0.0) ? s : nan;
  }
  __syncthreads();
  const int64_t per = T / D * G;  // (target, group) pairs of one definition
  for (int d = 0; d < D; ++d) {
    double dist = 0.0, sq = 0.0, cnt = 0.0;
    for (int64_t i = tid; i < per; i += kEvalThreads) {
      const double v = a.terms[d * per + i];
      if (v == v) {
        dist += sqrt(v);  // :118-119
        sq += v;
        cnt += 1.0;
      }
    }
    dist = block_sum_f64<kEvalWaves>(dist, red);
    sq = block_sum_f64<kEvalWaves>(sq, red);
    cnt = block_sum_f64<kEvalWaves>(cnt, red);
    if (tid == 0) {
      double* o = out_defs != nullptr ? out_defs + 3 * d : a.out + 2;
      o[0] = dist / cnt;  // np.mean([]) is NaN
      o[1] = sq / cnt;
      o[2] = cnt;
      if (out_defs != nullptr && d == 0) {
        a.out[2] = o[0];
        a.out[3] = o[1];
        a.out[4] = o[2];
      }
    }
  }
  double tp = 0.0, fp = 0.0, fn = 0.0, f1 = 0.0, nf = 0.0;
  for (int64_t l = tid; l < L; l += kEvalThreads) {
    const double t = a.counts[l], p = a.counts[L + l], n = a.counts[2 * L + l];
    tp += t;
    fp += p;
    fn += n;
    const double v = 2.0 * t / (2.0 * t + p + n + kEvalEps);  // evals.py:109
    if (isfinite(v)) {                                        // safe_div, :104-108
      f1 += v;
      nf += 1.0;
    }
  }
  tp = block_sum_f64<kEvalWaves>(tp, red);
  fp = block_sum_f64<kEvalWaves>(fp, red);
  fn = block_sum_f64<kEvalWaves>(fn, red);
  f1 = block_sum_f64<kEvalWaves>(f1, red);
  nf = block_sum_f64<kEvalWaves>(nf, red);
  if (tid == 0) {
    a.out[0] = 2.0 * tp / (2.0 * tp + fp + fn);  // evals.py:99-100
    a.out[1] = f1 / nf;                          // np.mean of the kept labels; none: NaN
  }
}

}  // namespace mpv

using namespace mpv;

// mpv_split_eval (D = 1, out_defs NULL) and mpv_split_eval_defs: `a->T` targets
// in each of D definitions, laid out as D * a->T targets.
static int split_eval_run(const mpv_split_eval_args* a, int64_t D, double* out_defs,
                          void* workspace, size_t workspace_bytes, void* stream) {
  MPV_REQUIRE(a != nullptr, "mpv_split_eval_args is NULL");
  MPV_REQUIRE(D >= 1 && D <= (int64_t(1) << 20), "definitions D must be in 1 .. 2^20 (got %lld)",
              (long long)D);
  MPV_REQUIRE(split_shape_ok(a->N, a->L, a->T, D, a->G),
              "bad split shape N=%lld L=%lld T=%lld G=%lld", (long long)a->N, (long long)a->L,
              (long long)(a->T * D), (long long)a->G);
  MPV_REQUIRE(split_slices_ok(a->R), "split row slices R must be in 1 .. 65535 (got %lld)",
              (long long)a->R);
  MPV_REQUIRE(a->pred && a->target, "NULL pred / target in mpv_split_eval_args");
  MPV_REQUIRE(a->goff != nullptr || a->G == 1, "NULL goff with G = %lld groups", (long long)a->G);
  MPV_REQUIRE(a->T == 0 || (a->w != nullptr && a->terms != nullptr), "NULL w / terms with T > 0");
  MPV_REQUIRE(a->counts && a->out, "NULL counts / out in mpv_split_eval_args");
  mpv_split_eval_args all = *a;
  all.T = a->T * D;
  Workspace carve(workspace);
  const EvalWs ws = eval_ws(carve, all.L, all.T, all.G, all.R);
  MPV_REQUIRE(carve.fits(workspace_bytes), "split workspace too small");
  hipStream_t st = as_stream(stream);
  const int lp = eval_lanes(all.L);
  MPV_LAUNCH("split_eval", split_eval_kernel,
             dim3((unsigned)cdiv(all.L, lp), (unsigned)all.G, (unsigned)all.R), dim3(kEvalThreads),
             0, st, all, ws, lp);
  MPV_LAUNCH("split_final", split_final_kernel, dim3(1), dim3(kEvalThreads), 0, st, all, ws,
             (int)D, out_defs);
  return MPV_OK;
}

extern "C" {

size_t mpv_split_eval_workspace_bytes(int64_t N, int64_t L, int64_t T, int64_t G, int64_t R) {
  if (!split_shape_ok(N, L, T, 1, G) || !split_slices_ok(R)) return 0;
  return layout_bytes(eval_ws, L, T, G, R);
}

int mpv_split_eval(const mpv_split_eval_args* a, void* workspace, size_t workspace_bytes,
                   void* stream) {
  return split_eval_run(a, 1, nullptr, workspace, workspace_bytes, stream);
}

int mpv_split_eval_defs(const mpv_split_eval_args* a, int64_t D, double* out_defs,
                        void* workspace, size_t workspace_bytes, void* stream) {
  MPV_REQUIRE(out_defs != nullptr, "NULL out_defs in mpv_split_eval_defs");
  return split_eval_run(a, D, out_defs, workspace, workspace_bytes, stream);
}

}  // extern "C"
