// The two per-step consumers of compute_loss's indiv_prob outputs in the
// reference training loop, on the device:
//
//   row_weights_kernel     per-row weights of up to 8 sources a launch, the row's
//                          0/1 label pattern packed by wave ballots once.  A
//                          template over the source set.  LabelTables: weight =
//                          label_distances[target].get(''.join(label.astype(
//                          str)), 0.) (fairsoft_train.py:85-93), the pattern
//                          looked up in an open-addressing table of packed
//                          patterns (built once on the host from the same dict)
//                          instead of a Python string join and dict lookup per
//                          row.  LabelSims: the weights without a dict:
//                          indication, constant, Jaccard and Hamming similarity
//                          to a packed target (label_distance_obs.py:9-168, with
//                          dist_gamma the clipped exponential) from popcounts
//                          of the packed row.
//   group_rows_kernel      the batch's sensitive groups (torch.unique(x, dim=0)'s
//                          inverse, fairsoft_train.py:81, :106-111) with the
//                          stable order by group and the group offsets, in one
//                          launch of one workgroup.
//   fair_fwd_kernel        the fairness regulariser (fairsoft_train.py:95-131):
//                          weighted means of indiv_prob_label / indiv_prob over
//                          the batch and over each sensitive group, l1 or l2
//                          distance, summed over target labels and groups.  fp64
//                          throughout.  The reference computes in fp64 when its
//                          distances are numpy float64 (torch.tensor(weights)
//                          is float64 and the products promote) and in fp32
//                          when they are Python floats; the host returns the
//                          loss in that dtype (mpvae_fair.py).  Also stashes
//                          f'(d) / W_tk and sum_k f'(d) / W_t for the backward.
//   fair_bwd_kernel        d penalty / d indiv_prob[_label] (autograd through
//                          the same lines; |x|' = sgn(x), sgn(0) = 0).
//   metric_rows_kernel,    evals.compute_metrics(..., all_metrics=False)
//   metric_cols_kernel,    (evals.py:178-238): ACC, HA, ebF1, miF1, maF1 and
//   metric_final_kernel    p@1/3/5 without copying the batch to the host.
//
// All reductions run in a fixed order: results are deterministic.
#include "abi_util.h"
#include "mpv_common.h"

namespace mpv {

// ------------------------------------------------------------ label weights
// splitmix64 finaliser; the host builder (mpvae_fair.py) uses the same mix
MPV_DEV uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// One wave per batch row.  Bit j of word w is label 64w + j (character
// 64w + j of the reference's key string).  A row with a label value whose
// int() is neither 0 nor 1 has no binary key: weight 0, as a dict miss.
constexpr int kLwWaves = 4;

// Row b's pattern into words[0..W) (this wave's LDS row) and its hash; true
// when the row has no binary key.
MPV_DEV bool pack_row(const float* __restrict__ y, int b, int L, int W, uint64_t* words,
                      uint64_t& h) {
  const int lane = threadIdx.x & 63;
  bool bad = false;
  h = 0x6A09E667F3BCC909ull ^ (uint64_t)W;
  for (int k = 0; k < W; ++k) {
    const int l = k * 64 + lane;
    const float v = l < L ? truncf(y[(int64_t)b * L + l]) : 0.0f;
    bad |= !(v == 0.0f || v == 1.0f);
    const uint64_t bits = __ballot(v == 1.0f);
    if (lane == 0) words[k] = bits;
    h = mix64(h ^ bits);
  }
  bad = __any(bad);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  return bad;
}

// The table's value for the packed row (0 when absent), the whole wave probing.
MPV_DEV double probe_table(const mpv_label_table& tab, uint64_t h, const uint64_t* words) {
  const int lane = threadIdx.x & 63, W = (int)tab.W;
  if (tab.nslots <= 0) return 0.0;
  const uint64_t mask = (uint64_t)tab.nslots - 1;
  for (uint64_t probe = 0; probe < (uint64_t)tab.nslots; ++probe) {
    const uint64_t slot = (h + probe) & mask;
    if (!tab.used[slot]) break;  // empty slot: not in the table
    bool diff = false;
    for (int k = lane; k < W; k += 64) diff |= tab.keys[slot * W + k] != words[k];
    if (!__any(diff)) return tab.vals[slot];
  }
  return 0.0;
}

// A set of up to N weight sources passed by value, rows t = 0 .. n - 1 of a
// launch's w.  The two kinds differ in weight() alone: the value of source i
// for the packed row (`words` in LDS with hash h; `row` is lane's word, 0 past
// W), the whole wave calling.
//
// Target tables (mpv_label_weights: N = 1; mpv_label_weights_batch): the row
// is packed and hashed once, then probed in every table.
template <int N>
struct LabelTables {
  mpv_label_table s[N];
  int n;
  MPV_DEV double weight(int i, uint64_t h, const uint64_t* words, uint64_t, int) const {
    return probe_table(s[i], h, words);
  }
};

// Similarity definitions: the weight is a closed form of the row's and the
// target's bit patterns (what the builders of label_distance_obs.py store per
// pair of label strings), three popcounts per word.
struct LabelSims {
  mpv_label_sim s[MPV_LABEL_SIMS_PER_LAUNCH];
  int n;
  MPV_DEV double weight(int i, uint64_t, const uint64_t*, uint64_t row, int L) const {
    const int lane = threadIdx.x & 63, W = (L + 63) / 64;
    const mpv_label_sim& d = s[i];
    const uint64_t tgt = lane < W ? d.target[lane] : 0;
    int n_and = __popcll(row & tgt), n_or = __popcll(row | tgt), n_xor = __popcll(row ^ tgt);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {  // integer sums: order-free
      n_and += __shfl_xor(n_and, o, 64);
      n_or += __shfl_xor(n_or, o, 64);
      n_xor += __shfl_xor(n_xor, o, 64);
    }
    double sim = 1.0;  // MPV_SIM_CONSTANT
    if (d.kind == MPV_SIM_INDICATION) {
      sim = n_xor == 0 ? 1.0 : 0.0;
    } else if (d.kind == MPV_SIM_JACCARD) {  // unequal patterns have n_or > 0
      sim = n_xor == 0 ? 1.0 : (double)n_and / (double)n_or;
    } else if (d.kind == MPV_SIM_HAMMING) {
      sim = (double)(L - n_xor) / (double)L;
    }
    // np.clip(np.exp(gamma * (sim - 1)), lo, hi): subtract, then multiply, so
    // nothing is contracted and exp sees numpy's argument
    if (d.has_gamma) return fmin(fmax(exp(d.gamma * (sim - 1.0)), d.clip_lo), d.clip_hi);
    return sim;
  }
};

template <typename Set>
__global__ __launch_bounds__(64 * kLwWaves) void row_weights_kernel(
    const float* __restrict__ y, int B, int L, Set set, double* __restrict__ w,
    int* __restrict__ contributed) {
  __shared__ uint64_t words[kLwWaves][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = (L + 63) / 64;
  const int b = blockIdx.x * kLwWaves + wv;
  if (b >= B) return;
  uint64_t h;
  const bool bad = pack_row(y, b, L, W, words[wv], h);
  const uint64_t row = lane < W ? words[wv][lane] : 0;
  int positive = 0;
  for (int t = 0; t < set.n; ++t) {
    const double val = bad ? 0.0 : set.weight(t, h, words[wv], row, L);
    if (lane == 0) w[(int64_t)t * B + b] = val;
    positive += val > 0.0;
  }
  if (lane == 0 && positive) atomicAdd(contributed, positive);  // integer count: order-free
}

// ------------------------------------------------------------- row grouping
// torch.unique(x, dim=0)'s inverse with the group layout mpv_fair_args wants,
// in one workgroup: every row's rank among the distinct rows, then its place
// in the stable order by group.  O(B^2 n) compares on integers in loops of a
// fixed order; the rows sit in LDS when they fit.
constexpr int kGroupThreads = 1024;
constexpr int kGroupStageBytes = 40960;  // + 20 KiB of static LDS below: under 64 KiB

// < 0, 0, > 0: row a sorts before, equals, sorts after row b; by value, so
// -0.0 equals +0.0
template <typename T>
MPV_DEV int row_cmp(const T* a, const T* b, int n) {
  for (int j = 0; j < n; ++j) {
    const T u = a[j], v = b[j];
    if (u != v) return u < v ? -1 : 1;
  }
  return 0;
}

template <typename T>
__global__ __launch_bounds__(kGroupThreads) void group_rows_kernel(
    const T* __restrict__ x, int B, int n, int G, int stage, int* __restrict__ gid,
    int* __restrict__ order, int* __restrict__ goff, uint8_t* __restrict__ overflow) {
  extern __shared__ __attribute__((aligned(16))) unsigned char group_stage[];
  __shared__ int s_gid[MPV_GROUP_MAX_B];
  __shared__ uint8_t s_first[MPV_GROUP_MAX_B];
  __shared__ int s_over;
  const int tid = threadIdx.x, nt = blockDim.x;
  const T* rows = x;
  if (stage) {
    T* s = reinterpret_cast<T*>(group_stage);
    for (int i = tid; i < B * n; i += nt) s[i] = x[i];
    rows = s;
  }
  if (tid == 0) s_over = 0;
  __syncthreads();
  // row b is the first occurrence of its pattern: no earlier identical row
  for (int b = tid; b < B; b += nt) {
    int c = 0;
    while (c < b && row_cmp(rows + c * n, rows + b * n, n) != 0) ++c;
    s_first[b] = c == b;
  }
  __syncthreads();
  // r(b) = distinct rows that sort before row b
  for (int b = tid; b < B; b += nt) {
    int r = 0;
    for (int c = 0; c < B; ++c)
      if (s_first[c] && row_cmp(rows + c * n, rows + b * n, n) < 0) ++r;
    if (r >= G) {
      s_over = 1;  // every writer stores the same value
      r = G - 1;
    }
    s_gid[b] = r;
    gid[b] = r;
  }
  __syncthreads();
  // the stable argsort by group: rows of a smaller group, then earlier rows of this one
  for (int b = tid; b < B; b += nt) {
    const int k = s_gid[b];
    int pos = 0;
    for (int c = 0; c < B; ++c) {
      const int kc = s_gid[c];
      pos += (kc < k || (kc == k && c < b)) ? 1 : 0;
    }
    order[pos] = b;
  }
  for (int k = tid; k <= G; k += nt) {
    int below = 0;
    for (int c = 0; c < B; ++c) below += s_gid[c] < k ? 1 : 0;
    goff[k] = below;
  }
  if (tid == 0) *overflow = s_over ? 1 : 0;
}

// -------------------------------------------------------- fairness penalty
constexpr int kFairThreads = 256;

// Weight sums W_t (index t*(G+1) + G) and W_tk (t*(G+1) + k), one thread per
// (t, k) pair, each a fixed-order loop: deterministic.
__global__ void fair_wsum_kernel(const double* __restrict__ w, const int* __restrict__ order,
                                 const int* __restrict__ goff, int B, int T, int G,
                                 double* __restrict__ wsum) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * (G + 1)) return;
  const int t = i / (G + 1), k = i % (G + 1);
  double s = 0.0;
  if (k == G) {
    for (int b = 0; b < B; ++b) s += w[(int64_t)t * B + b];
  } else {
    for (int j = goff[k]; j < goff[k + 1]; ++j) s += w[(int64_t)t * B + order[j]];
  }
  wsum[i] = s;
}

// One thread per (label l, branch br): br 0 = indiv_prob_label (label_z),
// br 1 = indiv_prob (feat_z).
__global__ __launch_bounds__(kFairThreads) void fair_fwd_kernel(mpv_fair_args a,
                                                                const double* __restrict__ wsum,
                                                                double* __restrict__ dtab,
                                                                double* __restrict__ etab,
                                                                double* __restrict__ part) {
  __shared__ double red[kFairThreads / 64];
  const int L = (int)a.L, B = (int)a.B, T = (int)a.T, G = (int)a.G;
  const int br = blockIdx.y;
  const int l = blockIdx.x * kFairThreads + threadIdx.x;
  const float* z = br == 0 ? a.label_z : a.feat_z;
  double pen = 0.0;
  if (l < L) {
    for (int t = 0; t < T; ++t) {
      const double* wt = a.w + (int64_t)t * B;
      const double Wt = wsum[t * (G + 1) + G];
      double esum = 0.0;
      if (Wt > 0.0) {  // fairsoft_train.py:97 `if weights.sum() > 0`
        double tot = 0.0;
        for (int b = 0; b < B; ++b) tot += (double)z[(int64_t)b * L + l] * wt[b];
        const double mt = tot / Wt;
        for (int k = 0; k < G; ++k) {
          const double Wk = wsum[t * (G + 1) + k];
          double fp = 0.0;
          if (Wk > 0.0) {  // :110 `if weight_sensitive.sum() > 0`
            double s = 0.0;
            for (int j = a.goff[k]; j < a.goff[k + 1]; ++j) {
              const int b = a.order[j];
              s += (double)z[(int64_t)b * L + l] * wt[b];
            }
            fp = fair_pair_step(s, Wk, mt, a.norm, pen, esum);
          }
          dtab[(((int64_t)br * T + t) * G + k) * L + l] = fp;
        }
        esum /= Wt;
      } else {
        for (int k = 0; k < G; ++k) dtab[(((int64_t)br * T + t) * G + k) * L + l] = 0.0;
      }
      etab[((int64_t)br * T + t) * L + l] = esum;
    }
  }
  pen = block_sum_f64<kFairThreads / 64>(pen, red);
  if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = pen;
}

__global__ void fair_final_kernel(const double* __restrict__ part, int n, double coeff,
                                  double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += part[i];
  *out = coeff * s;
}

// grad[b, l] = gout * coeff * sum_t w[t,b] (dtab[t, gid[b], l] - etab[t, l])
__global__ __launch_bounds__(kFairThreads) void fair_bwd_kernel(mpv_fair_args a,
                                                                const double* __restrict__ dtab,
                                                                const double* __restrict__ etab,
                                                                const double* __restrict__ gout,
                                                                float* __restrict__ g_label_z,
                                                                float* __restrict__ g_feat_z) {
  const int L = (int)a.L, B = (int)a.B, T = (int)a.T, G = (int)a.G;
  const int64_t i = (int64_t)blockIdx.x * kFairThreads + threadIdx.x;
  const int br = blockIdx.y;
  if (i >= (int64_t)B * L) return;
  const int b = (int)(i / L), l = (int)(i % L), k = a.gid[b];
  double g = 0.0;
  for (int t = 0; t < T; ++t) {
    const double wb = a.w[(int64_t)t * B + b];
    g += wb * (dtab[(((int64_t)br * T + t) * G + k) * L + l] - etab[((int64_t)br * T + t) * L + l]);
  }
  g *= *gout * a.fair_coeff;
  (br == 0 ? g_label_z : g_feat_z)[i] = (float)g;
}

// ------------------------------------------------------------ train metrics
constexpr int kMetThreads = 256;

struct ArgMax {
  float v;
  int i;
};
// larger value wins; on a tie the larger index (= numpy argsort(...)[::-1]
// with a stable sort; numpy's default sort is not stable)
MPV_DEV ArgMax better(ArgMax a, ArgMax b) {
  return (b.v > a.v || (b.v == a.v && b.i > a.i)) ? b : a;
}

// One block per batch row: subset accuracy, hamming, example-F1 terms and the
// top-5 hits (evals.py:13-45, 48-83).  rowstat[b] = [eq_all, xor_count,
// tp, sum_true, sum_pred, hit@1, hit@3, hit@5].
__global__ __launch_bounds__(kMetThreads) void metric_rows_kernel(const float* __restrict__ pred,
                                                                  const float* __restrict__ tgt,
                                                                  int B, int L, float thr,
                                                                  double* __restrict__ rowstat) {
  __shared__ float sred[5][kMetThreads / 64];
  __shared__ ArgMax am[kMetThreads / 64];
  __shared__ int chosen[5];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* pr = pred + (int64_t)b * L;
  const float* tr = tgt + (int64_t)b * L;
  float neq = 0.f, nxor = 0.f, tp = 0.f, st = 0.f, sp = 0.f;
  for (int l = tid; l < L; l += kMetThreads) {
    const float p = pr[l] < thr ? 0.0f : 1.0f;  // evals.py:201-202
    const float t = tr[l];
    neq += (t == p) ? 0.f : 1.f;
    nxor += ((t != 0.f) != (p != 0.f)) ? 1.f : 0.f;
    tp += t * p;
    st += t;
    sp += p;
  }
  float v[5] = {neq, nxor, tp, st, sp};
#pragma unroll
  for (int k = 0; k < 5; ++k) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if (lane == 0) sred[k][wv] = v[k];
  }
  // top-5 by the raw probabilities, one block argmax per rank
  int hits[5];
  for (int r = 0; r < 5; ++r) {
    ArgMax m{-INFINITY, -1};
    for (int l = tid; l < L; l += kMetThreads) {
      bool used = false;
      for (int q = 0; q < r; ++q) used |= chosen[q] == l;
      if (!used) m = better(m, ArgMax{pr[l], l});
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      ArgMax x{__shfl_xor(m.v, o, 64), __shfl_xor(m.i, o, 64)};
      m = better(m, x);
    }
    if (lane == 0) am[wv] = m;
    __syncthreads();
    if (tid == 0) {
      ArgMax best = am[0];
      for (int i = 1; i < kMetThreads / 64; ++i) best = better(best, am[i]);
      chosen[r] = best.i;
    }
    __syncthreads();
    hits[r] = (chosen[r] >= 0 && tr[chosen[r]] == 1.0f) ? 1 : 0;
  }
  if (tid == 0) {
    float s[5];
    for (int k = 0; k < 5; ++k) {
      s[k] = 0.f;
      for (int i = 0; i < kMetThreads / 64; ++i) s[k] += sred[k][i];
    }
    double* o = rowstat + (int64_t)b * 8;
    o[0] = s[0] == 0.f ? 1.0 : 0.0;  // all labels equal
    o[1] = s[1];
    o[2] = s[2];
    o[3] = s[3];
    o[4] = s[4];
    o[5] = hits[0];
    o[6] = hits[0] + hits[1] + hits[2];
    o[7] = hits[0] + hits[1] + hits[2] + hits[3] + hits[4];
  }
}

// One thread per label: tp, fp, fn over the batch (compute_tp_fp_fn axis=0).
__global__ void metric_cols_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                   int B, int L, float thr, float* __restrict__ colstat) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  float tp = 0.f, fp = 0.f, fn = 0.f;
  for (int b = 0; b < B; ++b) {
    const float p = pred[(int64_t)b * L + l] < thr ? 0.0f : 1.0f;
    const float t = tgt[(int64_t)b * L + l];
    tp += t * p;
    fp += (t == 0.f ? 1.f : 0.f) * p;
    fn += t * (p == 0.f ? 1.f : 0.f);
  }
  colstat[l] = tp;
  colstat[L + l] = fp;
  colstat[2 * L + l] = fn;
}

// out = [ACC, HA, ebF1, miF1, maF1, p@1, p@3, p@5] (evals.py:205-237)
__global__ void metric_final_kernel(const double* __restrict__ rowstat,
                                    const float* __restrict__ colstat, int B, int L,
                                    double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double acc = 0, hl = 0, ef = 0, p1 = 0, p3 = 0, p5 = 0;
  int nef = 0;
  for (int b = 0; b < B; ++b) {
    const double* r = rowstat + (int64_t)b * 8;
    acc += r[0];
    hl += r[1] / L;
    const float den = (float)r[3] + (float)r[4];
    if (den != 0.0f) {
      ef += (double)((2.0f * (float)r[2]) / den);
      ++nef;
    }
    p1 += r[5] / 1.0;
    p3 += r[6] / 3.0;
    p5 += r[7] / 5.0;
  }
  double tp = 0, fp = 0, fn = 0, ma = 0;
  int nma = 0;
  for (int l = 0; l < L; ++l) {
    const float a = colstat[l], c = colstat[L + l], d = colstat[2 * L + l];
    tp += a;
    fp += c;
    fn += d;
    const double f = (double)(2.0f * a) / (double)(2.0f * a + c + d + 1e-6f);
    if (isfinite(f)) {
      ma += f;
      ++nma;
    }
  }
  out[0] = acc / B;
  out[1] = 1.0 - hl / B;
  out[2] = nef ? ef / nef : NAN;
  out[3] = (2.0 * tp) / (2.0 * tp + fp + fn);
  out[4] = nma ? ma / nma : NAN;
  out[5] = p1 / B;
  out[6] = p3 / B;
  out[7] = p5 / B;
}

}  // namespace mpv

using namespace mpv;

static int check_label_table(const mpv_label_table* tab, int64_t L) {
  MPV_REQUIRE(tab->W == (L + 63) / 64, "table words %lld != ceil(L/64) = %lld",
              (long long)tab->W, (long long)((L + 63) / 64));
  MPV_REQUIRE(tab->nslots == 0 || (tab->keys && tab->vals && tab->used &&
                                   (tab->nslots & (tab->nslots - 1)) == 0),
              "table slots must be a power of two with keys/vals/used");
  MPV_REQUIRE(tab->W <= 64, "label_dim > 4096 is not supported by the pattern table");
  return MPV_OK;
}

// T sources in launches of a Set's capacity each, chunk t0 filling rows t0 ..
// of w (the unused slots of the last chunk repeat its first source).  `tag` is
// the timing label.
template <typename Set, typename Src>
static int launch_row_weights(const char* tag, const float* y, int64_t B, int64_t L,
                              const Src* src, int64_t T, double* w, int32_t* contributed,
                              void* stream) {
  constexpr int64_t cap = sizeof(Set::s) / sizeof(Src);
  const int blocks = (int)cdiv(B, kLwWaves);
  for (int64_t t0 = 0; t0 < T; t0 += cap) {
    Set set;
    set.n = (int)(T - t0 < cap ? T - t0 : cap);
    for (int64_t i = 0; i < cap; ++i) set.s[i] = src[t0 + (i < set.n ? i : 0)];
    MPV_LAUNCH(tag, row_weights_kernel<Set>, dim3(blocks), dim3(64 * kLwWaves), 0,
               as_stream(stream), y, (int)B, (int)L, set, w + t0 * B, contributed);
  }
  return MPV_OK;
}

template <typename T>
static int launch_group_rows(const void* x, int B, int n, int G, int32_t* gid, int32_t* order,
                              int32_t* goff, uint8_t* overflow, hipStream_t st) {
  const size_t bytes = sizeof(T) * (size_t)B * n;
  const int stage = bytes <= (size_t)kGroupStageBytes;
  const int threads = B >= kGroupThreads ? kGroupThreads : (int)cdiv(B, 64) * 64;
  MPV_LAUNCH("group_rows", group_rows_kernel<T>, dim3(1), dim3(threads), stage ? bytes : 0, st,
             static_cast<const T*>(x), B, n, G, stage, gid, order, goff, overflow);
  return MPV_OK;
}

static bool fair_shape_ok(int64_t L, int64_t T, int64_t G) { return L > 0 && T > 0 && G > 0; }

struct FairWs {
  double* dtab;  // (2, T, G, L)
  double* etab;  // (2, T, L)
  double* wsum;  // (T, G + 1)
  double* part;  // (2 NLB)  penalty partials
};

static FairWs fair_ws(Workspace& ws, int64_t L, int64_t T, int64_t G) {
  FairWs f;
  f.dtab = ws.take<double>(2, T, G, L);
  f.etab = ws.take<double>(2, T, L);
  f.wsum = ws.take<double>(T, G + 1);
  f.part = ws.take<double>(2, cdiv(L, kFairThreads));
  return f;
}

static bool metrics_shape_ok(int64_t B, int64_t L) { return B > 0 && L > 0; }

struct MetricsWs {
  double* rowstat;  // (B, 8)
  float* colstat;   // (3, L)
};

static MetricsWs metrics_ws(Workspace& ws, int64_t B, int64_t L) {
  MetricsWs m;
  m.rowstat = ws.take<double>(B, 8);
  m.colstat = ws.take<float>(3, L);
  return m;
}

extern "C" {

int mpv_label_weights(const float* y, int64_t B, int64_t L, const mpv_label_table* tab,
                      double* w, int32_t* contributed, void* stream) {
  MPV_REQUIRE(y && tab && w && contributed && B > 0 && L > 0, "bad label_weights arguments");
  if (int rc = check_label_table(tab, L)) return rc;
  return launch_row_weights<LabelTables<1>>("label_weights", y, B, L, tab, 1, w, contributed,
                                            stream);
}

int mpv_label_weights_batch(const float* y, int64_t B, int64_t L, const mpv_label_table* tables,
                            int64_t T, double* w, int32_t* contributed, void* stream) {
  MPV_REQUIRE(y && tables && w && contributed && B > 0 && L > 0 && T > 0,
              "bad label_weights_batch arguments");
  for (int64_t t = 0; t < T; ++t)  // every table is checked before the first launch
    if (int rc = check_label_table(tables + t, L)) return rc;
  return launch_row_weights<LabelTables<MPV_LABEL_TABLES_PER_LAUNCH>>(
      "label_weights", y, B, L, tables, T, w, contributed, stream);
}

int mpv_label_sim_weights(const float* y, int64_t B, int64_t L, const mpv_label_sim* sims,
                          int64_t T, double* w, int32_t* contributed, void* stream) {
  MPV_REQUIRE(L >= 1 && L <= 4096, "label_sim_weights supports 1 <= label_dim <= 4096 (got %lld)",
              (long long)L);
  MPV_REQUIRE(y && sims && w && contributed && B > 0 && T > 0, "bad label_sim_weights arguments");
  for (int64_t t = 0; t < T; ++t) {  // every definition is checked before the first launch
    MPV_REQUIRE(sims[t].target != nullptr, "similarity %lld has no target", (long long)t);
    MPV_REQUIRE(sims[t].kind >= MPV_SIM_INDICATION && sims[t].kind <= MPV_SIM_HAMMING,
                "similarity %lld: unknown kind %d", (long long)t, (int)sims[t].kind);
  }
  return launch_row_weights<LabelSims>("label_sim", y, B, L, sims, T, w, contributed, stream);
}

int mpv_group_rows(const void* x, int x_elem, int64_t B, int64_t n, int64_t G, int32_t* gid,
                   int32_t* order, int32_t* goff, uint8_t* overflow, void* stream) {
  MPV_REQUIRE(x && gid && order && goff && overflow, "NULL pointer in mpv_group_rows");
  MPV_REQUIRE(B >= 1 && B <= MPV_GROUP_MAX_B && n >= 1 && n <= MPV_GROUP_MAX_N && G >= 1 &&
                  G <= MPV_GROUP_MAX_B,
              "mpv_group_rows supports 1 <= B, G <= %d and 1 <= n <= %d (got B %lld, n %lld, "
              "G %lld)", MPV_GROUP_MAX_B, MPV_GROUP_MAX_N, (long long)B, (long long)n,
              (long long)G);
  hipStream_t st = as_stream(stream);
  switch (x_elem) {
    case MPV_EL_F32:
      return launch_group_rows<float>(x, (int)B, (int)n, (int)G, gid, order, goff, overflow, st);
    case MPV_EL_F64:
      return launch_group_rows<double>(x, (int)B, (int)n, (int)G, gid, order, goff, overflow, st);
    case MPV_EL_I32:
      return launch_group_rows<int32_t>(x, (int)B, (int)n, (int)G, gid, order, goff, overflow, st);
    case MPV_EL_I64:
      return launch_group_rows<int64_t>(x, (int)B, (int)n, (int)G, gid, order, goff, overflow, st);
    default:
      return fail(MPV_EINVAL, "mpv_group_rows: unknown element type %d", x_elem);
  }
}

size_t mpv_fair_workspace_bytes(int64_t L, int64_t T, int64_t G) {
  if (!fair_shape_ok(L, T, G)) return 0;
  return layout_bytes(fair_ws, L, T, G);
}

int mpv_fair_fwd(const mpv_fair_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  MPV_REQUIRE(a && a->label_z && a->feat_z && a->w && a->order && a->goff && a->gid && a->out,
              "NULL pointer in mpv_fair_args");
  MPV_REQUIRE(a->B > 0 && fair_shape_ok(a->L, a->T, a->G), "bad fairness shape");
  Workspace carve(workspace);
  const FairWs ws = fair_ws(carve, a->L, a->T, a->G);
  MPV_REQUIRE(carve.fits(workspace_bytes), "fairness workspace too small");
  hipStream_t st = as_stream(stream);
  const int npair = (int)(a->T * (a->G + 1));
  MPV_LAUNCH("fair_fwd", fair_wsum_kernel, dim3((unsigned)cdiv(npair, 64)), dim3(64), 0, st, a->w,
             a->order, a->goff, (int)a->B, (int)a->T, (int)a->G, ws.wsum);
  const int nlb = (int)cdiv(a->L, kFairThreads);
  MPV_LAUNCH("fair_fwd", fair_fwd_kernel, dim3(nlb, 2), dim3(kFairThreads), 0, st, *a, ws.wsum,
             ws.dtab, ws.etab, ws.part);
  MPV_LAUNCH("fair_fwd", fair_final_kernel, dim3(1), dim3(64), 0, st, ws.part, 2 * nlb,
             a->fair_coeff, a->out);
  return MPV_OK;
}

int mpv_fair_bwd(const mpv_fair_args* a, const double* gout, float* g_label_z, float* g_feat_z,
                 void* workspace, size_t workspace_bytes, void* stream) {
  MPV_REQUIRE(a && gout && g_label_z && g_feat_z && a->w && a->gid, "NULL pointer in fair_bwd");
  Workspace carve(workspace);
  const FairWs ws = fair_ws(carve, a->L, a->T, a->G);
  MPV_REQUIRE(carve.fits(workspace_bytes), "fairness workspace too small");
  const int64_t n = a->B * a->L;
  MPV_LAUNCH("fair_bwd", fair_bwd_kernel, dim3((unsigned)cdiv(n, kFairThreads), 2),
             dim3(kFairThreads), 0, as_stream(stream), *a, ws.dtab, ws.etab, gout, g_label_z,
             g_feat_z);
  return MPV_OK;
}

size_t mpv_metrics_workspace_bytes(int64_t B, int64_t L) {
  if (!metrics_shape_ok(B, L)) return 0;
  return layout_bytes(metrics_ws, B, L);
}

int mpv_train_metrics(const float* pred, const float* target, int64_t B, int64_t L,
                      float threshold, double* out, void* workspace, size_t workspace_bytes,
                      void* stream) {
  MPV_REQUIRE(pred && target && out && metrics_shape_ok(B, L), "bad train_metrics arguments");
  Workspace carve(workspace);
  const MetricsWs ws = metrics_ws(carve, B, L);
  MPV_REQUIRE(carve.fits(workspace_bytes), "metrics workspace too small");
  hipStream_t st = as_stream(stream);
  MPV_LAUNCH("metrics", metric_rows_kernel, dim3((unsigned)B), dim3(kMetThreads), 0, st, pred,
             target, (int)B, (int)L, threshold, ws.rowstat);
  MPV_LAUNCH("metrics", metric_cols_kernel, dim3((unsigned)cdiv(L, 256)), dim3(256), 0, st, pred,
             target, (int)B, (int)L, threshold, ws.colstat);
  MPV_LAUNCH("metrics", metric_final_kernel, dim3(1), dim3(64), 0, st, ws.rowstat, ws.colstat,
             (int)B, (int)L, out);
  return MPV_OK;
}

}  // extern "C"
