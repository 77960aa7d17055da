// The validation metrics of evals.compute_metrics(..., all_metrics=True)
// (evals.py:129-175) on the device: per-label ROC AUC, area under the
// precision-recall curve and recall at FDR <= 0.5, and their mean / median /
// variance over the labels, without copying the validation split to the host.
//
//   curve_keys_kernel    (N, L) row-major pred / target -> label-major (L, N)
//                        64-bit sort keys: the score's bits mapped to an
//                        unsigned integer monotone in the score (-0.0 folded
//                        onto +0.0), shifted left by one, the label bit below.
//                        Only per-run totals of equal scores are used later,
//                        so no row index rides along and the order inside a
//                        run never shows in a result.
//   curve_sort_kernel    one workgroup sorts one segment of up to `chunk` keys
//                        of one label in LDS (bitonic, descending).
//   curve_merge_kernel   N > chunk: pairwise merge passes over the sorted
//                        segments, global -> global between two ping-pong
//                        buffers, one launch per pass.  Each workgroup owns one
//                        output tile; its inputs come from a merge-path split,
//                        so no workgroup waits for another.
//   curve_pass_kernel    one workgroup per label walks the sorted keys in
//                        tiles: inclusive scan of the label bit (T), a max-scan
//                        that carries the previous run end, and the AUC / AUPR
//                        terms and the FDR candidate at every run end.
//   curve_agg_kernel     mean, median (np.median: the two middle values
//                        averaged) and population variance over the labels
//                        whose value is not NaN.
//
// fp64 throughout.  Every floating-point sum runs in an order fixed by N (or L)
// alone -- thread t adds its own run ends in index order, then a fixed shuffle
// tree, then the waves in order -- never by which sort path ran or by `chunk`:
// the sorted key array is the same bits either way.  No floating-point atomics.
#include "abi_util.h"
#include "mpv_common.h"

namespace mpv {

// Default (and largest) LDS sort segment: 4096 keys x 8 B = 32 KiB per
// workgroup of 512 threads.  Four such workgroups fill a CU's 32 wave slots
// and take 128 of its 160 KiB of LDS, so the wave cap and not LDS bounds
// occupancy; 8192 keys (64 KiB) would leave two workgroups (16 waves) per CU.
constexpr int kCurveChunk = 4096;
constexpr int kSortThreads = 512;
constexpr int kCurveMaxL = 4096;  // curve_agg_kernel sorts the L values in LDS

MPV_DEV uint64_t curve_key(float score, float target) {
  uint32_t u = __float_as_uint(score);
  if (u == 0x80000000u) u = 0;  // -0.0 == +0.0: one threshold run
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 1) | (target == 1.0f ? 1u : 0u);
}

// ---------------------------------------------------------------- key build
constexpr int kKeyTile = 64;
__global__ __launch_bounds__(256) void curve_keys_kernel(const float* __restrict__ pred,
                                                         const float* __restrict__ tgt, int64_t N,
                                                         int L, uint64_t* __restrict__ keys) {
  __shared__ uint64_t tile[kKeyTile][kKeyTile + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t n0 = (int64_t)blockIdx.x * kKeyTile;
  const int l0 = blockIdx.y * kKeyTile;
  for (int r = ty; r < kKeyTile; r += 4) {  // lanes along l: coalesced reads
    const int64_t n = n0 + r;
    const int l = l0 + tx;
    if (n < N && l < L) tile[tx][r] = curve_key(pred[n * L + l], tgt[n * L + l]);
  }
  __syncthreads();
  for (int li = ty; li < kKeyTile; li += 4) {  // lanes along n: coalesced writes
    const int64_t n = n0 + tx;
    const int l = l0 + li;
    if (n < N && l < L) keys[(int64_t)l * N + n] = tile[li][tx];
  }
}

// --------------------------------------------------------------------- sort
// Segment blockIdx.x (chunk keys, the last one ragged) of label blockIdx.y,
// padded in LDS to a power of two with key 0: the pad sorts to the end of a
// descending order and is not written back.
__global__ __launch_bounds__(kSortThreads) void curve_sort_kernel(uint64_t* __restrict__ keys,
                                                                  int64_t N, int chunk) {
  __shared__ uint64_t s[kCurveChunk];
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * chunk;
  const int64_t base = (int64_t)blockIdx.y * N + c0;
  const int n = (int)(N - c0 < chunk ? N - c0 : chunk);
  int m = 64;
  while (m < n) m <<= 1;  // m <= chunk <= kCurveChunk
  for (int i = tid; i < m; i += kSortThreads) s[i] = i < n ? keys[base + i] : 0;
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (m >> 1); t += kSortThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // bit j clear
        const int p = i | j;
        const bool desc = (i & k) == 0;
        const uint64_t a = s[i], b = s[p];
        if ((a < b) == desc) {
          s[i] = b;
          s[p] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n; i += kSortThreads) keys[base + i] = s[i];
}

// Merge path of two descending runs: how many of the first d outputs come
// from A, ties going to A.
template <typename P>
MPV_DEV int64_t merge_path(P A, int64_t na, P B, int64_t nb, int64_t d) {
  int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (A[mid] >= B[d - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One pass: runs of w keys (the last ragged, a run without a partner copied)
// merge pairwise from src into dst.  blockIdx.x = pair * tiles_per_pair + tile;
// a workgroup owns outputs [d0, d1) of its pair.
constexpr int kMergeThreads = 256, kMergeItems = 4, kMergeTile = kMergeThreads * kMergeItems;
__global__ __launch_bounds__(kMergeThreads) void curve_merge_kernel(
    const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, int64_t N, int64_t w,
    int tiles_per_pair) {
  __shared__ uint64_t s[kMergeTile];
  __shared__ int64_t split[2];
  const int tid = threadIdx.x;
  const int64_t ps = (int64_t)(blockIdx.x / tiles_per_pair) * 2 * w;  // < N by the grid
  const int64_t na = N - ps < w ? N - ps : w;
  const int64_t nb = N - ps - na < w ? N - ps - na : w;
  const int64_t d0 = (int64_t)(blockIdx.x % tiles_per_pair) * kMergeTile;
  if (d0 >= na + nb) return;  // uniform: the whole workgroup leaves
  const int64_t d1 = d0 + kMergeTile < na + nb ? d0 + kMergeTile : na + nb;
  const uint64_t* A = src + (int64_t)blockIdx.y * N + ps;
  const uint64_t* B = A + na;
  if (tid < 2) split[tid] = merge_path(A, na, B, nb, tid ? d1 : d0);
  __syncthreads();
  const int64_t a0 = split[0], b0 = d0 - a0;
  const int ca = (int)(split[1] - a0), cnt = (int)(d1 - d0), cb = cnt - ca;
  for (int i = tid; i < cnt; i += kMergeThreads) s[i] = i < ca ? A[a0 + i] : B[b0 + (i - ca)];
  __syncthreads();
  const int d = tid * kMergeItems < cnt ? tid * kMergeItems : cnt;
  int i = (int)merge_path(s, (int64_t)ca, s + ca, (int64_t)cb, (int64_t)d);
  int j = d - i;
  uint64_t* out = dst + (int64_t)blockIdx.y * N + ps + d0;
  for (int k = 0; k < kMergeItems && d + k < cnt; ++k) {
    const bool take_a = j >= cb || (i < ca && s[i] >= s[ca + j]);
    out[d + k] = take_a ? s[i++] : s[ca + j++];
  }
}

// --------------------------------------------------------------- curve pass
constexpr int kCurveThreads = 256, kCurveItems = 4, kCurveTile = kCurveThreads * kCurveItems;
constexpr int kCurveWaves = kCurveThreads / 64;

MPV_DEV uint64_t shfl_up_u64(uint64_t v, int o) {
  return (uint64_t)__shfl_up((unsigned long long)v, o, 64);
}
MPV_DEV uint64_t shfl_xor_u64(uint64_t v, int o) {
  return (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
}

// Workgroup scan of one uint64 per thread, sum or max (integers: exact in any
// order).  Returns the combination over the threads before this one (0 for
// thread 0) and sets `total`.  `wv` holds one word per wave.
template <bool IS_MAX>
MPV_DEV uint64_t block_scan_excl(uint64_t v, uint64_t* wv, uint64_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t x = shfl_up_u64(inc, o);
    if (lane >= o) inc = IS_MAX ? (x > inc ? x : inc) : inc + x;
  }
  uint64_t exc = shfl_up_u64(inc, 1);
  if (lane == 0) exc = 0;
  __syncthreads();  // the previous scan's wv reads are done
  if (lane == 63) wv[w] = inc;
  __syncthreads();
  uint64_t before = 0, all = 0;
  for (int i = 0; i < kCurveWaves; ++i) {
    const uint64_t x = wv[i];
    if (i < w) before = IS_MAX ? (x > before ? x : before) : before + x;
    all = IS_MAX ? (x > all ? x : all) : all + x;
  }
  total = all;
  return IS_MAX ? (exc > before ? exc : before) : exc + before;
}

// Label blockIdx.x.  A run end at position i is packed as (i + 1) << 32 | T[i]:
// both halves grow with i, so the maximum over earlier positions is the
// previous run end, and 0 means "none" (tp0 = fp0 = 0).
__global__ __launch_bounds__(kCurveThreads) void curve_pass_kernel(
    const uint64_t* __restrict__ keys, int64_t N, double* __restrict__ auc,
    double* __restrict__ aupr, double* __restrict__ fdr) {
  __shared__ uint64_t wv[kCurveWaves];
  __shared__ double red[kCurveWaves];
  const int tid = threadIdx.x;
  const uint64_t* k = keys + (int64_t)blockIdx.x * N;

  uint64_t cnt = 0;
  for (int64_t i = tid; i < N; i += kCurveThreads) cnt += k[i] & 1;
  uint64_t P;
  block_scan_excl<false>(cnt, wv, P);
  const uint64_t Nn = (uint64_t)N - P;
  const double dP = (double)P, dNn = (double)Nn;
  const bool has_auc = P > 0 && Nn > 0;

  uint64_t carry_t = 0, carry_e = 0, best = 0;
  double s_auc = 0.0, s_pr = 0.0;
  for (int64_t t0 = 0; t0 < N; t0 += kCurveTile) {
    const int64_t i0 = t0 + (int64_t)tid * kCurveItems;
    uint64_t key[kCurveItems + 1];
#pragma unroll
    for (int e = 0; e <= kCurveItems; ++e) key[e] = i0 + e < N ? k[i0 + e] : 0;
    uint64_t loc[kCurveItems], run = 0;
#pragma unroll
    for (int e = 0; e < kCurveItems; ++e) {
      run += i0 + e < N ? key[e] & 1 : 0;
      loc[e] = run;
    }
    uint64_t tile_t;
    const uint64_t off = carry_t + block_scan_excl<false>(run, wv, tile_t);
    uint64_t endv[kCurveItems], mine = 0;
#pragma unroll
    for (int e = 0; e < kCurveItems; ++e) {
      const int64_t i = i0 + e;
      const bool end = i < N && (i == N - 1 || (key[e] >> 1) != (key[e + 1] >> 1));
      endv[e] = end ? ((uint64_t)(i + 1) << 32) | (off + loc[e]) : 0;
      mine = endv[e] ? endv[e] : mine;  // increasing in e
    }
    uint64_t tile_e;
    uint64_t prev = block_scan_excl<true>(mine, wv, tile_e);
    prev = prev > carry_e ? prev : carry_e;
#pragma unroll
    for (int e = 0; e < kCurveItems; ++e) {
      if (!endv[e]) continue;
      const uint64_t n1 = endv[e] >> 32, tpi = endv[e] & 0xFFFFFFFFull;  // i + 1, T[i]
      const uint64_t s = prev >> 32, tp0i = prev & 0xFFFFFFFFull;       // run start, T[s-1]
      const double tp = (double)tpi, fp = (double)(n1 - tpi);
      const double tp0 = (double)tp0i, fp0 = (double)(s - tp0i);
      if (has_auc) s_auc += (fp - fp0) / dNn * ((tp + tp0) / dP) / 2.0;
      const double prec = tp / (tp + fp), rec = P ? tp / dP : 1.0;
      const double prec0 = s ? tp0 / (tp0 + fp0) : 1.0;
      const double rec0 = s ? (P ? tp0 / dP : 1.0) : 0.0;
      s_pr += (rec - rec0) * (prec + prec0) / 2.0;
      // evals.py:134-135 tests 1 - precision <= 0.5 in fp64.  2 tp >= tp + fp is
      // exactly that predicate: tp / (tp + fp) rounds monotonically and equals
      // 0.5 only when 2 tp = tp + fp, and below that it is at most
      // 0.5 - 1 / (2 (tp + fp)), far more than an ulp away for tp + fp < 2^31.
      if (2 * tpi >= n1) best = endv[e];  // increasing in e and over the tiles
      prev = endv[e];
    }
    carry_t += tile_t;
    carry_e = tile_e > carry_e ? tile_e : carry_e;
  }
  const double t_auc = block_sum_f64<kCurveWaves>(s_auc, red);
  const double t_pr = block_sum_f64<kCurveWaves>(s_pr, red);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t x = shfl_xor_u64(best, o);
    best = x > best ? x : best;
  }
  __syncthreads();
  if ((tid & 63) == 0) wv[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < kCurveWaves; ++i) best = wv[i] > best ? wv[i] : best;
    auc[blockIdx.x] = has_auc ? t_auc : NAN;  // roc_auc_score: one class only
    aupr[blockIdx.x] = t_pr;
    fdr[blockIdx.x] = best ? (double)(best & 0xFFFFFFFFull) / dP : 0.0;  // best: tp >= 1, so P >= 1
  }
}

// ---------------------------------------------------------------- aggregate
// Block b: mean, median, population variance of metric b over its non-NaN
// labels -> agg[3 b .. 3 b + 2]; all NaN when no label is kept.
__global__ __launch_bounds__(kSortThreads) void curve_agg_kernel(const double* __restrict__ auc,
                                                                 const double* __restrict__ aupr,
                                                                 const double* __restrict__ fdr,
                                                                 int L, double* __restrict__ agg) {
  __shared__ double s[kCurveMaxL];
  __shared__ double red[kSortThreads / 64];
  const int tid = threadIdx.x;
  const double* v = blockIdx.x == 0 ? auc : (blockIdx.x == 1 ? aupr : fdr);
  int m = 64;
  while (m < L) m <<= 1;  // m <= kCurveMaxL
  double cnt = 0.0, sum = 0.0;
  for (int i = tid; i < m; i += kSortThreads) {
    const double x = i < L ? v[i] : NAN;
    const bool ok = x == x;
    s[i] = ok ? x : INFINITY;  // dropped labels and the pad sort to the end
    cnt += ok ? 1.0 : 0.0;
    sum += ok ? x : 0.0;
  }
  const double kept = block_sum_f64<kSortThreads / 64>(cnt, red);  // a count <= 4096: exact
  const double mean = block_sum_f64<kSortThreads / 64>(sum, red) / kept;
  double q = 0.0;
  for (int i = tid; i < L; i += kSortThreads) {
    const double x = v[i];
    if (x == x) q += (x - mean) * (x - mean);
  }
  // also the barrier after the writes of s
  const double var = block_sum_f64<kSortThreads / 64>(q, red) / kept;
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (m >> 1); t += kSortThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int p = i | j;
        const bool asc = (i & k) == 0;
        const double a = s[i], b = s[p];
        if ((a > b) == asc) {
          s[i] = b;
          s[p] = a;
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    const int n = (int)kept;
    double* o = agg + 3 * blockIdx.x;
    o[0] = n ? mean : NAN;
    o[1] = n ? ((n & 1) ? s[n >> 1] : (s[(n >> 1) - 1] + s[n >> 1]) / 2.0) : NAN;
    o[2] = n ? var : NAN;
  }
}

static bool curve_chunk_ok(int64_t c) {
  return c == 0 || (c >= 64 && c <= kCurveChunk && (c & (c - 1)) == 0);
}

static bool curve_shape_ok(int64_t N, int64_t L) { return N > 0 && L > 0 && N <= INT32_MAX; }

struct CurveWs {
  uint64_t* cur;  // (L, N) keys
  uint64_t* alt;  // the merge passes' second buffer, when chunks are merged
};

static CurveWs curve_ws(Workspace& ws, int64_t N, int64_t L, int64_t chunk) {
  CurveWs c;
  c.cur = ws.take<uint64_t>(N, L);
  c.alt = ws.take<uint64_t>(N > (chunk ? chunk : kCurveChunk) ? N : 0, L);
  return c;
}

}  // namespace mpv

using namespace mpv;

extern "C" {

size_t mpv_curves_workspace_bytes(int64_t N, int64_t L, int64_t chunk) {
  if (!curve_shape_ok(N, L) || !curve_chunk_ok(chunk)) return 0;
  return layout_bytes(curve_ws, N, L, chunk);
}

int mpv_curve_metrics(const mpv_curve_args* a, void* workspace, size_t workspace_bytes,
                      void* stream) {
  MPV_REQUIRE(a && a->pred && a->target && a->auc && a->aupr && a->fdr && a->agg,
              "NULL pointer in mpv_curve_args");
  MPV_REQUIRE(curve_shape_ok(a->N, a->L), "bad curve shape N=%lld L=%lld", (long long)a->N,
              (long long)a->L);
  MPV_REQUIRE(a->L <= kCurveMaxL, "label_dim %lld > %d is not supported by the curve aggregate",
              (long long)a->L, kCurveMaxL);
  MPV_REQUIRE(curve_chunk_ok(a->chunk),
              "chunk %lld must be 0 or a power of two in [64, %d]", (long long)a->chunk,
              kCurveChunk);
  Workspace carve(workspace);
  const CurveWs ws = curve_ws(carve, a->N, a->L, a->chunk);
  MPV_REQUIRE(carve.fits(workspace_bytes), "curve workspace too small");
  hipStream_t st = as_stream(stream);
  const int64_t N = a->N;
  const int L = (int)a->L, chunk = a->chunk ? (int)a->chunk : kCurveChunk;
  uint64_t *cur = ws.cur, *alt = ws.alt;
  MPV_LAUNCH("curve_keys", curve_keys_kernel,
             dim3((unsigned)cdiv(N, kKeyTile), (unsigned)cdiv(L, kKeyTile)), dim3(256), 0, st,
             a->pred, a->target, N, L, cur);
  MPV_LAUNCH("curve_sort", curve_sort_kernel, dim3((unsigned)cdiv(N, chunk), (unsigned)L),
             dim3(kSortThreads), 0, st, cur, N, chunk);
  for (int64_t w = chunk; w < N; w *= 2) {
    const int64_t pair = 2 * w < N ? 2 * w : N;
    const int tpp = (int)cdiv(pair, kMergeTile);
    MPV_LAUNCH("curve_merge", curve_merge_kernel,
               dim3((unsigned)(cdiv(N, 2 * w) * tpp), (unsigned)L), dim3(kMergeThreads), 0, st,
               cur, alt, N, w, tpp);
    uint64_t* t = cur;
    cur = alt;
    alt = t;
  }
  MPV_LAUNCH("curve_pass", curve_pass_kernel, dim3((unsigned)L), dim3(kCurveThreads), 0, st, cur, N,
             a->auc, a->aupr, a->fdr);
  MPV_LAUNCH("curve_agg", curve_agg_kernel, dim3(3), dim3(kSortThreads), 0, st, a->auc, a->aupr,
             a->fdr, L, a->agg);
  return MPV_OK;
}

}  // extern "C"
