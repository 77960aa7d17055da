// The threshold sweep of validate_mpvae (fairsoft_train.py:400-416) on the
// device: evals.compute_metrics(pred, target, thr, all_metrics=False)
// (evals.py:178-238) for up to 64 thresholds from one read of the validation
// split.  Row j of the (n_thr, 8) table is what metric_rows / metric_cols /
// metric_final (fairness.hip) give at thr[j]: [ACC, HA, ebF1, miF1, maF1,
// p@1, p@3, p@5].
//
//   sweep_zero_kernel   L > 64 only: clears the per-row words that the scan's
//                       chunks add into.
//   sweep_scan_kernel   workgroup (row block, 64-label chunk), one wave per row
//                       of the block at a time.  Per threshold one compare per
//                       lane and the ballots P (prediction, !(p < thr)) and T
//                       (target): tp = popc(P & T), sum_p = popc(P), xor =
//                       popc(P ^ T), packed with sum_t into one 64-bit word per
//                       (row, threshold), 16 bits each (L <= 4096).  Lane j
//                       keeps threshold j's word and stores it (L <= 64) or
//                       adds it to the row's word (one integer atomic per lane
//                       and chunk).  Each lane also counts its label's
//                       predicted positives and true positives per threshold
//                       (two 16-bit halves of one register: a workgroup owns at
//                       most 65535 rows) and its positives; the four waves add
//                       them in LDS and the workgroup writes one partial.  The
//                       top-5 hits of a row (threshold-free) are taken by one of
//                       the row's chunks -- the block's turn number modulo the
//                       chunk count -- which walks the whole row once with the
//                       ArgMax / better rule of metric_rows_kernel.
//   sweep_reduce_kernel two kinds of workgroup in one launch.  Row workgroups:
//                       lane j, a wave per row: the row's terms at threshold j
//                       (all labels equal, xor count, the fp32 example-F1
//                       quotient) summed per workgroup.  Label workgroups
//                       (chunk, threshold): the scan's per-label partials
//                       added over the row blocks.
//   sweep_final_kernel  workgroup j: the row partials, the labels' F1 terms
//                       from their totals, the hit counts -> table row j.
//
// Every count is an integer (exact at any N < 2^31, in any order, so the
// atomics are order-free).  The two fp64 sums -- the example-F1 quotients and
// the per-label F1 terms -- run in an order fixed by N and L alone: a wave's
// rows or a thread's labels in index order, the waves of a workgroup in order,
// the workgroups in order with a fixed shuffle tree at the end.  Two calls give
// the same bits.
#include "abi_util.h"
#include "mpv_common.h"

namespace mpv {

constexpr int kSweepThreads = 256, kSweepWaves = kSweepThreads / 64;
constexpr int kSweepMaxL = 4096;            // 16-bit fields of the row word; as mpv_curve_args
constexpr int kSweepMaxBlockRows = 65535;   // 16-bit halves of the per-label counters
constexpr int kRedThreads = 1024, kRedWaves = kRedThreads / 64;  // sweep_reduce_kernel
constexpr int kSweepRowBlocks = 4096;       // most row workgroups of sweep_reduce_kernel

// (score, index) as one integer that orders as metric_rows_kernel's ArgMax /
// better rule does: the larger score first, on a tie the larger index (-0.0
// ties with +0.0).  0 for a NaN, which is never picked, and for "none"; every
// other key is larger (-inf maps to 0x007FFFFF in the high word).
MPV_DEV uint64_t sweep_rank_key(float v, int i) {
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return v != v ? 0 : ((uint64_t)u << 32) | (uint32_t)i;
}

// Lane `lane` (a constant after unrolling) of a and of b takes the
// wave-uniform sa and sb (v_writelane_b32; the compiler has no builtin for it).
// The hazard recogniser does not look inside inline assembly, so the wait
// states that a preceding VALU write of EXEC (4) or of a source SGPR (2) would
// need on gfx950 are spent here.
MPV_DEV void sweep_writelane2(int& a, int& b, int sa, int sb, int lane) {
  asm("s_nop 3\n\tv_writelane_b32 %0, %2, %4\n\tv_writelane_b32 %1, %3, %4"
      : "+v"(a), "+v"(b)
      : "s"(sa), "s"(sb), "n"(lane));
}

struct SweepThr {
  float v[MPV_MAX_THRESHOLDS];
};

// Launch geometry and the workspace's pieces (NULL from the sizing pass).
struct SweepPlan {
  int64_t N;
  int L, n_thr, chunks;
  int64_t rows_per_block, row_blocks, blocks;  // scan grid: blocks = row_blocks * chunks
  int64_t fin_rows, fin_blocks;                // row workgroups of sweep_reduce_kernel
  uint64_t* rowword;
  uint32_t* colpart;
  int32_t* pkpart;
  uint64_t* coltot;
  double* ef_part;
  int64_t* xs_part;
  int32_t *acc_part, *nef_part;
};

static SweepPlan sweep_plan(Workspace& ws, int64_t N, int64_t L, int64_t n_thr) {
  SweepPlan p{};
  p.N = N;
  p.L = (int)L;
  p.n_thr = (int)n_thr;
  p.chunks = (int)cdiv(L, 64);
  int64_t rb = (int64_t)4 * num_cus() / p.chunks;
  if (rb < 1) rb = 1;
  if (rb > cdiv(N, kSweepWaves)) rb = cdiv(N, kSweepWaves);
  if (rb < cdiv(N, kSweepMaxBlockRows)) rb = cdiv(N, kSweepMaxBlockRows);
  p.rows_per_block = cdiv(N, rb);  // <= kSweepMaxBlockRows
  p.row_blocks = cdiv(N, p.rows_per_block);
  p.blocks = p.row_blocks * p.chunks;
  int64_t fb = cdiv(N, 4 * kRedWaves);  // four rows a wave while the count allows
  if (fb > kSweepRowBlocks) fb = kSweepRowBlocks;
  p.fin_rows = cdiv(N, fb);
  p.fin_blocks = cdiv(N, p.fin_rows);
  p.rowword = ws.take<uint64_t>(N, n_thr);
  p.colpart = ws.take<uint32_t>(64, n_thr + 1, p.blocks);
  p.pkpart = ws.take<int32_t>(4, p.blocks);
  p.coltot = ws.take<uint64_t>(64, n_thr + 1, p.chunks);
  p.ef_part = ws.take<double>(64, p.fin_blocks);
  p.xs_part = ws.take<int64_t>(64, p.fin_blocks);
  p.acc_part = ws.take<int32_t>(64, p.fin_blocks);
  p.nef_part = ws.take<int32_t>(64, p.fin_blocks);
  return p;
}

static bool sweep_shape_ok(int64_t N, int64_t L) {
  return N > 0 && N <= INT32_MAX && L > 0 && L <= kSweepMaxL;
}

__global__ __launch_bounds__(kSweepThreads) void sweep_zero_kernel(uint64_t* __restrict__ w,
                                                                   int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kSweepThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kSweepThreads)
    w[i] = 0;
}

// --------------------------------------------------------------------- scan
// blockIdx.x = row block * chunks + chunk.  rowword[r * n_thr + j] =
// tp | sum_p << 16 | xor << 32 | sum_t << 48 of row r at threshold j;
// colpart[(block * (n_thr + 1) + j) * 64 + lane] = the chunk's label `lane`:
// predicted positives | true positives << 16 at threshold j < n_thr, the
// label's positives at j = n_thr; pkpart[block * 4 + {0, 1, 2}] = the hits in
// the top 1 / 3 / 5 over the rows that this block ranks.
__global__ __launch_bounds__(kSweepThreads) void sweep_scan_kernel(
    const float* __restrict__ pred, const float* __restrict__ tgt, int64_t N, int L, int n_thr,
    int chunks, int64_t rows_per_block, SweepThr thr, uint64_t* __restrict__ rowword,
    uint32_t* __restrict__ colpart, int32_t* __restrict__ pkpart) {
  __shared__ uint32_t scol[MPV_MAX_THRESHOLDS + 1][64];
  __shared__ int spk[3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = (int)(blockIdx.x % chunks);
  const int64_t rb = blockIdx.x / chunks;
  const int64_t r0 = rb * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
  for (int i = tid; i < (MPV_MAX_THRESHOLDS + 1) * 64; i += kSweepThreads) (&scol[0][0])[i] = 0;
  if (tid < 3) spk[tid] = 0;
  __syncthreads();

  const int l = c * 64 + lane;
  const bool valid = l < L;
  uint32_t cnt[MPV_MAX_THRESHOLDS];
#pragma unroll
  for (int j = 0; j < MPV_MAX_THRESHOLDS; ++j) cnt[j] = 0;
  uint32_t lpos = 0;
  int h1 = 0, h3 = 0, h5 = 0;
  float p_next = 0.0f, t_next = 0.0f;
  if (valid && r0 + wv < r1) {
    p_next = pred[(r0 + wv) * L + l];
    t_next = tgt[(r0 + wv) * L + l];
  }
  for (int64_t r = r0 + wv; r < r1; r += kSweepWaves) {
    const float* pr = pred + r * L;
    const float* tr = tgt + r * L;
    const float p = p_next;
    const bool tb = t_next == 1.0f;  // 0 in a lane past L
    if (valid && r + kSweepWaves < r1) {  // the next row's loads fly under this row's compares
      p_next = pred[(r + kSweepWaves) * L + l];
      t_next = tgt[(r + kSweepWaves) * L + l];
    }
    const uint64_t T = __builtin_amdgcn_ballot_w64(tb);
    const uint64_t V = __builtin_amdgcn_ballot_w64(valid);  // the chunk's lanes below L
    const uint32_t inc = tb ? 0x10001u : 1u;
    lpos += tb ? 1u : 0u;
    // per row, so that the 64 `j < nt` tests below stay scalar compares
    // instead of 64 loop-invariant lane masks held across the row loop
    int nt = n_thr;
    asm volatile("" : "+s"(nt));
    const uint32_t st16 = (uint32_t)__popcll(T) << 16;
    int mine_lo = 0, mine_hi = 0;  // lane j: tp | sum_p << 16, xor | sum_t << 16 at threshold j
#pragma unroll
    for (int j = 0; j < MPV_MAX_THRESHOLDS; ++j) {
      if (j < nt) {  // uniform
        const bool pb = !(p < thr.v[j]);  // evals.py:201-202; a NaN score predicts 1
        const uint64_t P = __builtin_amdgcn_ballot_w64(pb) & V;
        cnt[j] += pb ? inc : 0u;  // a lane past L counts what nobody reads
        const uint32_t lo = (uint32_t)__popcll(P & T) | ((uint32_t)__popcll(P) << 16);
        const uint32_t hi = (uint32_t)__popcll(P ^ T) | st16;
        sweep_writelane2(mine_lo, mine_hi, (int)lo, (int)hi, j);
      }
    }
    const uint64_t mine = (uint64_t)(uint32_t)mine_lo | ((uint64_t)(uint32_t)mine_hi << 32);
    if (lane < n_thr) {
      uint64_t* dst = rowword + r * n_thr + lane;
      if (chunks == 1) *dst = mine;
      else atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)mine);
    }
    // the block's waves rank in the same turns (turn % chunks == chunk), so
    // no wave of a block carries the ranking of all its rows
    if ((int)(((r - r0) / kSweepWaves) % chunks) == c) {  // uniform: this wave ranks row r
      // each lane's five best of its labels in one pass over the row, then
      // five rounds of a wave maximum over the lanes' heads
      uint64_t top[5] = {0, 0, 0, 0, 0};
#pragma unroll 4
      for (int q = lane; q < L; q += 64) {
        uint64_t x = sweep_rank_key(pr[q], q);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const uint64_t hi = x > top[k] ? x : top[k];
          x = x > top[k] ? top[k] : x;
          top[k] = hi;
        }
      }
      int chosen[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        uint64_t m = top[0];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
          const uint64_t x = (uint64_t)__shfl_xor((unsigned long long)m, o, 64);
          m = x > m ? x : m;
        }
        chosen[k] = m ? (int)(uint32_t)m : -1;  // the same in every lane
        if (m && top[0] == m) {  // the one lane that held it (the index is in the key)
#pragma unroll
          for (int u = 0; u < 4; ++u) top[u] = top[u + 1];
          top[4] = 0;
        }
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int hit = (chosen[k] >= 0 && tr[chosen[k] >= 0 ? chosen[k] : 0] == 1.0f) ? 1 : 0;
        h1 += k < 1 ? hit : 0;
        h3 += k < 3 ? hit : 0;
        h5 += hit;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < MPV_MAX_THRESHOLDS; ++j)
    if (j < n_thr) atomicAdd(&scol[j][lane], cnt[j]);  // LDS, integers
  atomicAdd(&scol[n_thr][lane], lpos);
  if (lane == 0) {
    atomicAdd(&spk[0], h1);
    atomicAdd(&spk[1], h3);
    atomicAdd(&spk[2], h5);
  }
  __syncthreads();
  uint32_t* out = colpart + (int64_t)blockIdx.x * (n_thr + 1) * 64;
  for (int i = tid; i < (n_thr + 1) * 64; i += kSweepThreads) out[i] = (&scol[0][0])[i];
  if (tid < 3) pkpart[(int64_t)blockIdx.x * 4 + tid] = spk[tid];
}

// ------------------------------------------------------------------- reduce
// Workgroups [0, fin_blocks): workgroup b owns rows [b * fin_rows, ...); lane
// j of wave w takes rows w, w + 16, ... of them at threshold j.  Partials at
// [b * 64 + j].
MPV_DEV void sweep_reduce_rows(const uint64_t* __restrict__ rowword, int64_t N, int n_thr,
                               int64_t fin_rows, double* __restrict__ ef_part,
                               int64_t* __restrict__ xs_part, int32_t* __restrict__ acc_part,
                               int32_t* __restrict__ nef_part) {
  __shared__ double sef[kRedWaves][64];
  __shared__ int64_t sxs[kRedWaves][64];
  __shared__ int32_t sacc[kRedWaves][64], snef[kRedWaves][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * fin_rows;
  const int64_t r1 = r0 + fin_rows < N ? r0 + fin_rows : N;
  double ef = 0.0;
  int64_t xs = 0;
  int32_t acc = 0, nef = 0;
  if (lane < n_thr) {
#pragma unroll 4
    for (int64_t r = r0 + wv; r < r1; r += kRedWaves) {
      const uint64_t w = rowword[r * n_thr + lane];
      const uint32_t tp = (uint32_t)(w & 0xFFFFu), sp = (uint32_t)((w >> 16) & 0xFFFFu);
      const uint32_t xr = (uint32_t)((w >> 32) & 0xFFFFu), st = (uint32_t)(w >> 48);
      acc += xr == 0 ? 1 : 0;  // all labels equal (evals.py:13-24)
      xs += xr;
      const float den = (float)st + (float)sp;
      if (den != 0.0f) {  // metric_final_kernel's fp32 quotient
        ef += (double)((2.0f * (float)tp) / den);
        ++nef;
      }
    }
  }
  sef[wv][lane] = ef;
  sxs[wv][lane] = xs;
  sacc[wv][lane] = acc;
  snef[wv][lane] = nef;
  __syncthreads();
  if (wv == 0) {
    for (int i = 1; i < kRedWaves; ++i) {  // the waves in order
      ef += sef[i][lane];
      xs += sxs[i][lane];
      acc += sacc[i][lane];
      nef += snef[i][lane];
    }
    const int64_t o = (int64_t)blockIdx.x * 64 + lane;
    ef_part[o] = ef;
    xs_part[o] = xs;
    acc_part[o] = acc;
    nef_part[o] = nef;
  }
}

// Workgroup q = chunk * (n_thr + 1) + j past the row workgroups: the sixteen
// waves split the row blocks.  coltot[q * 64 + lane] = predicted positives |
// true positives << 32 over all rows (j = n_thr: the label's positives).
MPV_DEV void sweep_reduce_cols(const uint32_t* __restrict__ colpart, int q, int n_thr, int chunks,
                               int64_t row_blocks, uint64_t* __restrict__ coltot) {
  __shared__ uint32_t slo[kRedWaves][64], shi[kRedWaves][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = q / (n_thr + 1), j = q % (n_thr + 1);
  uint32_t lo = 0, hi = 0;  // < 2^31 each: counts of rows
#pragma unroll 8
  for (int64_t rb = wv; rb < row_blocks; rb += kRedWaves) {
    const uint32_t w = colpart[((rb * chunks + c) * (int64_t)(n_thr + 1) + j) * 64 + lane];
    lo += w & 0xFFFFu;
    hi += w >> 16;
  }
  slo[wv][lane] = lo;
  shi[wv][lane] = hi;
  __syncthreads();
  if (wv == 0) {
    for (int i = 1; i < kRedWaves; ++i) {
      lo += slo[i][lane];
      hi += shi[i][lane];
    }
    coltot[(int64_t)q * 64 + lane] = (uint64_t)lo | ((uint64_t)hi << 32);
  }
}

__global__ __launch_bounds__(kRedThreads) void sweep_reduce_kernel(
    const uint64_t* __restrict__ rowword, const uint32_t* __restrict__ colpart, int64_t N,
    int n_thr, int chunks, int64_t row_blocks, int64_t fin_rows, int64_t fin_blocks,
    double* __restrict__ ef_part, int64_t* __restrict__ xs_part, int32_t* __restrict__ acc_part,
    int32_t* __restrict__ nef_part, uint64_t* __restrict__ coltot) {
  if ((int64_t)blockIdx.x < fin_blocks)  // uniform over the workgroup
    sweep_reduce_rows(rowword, N, n_thr, fin_rows, ef_part, xs_part, acc_part, nef_part);
  else
    sweep_reduce_cols(colpart, (int)(blockIdx.x - fin_blocks), n_thr, chunks, row_blocks, coltot);
}

// -------------------------------------------------------------------- final
MPV_DEV int64_t sweep_wave_sum_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (int64_t)__shfl_xor((long long)v, o, 64);
  return v;
}

// Workgroup j -> out[8 j .. 8 j + 7].  Each sum: thread t adds its items t,
// t + 256, ... in order, then a shuffle tree, then the waves in order.
__global__ __launch_bounds__(kSweepThreads) void sweep_final_kernel(
    const uint64_t* __restrict__ coltot, const int32_t* __restrict__ pkpart,
    const double* __restrict__ ef_part, const int64_t* __restrict__ xs_part,
    const int32_t* __restrict__ acc_part, const int32_t* __restrict__ nef_part, int64_t N, int L,
    int n_thr, int64_t blocks, int64_t fin_blocks, double* __restrict__ out) {
  __shared__ double sd[kSweepWaves];
  __shared__ int64_t si[10][kSweepWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = blockIdx.x;
  double ef = 0.0, ma = 0.0;
  int64_t v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // xor, acc, nef, h1, h3, h5, nma, TP, FP, FN
  for (int64_t b = tid; b < fin_blocks; b += kSweepThreads) {
    ef += ef_part[b * 64 + j];
    v[0] += xs_part[b * 64 + j];
    v[1] += acc_part[b * 64 + j];
    v[2] += nef_part[b * 64 + j];
  }
  for (int64_t b = tid; b < blocks; b += kSweepThreads) {  // every scan workgroup's hits
    v[3] += pkpart[b * 4 + 0];
    v[4] += pkpart[b * 4 + 1];
    v[5] += pkpart[b * 4 + 2];
  }
  // label l's F1 term from its totals (compute_tp_fp_fn axis=0, evals.py:85-117)
  for (int l = tid; l < L; l += kSweepThreads) {
    const int64_t base = (int64_t)(l >> 6) * (n_thr + 1);
    const uint64_t w = coltot[(base + j) * 64 + (l & 63)];
    const int64_t pos = (int64_t)(coltot[(base + n_thr) * 64 + (l & 63)] & 0xFFFFFFFFull);
    const int64_t pp = (int64_t)(w & 0xFFFFFFFFull), tp = (int64_t)(w >> 32);
    const int64_t fp = pp - tp, fn = pos - tp;
    v[7] += tp;
    v[8] += fp;
    v[9] += fn;
    const float a = (float)tp, b = (float)fp, d = (float)fn;
    const double f = (double)(2.0f * a) / (double)(2.0f * a + b + d + 1e-6f);
    if (isfinite(f)) {
      ma += f;
      ++v[6];
    }
  }
  const double efs = block_sum_f64<kSweepWaves>(ef, sd);
  const double mas = block_sum_f64<kSweepWaves>(ma, sd);
#pragma unroll
  for (int k = 0; k < 10; ++k) v[k] = sweep_wave_sum_i64(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 10; ++k) si[k][wv] = v[k];
  }
  __syncthreads();
  if (tid == 0) {
    int64_t s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < kSweepWaves; ++i)
      for (int k = 0; k < 10; ++k) s[k] += si[k][i];
    const double n = (double)N, tp2 = 2.0 * (double)s[7];
    double* o = out + (int64_t)j * 8;
    o[0] = (double)s[1] / n;
    o[1] = 1.0 - ((double)s[0] / (double)L) / n;
    o[2] = s[2] ? efs / (double)s[2] : NAN;
    o[3] = tp2 / (tp2 + (double)s[8] + (double)s[9]);
    o[4] = s[6] ? mas / (double)s[6] : NAN;
    o[5] = (double)s[3] / n;
    o[6] = ((double)s[4] / 3.0) / n;
    o[7] = ((double)s[5] / 5.0) / n;
  }
}

}  // namespace mpv

using namespace mpv;

extern "C" {

size_t mpv_sweep_workspace_bytes(int64_t N, int64_t L, int64_t n_thr) {
  if (!sweep_shape_ok(N, L) || n_thr < 1 || n_thr > MPV_MAX_THRESHOLDS) return 0;
  return layout_bytes(sweep_plan, N, L, n_thr);
}

int mpv_threshold_sweep(const mpv_sweep_args* a, void* workspace, size_t workspace_bytes,
                        void* stream) {
  MPV_REQUIRE(a && a->pred && a->target && a->out, "NULL pointer in mpv_sweep_args");
  MPV_REQUIRE(sweep_shape_ok(a->N, a->L), "bad sweep shape N=%lld L=%lld (0 < N < 2^31, 0 < L <= %d)",
              (long long)a->N, (long long)a->L, kSweepMaxL);
  MPV_REQUIRE(a->n_thr >= 1 && a->n_thr <= MPV_MAX_THRESHOLDS,
              "%lld thresholds: 1 .. %d per call", (long long)a->n_thr, MPV_MAX_THRESHOLDS);
  Workspace carve(workspace);
  const SweepPlan p = sweep_plan(carve, a->N, a->L, a->n_thr);
  MPV_REQUIRE(carve.fits(workspace_bytes), "sweep workspace too small");
  hipStream_t st = as_stream(stream);
  SweepThr thr{};
  for (int j = 0; j < p.n_thr; ++j) thr.v[j] = a->thr[j];
  if (p.chunks > 1) {
    const int64_t n = p.N * p.n_thr;
    const int64_t zb = cdiv(n, kSweepThreads * 8);
    MPV_LAUNCH("metric_sweep", sweep_zero_kernel, dim3((unsigned)(zb < 4096 ? zb : 4096)),
               dim3(kSweepThreads), 0, st, p.rowword, n);
  }
  MPV_LAUNCH("metric_sweep", sweep_scan_kernel, dim3((unsigned)p.blocks), dim3(kSweepThreads), 0, st,
             a->pred, a->target, p.N, p.L, p.n_thr, p.chunks, p.rows_per_block, thr, p.rowword,
             p.colpart, p.pkpart);
  const int64_t col_blocks = (int64_t)p.chunks * (p.n_thr + 1);
  MPV_LAUNCH("metric_sweep", sweep_reduce_kernel, dim3((unsigned)(p.fin_blocks + col_blocks)),
             dim3(kRedThreads), 0, st, p.rowword, p.colpart, p.N, p.n_thr, p.chunks, p.row_blocks,
             p.fin_rows, p.fin_blocks, p.ef_part, p.xs_part, p.acc_part, p.nef_part, p.coltot);
  MPV_LAUNCH("metric_sweep", sweep_final_kernel, dim3((unsigned)p.n_thr), dim3(kSweepThreads), 0, st,
             p.coltot, p.pkpart, p.ef_part, p.xs_part, p.acc_part, p.nef_part, p.N, p.L, p.n_thr,
             p.blocks, p.fin_blocks, a->out);
  return MPV_OK;
}

}  // extern "C"
