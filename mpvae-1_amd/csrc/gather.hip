// The batch feed of a whole epoch on the device (mpvae_step.DeviceSplit,
// TrainStep.run_epoch): the reference builds every batch on the host,
//   torch.from_numpy(data.input_feat[idx]).float().to(device)
// for the features, the labels and the sensitive columns (fairsoft_train.py:
// 48-56, :235-243, :266-267) -- a numpy fancy-index gather, a dtype conversion
// and a pageable host-to-device copy, three times per step.  Here the split
// lives in device memory, the epoch's shuffled order is uploaded once, and one
// launch gathers the rows order[p .. p + B) of up to four source matrices into
// the step's input buffers.  p is a host integer or a cursor in device memory,
// so the launch is a node of the captured step graph and an epoch is N // B
// replays with nothing in between.
//
// Layout: one wave per batch row, four rows per workgroup, lanes across the
// row's columns; the sources are walked one after the other by the same wave.
// A source whose copy is raw (same element type) and whose bases and row
// pitches are 16-B aligned moves 16 bytes per lane; every other source moves
// one element per lane, cast with static_cast<float> where the destination is
// fp32 (round to nearest even from fp64 and the 64-bit integers, as torch's
// .float()).  The kernel is latency-bound (a C1 batch is 133 KB): nothing is
// tuned beyond these two paths.
//
// A row whose position or index is out of range reads nothing: it is filled
// with NaN (a floating-point destination) or zero bytes (an integer one) and
// *bad is set; *bad is never cleared here.  With `advance`, a trailing
// one-thread launch on the same stream moves the cursor: every row of the
// gather has read it before (stream order), and no workgroup waits for another.
#include <limits>

#include "abi_util.h"
#include "mpv_common.h"

namespace mpv {
namespace {

constexpr int kGatherThreads = 256;
constexpr int kGatherRows = kGatherThreads / 64;  // one wave per batch row

struct GatherBatch {
  const char* src[MPV_GATHER_MAX_SOURCES];
  char* dst[MPV_GATHER_MAX_SOURCES];
  int64_t cols[MPV_GATHER_MAX_SOURCES];
  int src_elem[MPV_GATHER_MAX_SOURCES];
  int cast[MPV_GATHER_MAX_SOURCES];   // 1: the destination is fp32 and the source is not
  int vec16[MPV_GATHER_MAX_SOURCES];  // 1: raw copy, 16 bytes per lane
  int n_sources;
  int64_t n_rows, n_idx, B, start;
  const int64_t* idx;
  const int64_t* pos;
  uint8_t* bad;
};

MPV_DEV int elem_bytes(int e) {
  return e == MPV_EL_U8 ? 1 : (e == MPV_EL_F32 || e == MPV_EL_I32) ? 4 : 8;
}

// dst[c] = float(src[c]) over one row
template <typename S>
MPV_DEV void cast_row(const char* src, char* dst, int64_t cols, int lane) {
  const S* s = reinterpret_cast<const S*>(src);
  float* d = reinterpret_cast<float*>(dst);
  for (int64_t c = lane; c < cols; c += 64) d[c] = static_cast<float>(s[c]);
}

template <typename W>
MPV_DEV void copy_row(const char* src, char* dst, int64_t n, int lane) {
  const W* s = reinterpret_cast<const W*>(src);
  W* d = reinterpret_cast<W*>(dst);
  for (int64_t c = lane; c < n; c += 64) d[c] = s[c];
}

template <typename W>
MPV_DEV void fill_row(char* dst, int64_t n, W v, int lane) {
  W* d = reinterpret_cast<W*>(dst);
  for (int64_t c = lane; c < n; c += 64) d[c] = v;
}

// A row that has no source row: NaN in a floating-point destination, zero
// bytes in an integer one.
MPV_DEV void poison_row(char* dst, int64_t cols, int dst_elem, int lane) {
  switch (dst_elem) {
    case MPV_EL_F32: fill_row<float>(dst, cols, std::numeric_limits<float>::quiet_NaN(), lane); break;
    case MPV_EL_F64: fill_row<double>(dst, cols, std::numeric_limits<double>::quiet_NaN(), lane); break;
    case MPV_EL_I32: fill_row<int32_t>(dst, cols, 0, lane); break;
    case MPV_EL_I64: fill_row<int64_t>(dst, cols, 0, lane); break;
    default: fill_row<uint8_t>(dst, cols, 0, lane); break;
  }
}

__global__ __launch_bounds__(kGatherThreads) void gather_batch_kernel(GatherBatch a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kGatherRows + (threadIdx.x >> 6);
  if (r >= a.B) return;
  const int64_t p = a.pos != nullptr ? *a.pos : a.start;
  // p + r in [0, n_idx), decided before the sum is formed (p may sit at either
  // end of the int64 range; r and n_idx are non-negative)
  bool ok = p >= -r && p < a.n_idx - r;
  int64_t row = 0;
  if (ok) {
    row = a.idx != nullptr ? a.idx[p + r] : p + r;
    ok = row >= 0 && row < a.n_rows;
  }
  if (!ok && lane == 0) *a.bad = 1;
#pragma unroll
  for (int k = 0; k < MPV_GATHER_MAX_SOURCES; ++k) {
    if (k >= a.n_sources) break;
    const int se = a.src_elem[k];
    const int de = a.cast[k] ? (int)MPV_EL_F32 : se;
    const int64_t cols = a.cols[k];
    char* d = a.dst[k] + r * cols * elem_bytes(de);
    if (!ok) {
      poison_row(d, cols, de, lane);
      continue;
    }
    const int64_t src_pitch = cols * elem_bytes(se);
    const char* s = a.src[k] + row * src_pitch;
    if (a.vec16[k]) {
      copy_row<uint4>(s, d, src_pitch >> 4, lane);
    } else if (!a.cast[k]) {
      switch (elem_bytes(se)) {
        case 1: copy_row<uint8_t>(s, d, cols, lane); break;
        case 4: copy_row<uint32_t>(s, d, cols, lane); break;
        default: copy_row<uint64_t>(s, d, cols, lane); break;
      }
    } else {
      switch (se) {
        case MPV_EL_F64: cast_row<double>(s, d, cols, lane); break;
        case MPV_EL_I32: cast_row<int32_t>(s, d, cols, lane); break;
        case MPV_EL_I64: cast_row<int64_t>(s, d, cols, lane); break;
        default: cast_row<uint8_t>(s, d, cols, lane); break;
      }
    }
  }
}

// After the gather, in stream order: the cursor moves past the batch.
__global__ __launch_bounds__(64) void gather_advance_kernel(int64_t* pos, int64_t B) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *pos += B;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace mpv

using namespace mpv;

extern "C" int mpv_gather_batch(const mpv_gather_args* args, void* stream) {
  MPV_REQUIRE(args != nullptr, "gather_batch: args is NULL");
  MPV_REQUIRE(args->n_sources >= 1 && args->n_sources <= MPV_GATHER_MAX_SOURCES,
              "gather_batch: 1..%d sources per launch (got %d)", MPV_GATHER_MAX_SOURCES,
              args->n_sources);
  MPV_REQUIRE(args->B >= 1 && args->B <= (int64_t(1) << 31) - kGatherRows,
              "gather_batch: B must be in [1, 2^31) (got %lld)", (long long)args->B);
  MPV_REQUIRE(args->n_rows >= 0 && args->n_idx >= 0, "gather_batch: negative n_rows or n_idx");
  MPV_REQUIRE(args->bad != nullptr, "gather_batch: NULL bad flag");
  MPV_REQUIRE(args->advance == 0 || args->advance == 1, "gather_batch: advance must be 0 or 1");
  MPV_REQUIRE(!args->advance || args->pos != nullptr,
              "gather_batch: advance needs a device cursor (pos is NULL)");
  GatherBatch a = {};
  a.n_sources = args->n_sources;
  for (int k = 0; k < args->n_sources; ++k) {
    const int se = args->src_elem[k], de = args->dst_elem[k];
    MPV_REQUIRE(se >= MPV_EL_F32 && se <= MPV_EL_U8, "gather_batch: unknown element type %d "
                "(source %d)", se, k);
    MPV_REQUIRE(de == MPV_EL_F32 || de == se, "gather_batch: dst_elem must be fp32 or the "
                "source's element type (source %d: %d -> %d)", k, se, de);
    MPV_REQUIRE(args->cols[k] >= 1, "gather_batch: cols must be >= 1 (source %d)", k);
    MPV_REQUIRE(args->src[k] != nullptr && args->dst[k] != nullptr,
                "gather_batch: NULL src or dst (source %d)", k);
    a.src[k] = static_cast<const char*>(args->src[k]);
    a.dst[k] = static_cast<char*>(args->dst[k]);
    a.cols[k] = args->cols[k];
    a.src_elem[k] = se;
    a.cast[k] = de != se;
    const int64_t eb = se == MPV_EL_U8 ? 1 : (se == MPV_EL_F32 || se == MPV_EL_I32) ? 4 : 8;
    a.vec16[k] = !a.cast[k] && (args->cols[k] * eb) % 16 == 0 && aligned16(args->src[k]) &&
                 aligned16(args->dst[k]);
  }
  a.n_rows = args->n_rows;
  a.n_idx = args->n_idx;
  a.B = args->B;
  a.start = args->start;
  a.idx = args->idx;
  a.pos = args->pos;
  a.bad = args->bad;
  hipStream_t s = as_stream(stream);
  MPV_LAUNCH("gather_batch", gather_batch_kernel, dim3((unsigned)cdiv(a.B, kGatherRows)),
             dim3(kGatherThreads), 0, s, a);
  if (args->advance)
    MPV_LAUNCH("gather_batch", gather_advance_kernel, dim3(1), dim3(64), 0, s, args->pos, a.B);
  return MPV_OK;
}
