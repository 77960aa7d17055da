// Host-side helpers shared by the C-ABI entry points.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpvae_hip.h"
#include "workspace.h"

namespace mpv {

// Record a message for mpv_last_error() and return `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// After a kernel launch: MPV_OK, or MPV_ELAUNCH with the HIP error text.  For
// MPV_LAUNCH alone.
int check_launch(const char* what);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Shape sanity shared by forward and backward.
int check_shape(const mpv_shape* s);

// out[i] = sum over k < nslab of in[k * n + i], the slabs in order (util.hip);
// out_dtype MPV_F32 or MPV_F64.  The pair is two such sums in one launch, each
// with the bits of a launch of its own.
int launch_sum_slabs(const float* in, int64_t nslab, int64_t n, void* out, int out_dtype,
                     hipStream_t s);
// Whether that sum takes the split layout (16 strided slab groups per output
// element, added in order) rather than slab by slab: too few columns to hide
// the slab chain.  predict_final sums in the same order.
inline bool slab_sum_is_split(int64_t nslab, int64_t n) { return nslab >= 64 && n <= 256 * 256; }
int launch_sum_slabs_pair(const float* in0, int64_t nslab0, int64_t n0, void* out0,
                          int out0_dtype, const float* in1, int64_t nslab1, int64_t n1,
                          void* out1, int out1_dtype, hipStream_t s);

// Brackets one kernel launch with HIP events when mpv_timing_enable(1) is on
// (no cost otherwise beyond one branch).
class TimedLaunch {
 public:
  TimedLaunch(const char* kernel, hipStream_t s);
  ~TimedLaunch();

 private:
  int slot_ = -1;
  size_t pair_ = 0;
  hipStream_t s_;
};

}  // namespace mpv

// The one launch form: hipLaunchKernelGGL under a TimedLaunch scope named
// `tag`, then, the scope closed, hipGetLastError(); a failed launch returns
// MPV_ELAUNCH, its message naming `kernel`, from the enclosing function.
#define MPV_LAUNCH(tag, kernel, grid, block, shm, stream, ...)                  \
  do {                                                                         \
    {                                                                          \
      ::mpv::TimedLaunch mpv_tl_(tag, stream);                                 \
      hipLaunchKernelGGL(kernel, grid, block, shm, stream, __VA_ARGS__);       \
    }                                                                          \
    if (int mpv_rc_ = ::mpv::check_launch(#kernel)) return mpv_rc_;            \
  } while (0)

#define MPV_REQUIRE(cond, ...)                         \
  do {                                                 \
    if (!(cond)) return ::mpv::fail(MPV_EINVAL, __VA_ARGS__); \
  } while (0)
