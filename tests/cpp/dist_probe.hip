// Test-only probe of the device's scalar samplers, for tests/test_dist_samplers_gpu.py.
//
// The kernels here instantiate the product's own device functions -- d_exp_rand, d_norm_rand,
// d_runif, d_random_int, d_rtrun_exp, d_rgamma_scale, d_draw_variance (device_rng.h) and
// ar_rtrun_norm_2 (ar_trunc_device.h) over SeqRng and WinRng -- and restate none of them.  The
// conventions are those of rng_probe.hip: every exported wrapper takes host arrays with explicit
// lengths (in elements), checks ON THE HOST that the request fits them and that every argument
// is one the device's loops end for (DP_BAD_REQUEST instead of a launch where not), allocates
// device buffers of exactly those lengths, copies everything in -- the output too, which the
// caller has filled with a sentinel and extended by guard bands --, launches on the null stream,
// synchronises, copies the writable buffer back whole and returns the hipError_t.
//
// A request is n draws of ONE function, draw i with its own four arguments args[4 i ..] and
// (unless chained) its own slot SeqRng::slot(key, index0 + i, stride, serve), so that it starts
// at a known position whatever draw i - 1 consumed.  Per draw DP_WORDS words come back:
//   0, 1  the value's bits as lane 0 and lane 63 saw them (d_random_int: the integer, sign-extended)
//   2, 3  the view's final position, as lane 0 / lane 63
//   4, 5  the view's final stream id (a slot's spill shows there)
//   6, 7  *bad
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "ar_trunc_device.h"

using namespace boom_amd;

namespace {

enum : int { DP_BAD_REQUEST = -1 };
enum : int { DP_WORDS = 8, DP_NARGS = 4 };
enum : int { FN_EXP = 0, FN_NORM, FN_RUNIF, FN_RANDOM_INT, FN_RTRUN_EXP, FN_RGAMMA, FN_VARIANCE, FN_RTRUN_NORM_2, FN_COUNT };
enum : int { VIEW_SEQ = 0, VIEW_WIN = 1 };
// uniform: every lane of every wavefront of the workgroup makes every draw, with the same
// arguments; per lane: draw i is made by lane i % 64 alone, in rounds of 64 draws
enum : int { MODE_UNIFORM = 0, MODE_PER_LANE = 1 };

template <class T>
struct Dev {
  T *ptr = nullptr;
  T *host;
  size_t bytes;
  hipError_t err = hipSuccess;
  Dev(const T *h, size_t count) : host(const_cast<T *>(h)), bytes(count * sizeof(T)) {
    if (!h || !count) return;
    err = hipMalloc((void **)&ptr, bytes);
    if (err == hipSuccess) err = hipMemcpy(ptr, h, bytes, hipMemcpyHostToDevice);
  }
  hipError_t back() { return ptr ? hipMemcpy(host, ptr, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
  ~Dev() {
    if (ptr) (void)hipFree(ptr);
  }
  Dev(const Dev &) = delete;
};

#define DP_TRY(expr)                              \
  do {                                            \
    hipError_t e__ = (expr);                      \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)

__device__ __forceinline__ uint64_t f64_bits(double x) { return __builtin_bit_cast(uint64_t, x); }
__device__ __forceinline__ double uniform_f64(double v) {
  const uint64_t b = f64_bits(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

struct Request {
  PhiloxKey key;
  uint64_t index0;
  uint32_t stride, serve;
  int64_t n;
  int chained;   // one view from position index0 * stride on, draw after draw (no slots)
};

template <class R>
__device__ __forceinline__ R view_at(const Request &q, int64_t i, int lane);
template <>
__device__ __forceinline__ SeqRng view_at<SeqRng>(const Request &q, int64_t i, int lane) {
  if (q.chained) return SeqRng{q.key, q.index0 * q.stride};
  return SeqRng::slot(q.key, q.index0 + (uint64_t)i, q.stride, q.serve);
}
template <>
__device__ __forceinline__ WinRng view_at<WinRng>(const Request &q, int64_t i, int lane) {
  WinRng w;   // (no slots: the host asks for serve == stride)
  w.init(q.key, lane, (q.index0 + (uint64_t)(q.chained ? 0 : i)) * q.stride);
  return w;
}

template <int FN, class R>
__device__ __forceinline__ uint64_t draw_one(R &r, const double *a, int *bad) {
  if constexpr (FN == FN_EXP) {
    return f64_bits(d_exp_rand(r));
  } else if constexpr (FN == FN_NORM) {
    return f64_bits(d_norm_rand(r));
  } else if constexpr (FN == FN_RUNIF) {
    return f64_bits(d_runif(r, a[0], a[1]));
  } else if constexpr (FN == FN_RANDOM_INT) {
    return (uint64_t)(int64_t)d_random_int(r, (int)a[0], (int)a[1]);
  } else if constexpr (FN == FN_RTRUN_EXP) {
    return f64_bits(d_rtrun_exp(r, a[0], a[1], a[2]));
  } else if constexpr (FN == FN_RGAMMA) {
    return f64_bits(d_rgamma_scale(r, a[0], a[1], bad));
  } else if constexpr (FN == FN_VARIANCE) {
    return f64_bits(d_draw_variance(r, a[0], a[1], a[2], bad));
  } else {
    static_assert(FN == FN_RTRUN_NORM_2 && std::is_same<R, SeqRng>::value, "ar_rtrun_norm_2 reads a SeqRng");
    return f64_bits(ar_rtrun_norm_2(r, a[0], a[1], a[2], a[3], bad));
  }
}

// out[((wave * n + i) * DP_WORDS) + word]; 64 or 256 threads, every one active
template <int FN, class R>
__global__ void uniform_kernel(Request q, const double *args, uint64_t *out) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int w = lane == 0 ? 0 : (lane == 63 ? 1 : -1);
  R r = view_at<R>(q, 0, lane);
  for (int64_t i = 0; i < q.n; ++i) {
    if (!q.chained) r = view_at<R>(q, i, lane);
    double a[DP_NARGS];
    for (int j = 0; j < DP_NARGS; ++j) a[j] = uniform_f64(args[DP_NARGS * i + j]);
    int bad = 0;
    const uint64_t v = draw_one<FN>(r, a, &bad);
    if (w >= 0) {
      uint64_t *o = out + ((int64_t)wave * q.n + i) * DP_WORDS;
      o[0 + w] = v;
      o[2 + w] = stream_pos(r);
      o[4 + w] = stream_key(r).stream;
      o[6 + w] = (uint64_t)(int64_t)bad;
    }
  }
}

// draw i by lane i % 64 alone: its own arguments, its own slot; both words of a pair are the lane's
template <int FN>
__global__ void __launch_bounds__(64) per_lane_kernel(Request q, const double *args, uint64_t *out) {
  const int lane = (int)(threadIdx.x & 63);
  for (int64_t i = lane; i < q.n; i += 64) {
    SeqRng r = view_at<SeqRng>(q, i, lane);
    double a[DP_NARGS];
    for (int j = 0; j < DP_NARGS; ++j) a[j] = args[DP_NARGS * i + j];
    int bad = 0;
    const uint64_t v = draw_one<FN>(r, a, &bad);
    uint64_t *o = out + i * DP_WORDS;
    o[0] = o[1] = v;
    o[2] = o[3] = stream_pos(r);
    o[4] = o[5] = stream_key(r).stream;
    o[6] = o[7] = (uint64_t)(int64_t)bad;
  }
}

bool positive(double x) { return std::isfinite(x) && x > 0.0; }

// the arguments for which every loop of the device function ends
bool args_ok(int fn, int mode, const double *a) {
  switch (fn) {
    case FN_EXP:
    case FN_NORM:
      return true;
    case FN_RUNIF:
      return std::isfinite(a[0]) && std::isfinite(a[1]);
    case FN_RANDOM_INT:
      return a[0] == std::floor(a[0]) && a[1] == std::floor(a[1]) && a[0] >= (double)INT_MIN && a[1] < (double)INT_MAX &&
             a[0] <= a[1];
    case FN_RTRUN_EXP:
      return positive(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]) && a[1] < a[2];
    case FN_RGAMMA:
      // (the shape below .3 broadcasts lane 0's draw: wave-uniform callers only)
      return positive(a[0]) && positive(a[1]) && (mode == MODE_UNIFORM || a[0] >= .3);
    case FN_VARIANCE: {
      const double DF = a[0], SS = a[1], sigma_max = a[2];
      if (!(DF >= 0.0) || !(SS >= 0.0) || !(sigma_max >= 0.0)) return false;   // (NaN: false)
      if (sigma_max == 0.0) return true;
      if (!positive(DF / 2) || !positive(SS / 2) || !positive(1.0 / (SS / 2))) return false;
      if (std::isinf(sigma_max)) return true;
      return positive(1.0 / (sigma_max * sigma_max));
    }
    case FN_RTRUN_NORM_2:
      return std::isfinite(a[0]) && positive(a[1]) && std::isfinite(a[2]) && std::isfinite(a[3]) && a[2] < a[3];
  }
  return false;
}

template <int FN>
void launch(int view, int mode, int threads, const Request &q, const double *args, uint64_t *out) {
  if (mode == MODE_PER_LANE) {
    if constexpr (FN <= FN_RGAMMA) hipLaunchKernelGGL(per_lane_kernel<FN>, dim3(1), dim3(64), 0, nullptr, q, args, out);
  } else if (view == VIEW_WIN) {
    if constexpr (FN != FN_RTRUN_NORM_2)
      hipLaunchKernelGGL((uniform_kernel<FN, WinRng>), dim3(1), dim3(threads), 0, nullptr, q, args, out);
  } else {
    hipLaunchKernelGGL((uniform_kernel<FN, SeqRng>), dim3(1), dim3(threads), 0, nullptr, q, args, out);
  }
}

}  // namespace

extern "C" {

int dp_words() { return DP_WORDS; }
int dp_nargs() { return DP_NARGS; }
int dp_spill_shift() { return SPILL_SHIFT; }

// args: nargs >= 4 n; out: nout >= (threads / 64) * n * DP_WORDS.  threads: 64, or 256 (four
// wavefronts that make the same draws).  view 1 (WinRng): uniform mode, serve == stride, not
// ar_rtrun_norm_2 (which reads a SeqRng).  mode 1 (per lane): SeqRng, 64 threads, the functions
// whose lanes are independent (d_rgamma_scale from shape .3 on).
int dp_draws(int fn, int view, int mode, int threads, int chained, uint32_t k0, uint32_t k1, uint32_t chain,
             uint32_t stream, uint64_t index0, uint32_t stride, uint32_t serve, int64_t n, const double *args,
             size_t nargs, uint64_t *out, size_t nout) {
  if (!args || !out || fn < 0 || fn >= FN_COUNT || n < 1 || n > (1 << 18)) return DP_BAD_REQUEST;
  if ((view != VIEW_SEQ && view != VIEW_WIN) || (mode != MODE_UNIFORM && mode != MODE_PER_LANE)) return DP_BAD_REQUEST;
  if (threads != 64 && threads != 256) return DP_BAD_REQUEST;
  if (mode == MODE_PER_LANE && (view != VIEW_SEQ || threads != 64 || chained || fn > FN_RGAMMA)) return DP_BAD_REQUEST;
  if (view == VIEW_WIN && (fn == FN_RTRUN_NORM_2 || serve != stride)) return DP_BAD_REQUEST;
  if (stride < 1 || stride > (1u << 20) || serve > stride || index0 > (1ull << 40)) return DP_BAD_REQUEST;
  if (stream & SPILL_STREAM_BIT) return DP_BAD_REQUEST;
  const size_t waves = (size_t)threads / 64;
  if ((size_t)n * DP_NARGS > nargs || waves * (size_t)n * DP_WORDS > nout) return DP_BAD_REQUEST;
  for (int64_t i = 0; i < n; ++i)
    if (!args_ok(fn, mode, args + DP_NARGS * i)) return DP_BAD_REQUEST;
  Dev<double> dA(args, nargs);
  Dev<uint64_t> dO(out, nout);
  DP_TRY(dA.err); DP_TRY(dO.err);
  const Request q{PhiloxKey{k0, k1, chain, stream}, index0, stride, serve, n, chained ? 1 : 0};
  switch (fn) {
    case FN_EXP: launch<FN_EXP>(view, mode, threads, q, dA.ptr, dO.ptr); break;
    case FN_NORM: launch<FN_NORM>(view, mode, threads, q, dA.ptr, dO.ptr); break;
    case FN_RUNIF: launch<FN_RUNIF>(view, mode, threads, q, dA.ptr, dO.ptr); break;
    case FN_RANDOM_INT: launch<FN_RANDOM_INT>(view, mode, threads, q, dA.ptr, dO.ptr); break;
    case FN_RTRUN_EXP: launch<FN_RTRUN_EXP>(view, mode, threads, q, dA.ptr, dO.ptr); break;
    case FN_RGAMMA: launch<FN_RGAMMA>(view, mode, threads, q, dA.ptr, dO.ptr); break;
    case FN_VARIANCE: launch<FN_VARIANCE>(view, mode, threads, q, dA.ptr, dO.ptr); break;
    default: launch<FN_RTRUN_NORM_2>(view, mode, threads, q, dA.ptr, dO.ptr); break;
  }
  DP_TRY(hipGetLastError());
  DP_TRY(hipDeviceSynchronize());
  return (int)dO.back();
}

}  // extern "C"
