// Test-only probe of the device's stream readers and state-stream normals, for
// tests/test_stream_views_gpu.py and tests/test_stream_normals_gpu.py.
//
// The kernels here instantiate the product's own device functions -- SeqRng, PairRng, WinRng,
// stream_seek, seq_view / seq_resume (device_rng.h), stream_normals with NormalsInOrder
// (stream_normals.h) and LmSlots, normals_share_ctx / normals_share_chunk (kalman_lm_device.h)
// -- and restate none of them.  Every exported wrapper takes host arrays with explicit lengths
// (in elements), checks ON THE HOST that the request fits them (RP_BAD_REQUEST instead of a
// launch where it does not), allocates device buffers of exactly those lengths, copies
// everything in -- outputs too, which the caller has filled with a sentinel and extended by
// guard bands --, launches on the null stream, synchronises, copies every writable buffer back
// whole and returns the hipError_t.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kalman_lm_device.h"

using namespace boom_amd;

namespace {

enum : int { RP_BAD_REQUEST = -1 };
// operations of rp_views: {code, argument} pairs of int64
enum : int64_t { OP_DRAW = 0, OP_SEEK = 1, OP_SEQ_ROUND_TRIP = 2 };

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

#define RP_TRY(expr)                              \
  do {                                            \
    hipError_t e__ = (expr);                      \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)

__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uint64_t)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint64_t f64_bits(double x) { return __builtin_bit_cast(uint64_t, x); }

// One full wavefront runs the operation list through the three views of one stream.
// out[(view * 2 + w) * total + i]: number i of view (0 Seq, 1 Pair, 2 Win) as lane 0 (w = 0)
// and lane 63 (w = 1) saw it; pos_out[view * 2 + w]: the view's final position.
__global__ void __launch_bounds__(64) views_kernel(PhiloxKey key, uint64_t pos0, const int64_t *ops, int nops,
                                                   int64_t total, uint64_t *out, uint64_t *pos_out) {
  const int lane = (int)(threadIdx.x & 63);
  const int w = lane == 0 ? 0 : (lane == 63 ? 1 : -1);
  SeqRng sq{key, pos0};
  PairRng pr;
  pr.init(key, pos0);
  WinRng wn;
  wn.init(key, lane, pos0);
  int64_t n = 0;
  for (int o = 0; o < nops; ++o) {
    const int64_t code = uniform_i64(ops[2 * o]), arg = uniform_i64(ops[2 * o + 1]);
    if (code == OP_SEEK) {
      stream_seek(sq, (uint64_t)arg);
      pr.pos = (uint64_t)arg;   // (PairRng: a plain cursor; the held block is checked by number)
      stream_seek(wn, (uint64_t)arg);
    } else if (code == OP_DRAW) {
      for (int64_t i = 0; i < arg; ++i, ++n) {
        const uint64_t a = f64_bits(sq()), b = f64_bits(pr()), c = f64_bits(wn());
        if (w >= 0) {
          out[(0 * 2 + w) * total + n] = a;
          out[(1 * 2 + w) * total + n] = b;
          out[(2 * 2 + w) * total + n] = c;
        }
      }
    } else {   // the out-of-line routines' hand-over: seq_view, arg numbers through it, seq_resume
      SeqRng va = seq_view(sq), vc = seq_view(wn);
      for (int64_t i = 0; i < arg; ++i, ++n) {
        const uint64_t a = f64_bits(va()), b = f64_bits(pr()), c = f64_bits(vc());
        if (w >= 0) {
          out[(0 * 2 + w) * total + n] = a;
          out[(1 * 2 + w) * total + n] = b;
          out[(2 * 2 + w) * total + n] = c;
        }
      }
      seq_resume(sq, va);
      seq_resume(wn, vc);
    }
  }
  if (w >= 0) {
    pos_out[0 * 2 + w] = stream_pos(sq);
    pos_out[1 * 2 + w] = pr.pos;
    pos_out[2 * 2 + w] = stream_pos(wn);
  }
}

// A slot of a substream through SeqRng::slot and PairRng::init_slot: n numbers each.
// out[(view * 2 + w) * n + i]; info[(view * 2 + w) * 3 + {0, 1, 2}] = final position, final
// stream id, overran().
__global__ void __launch_bounds__(64) slot_kernel(PhiloxKey key, uint64_t index, uint32_t stride, uint32_t serve,
                                                  int64_t n, uint64_t *out, uint64_t *info) {
  const int lane = (int)(threadIdx.x & 63);
  const int w = lane == 0 ? 0 : (lane == 63 ? 1 : -1);
  SeqRng sq = SeqRng::slot(key, index, stride, serve);
  PairRng pr;
  pr.init_slot(key, index, stride, serve);
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t a = f64_bits(sq()), b = f64_bits(pr());
    if (w >= 0) {
      out[(0 * 2 + w) * n + i] = a;
      out[(1 * 2 + w) * n + i] = b;
    }
  }
  if (w >= 0) {
    info[(0 * 2 + w) * 3 + 0] = sq.pos;
    info[(0 * 2 + w) * 3 + 1] = sq.key.stream;
    info[(0 * 2 + w) * 3 + 2] = sq.overran() ? 1u : 0u;
    info[(1 * 2 + w) * 3 + 0] = pr.pos;
    info[(1 * 2 + w) * 3 + 1] = pr.key.stream;
    info[(1 * 2 + w) * 3 + 2] = pr.overran() ? 1u : 0u;
  }
}

// stream_normals by a whole workgroup, or (ONE_WAVE) by the first wavefront of a workgroup of
// 128 whose second wavefront returns at once.  status[thread] = what the call returned.
template <bool ONE_WAVE, class Slots>
__global__ void normals_kernel(PhiloxKey key, uint64_t bpos0, int N, Slots slots, double *szz, uint64_t *pos_out,
                               int32_t *status) {
  __shared__ NormalsLds lds;
  if (ONE_WAVE && threadIdx.x >= 64) return;
  status[threadIdx.x] = stream_normals<ONE_WAVE>(lds, key, bpos0, N, szz, pos_out, slots);
}

// One wavefront makes the listed sub-chunks of a shared job, the job's words put into LDS as
// kalman_prepare_lead posts them.
__global__ void __launch_bounds__(64) share_kernel(SsParams P, uint32_t pos_lo, uint32_t pos_hi, int nfirst, int nper,
                                                   int dI, int dL, int dH, const int32_t *list, int nlist) {
  __shared__ KalmanLmLds lds;
  if (threadIdx.x == 0) {
    NormalsShare &J = lds.share;
    J.seq = 1; J.lo = 0; J.hi = 0; J.hfin = 0; J.bad = 0;
    J.pos_lo = pos_lo; J.pos_hi = pos_hi;
    J.N = nfirst + (P.T - 1) * nper; J.nfirst = nfirst; J.nper = nper; J.dI = dI; J.dL = dL; J.dH = dH;
  }
  __syncthreads();
  const NormalsShareCtx X = normals_share_ctx(P, 0, lds);
  for (int i = 0; i < nlist; ++i) normals_share_chunk(X, __builtin_amdgcn_readfirstlane(list[i]));
}

template <bool ONE_WAVE, class Slots>
int run_normals(const PhiloxKey &key, uint64_t bpos0, int N, const Slots &slots, int threads, double *szz, size_t nszz,
                size_t szz_off, uint64_t *pos_out, int32_t *status, size_t nstatus) {
  Dev<double> dZ(szz, nszz);
  Dev<uint64_t> dP(pos_out, 1);
  Dev<int32_t> dS(status, nstatus);
  RP_TRY(dZ.err); RP_TRY(dP.err); RP_TRY(dS.err);
  hipLaunchKernelGGL((normals_kernel<ONE_WAVE, Slots>), dim3(1), dim3(threads), 0, nullptr, key, bpos0, N, slots,
                     dZ.ptr + szz_off, dP.ptr, dS.ptr);
  RP_TRY(hipGetLastError());
  RP_TRY(hipDeviceSynchronize());
  RP_TRY(dZ.back());
  RP_TRY(dP.back());
  return (int)dS.back();
}

bool team_ok(int threads, int one_wave) {
  return one_wave ? threads == 128 : (threads == 64 || threads == 128 || threads == 256);
}

}  // namespace

extern "C" {

int rp_state_slot_stride() { return STATE_SLOT_STRIDE; }
int rp_lm_tp() { return LM_TP; }
int rp_sn_sub() { return SN_SUB; }
int rp_chain_ok() { return CHAIN_OK; }

// ops: nops {code, argument} pairs; out: nout >= 6 * (numbers drawn); pos_out: 6
int rp_views(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t stream, uint64_t pos0, const int64_t *ops, int nops,
             uint64_t *out, size_t nout, uint64_t *pos_out, size_t npos) {
  if (!ops || !out || !pos_out || nops < 1 || nops > 4096 || npos < 6) return RP_BAD_REQUEST;
  int64_t total = 0;
  for (int o = 0; o < nops; ++o) {
    const int64_t code = ops[2 * o], arg = ops[2 * o + 1];
    if (code == OP_SEEK) continue;
    if ((code != OP_DRAW && code != OP_SEQ_ROUND_TRIP) || arg < 0 || arg > (1 << 20)) return RP_BAD_REQUEST;
    total += arg;
  }
  if (total < 1 || total > (1 << 22) || (size_t)(6 * total) > nout) return RP_BAD_REQUEST;
  Dev<int64_t> dOps(ops, 2 * (size_t)nops);
  Dev<uint64_t> dO(out, nout), dP(pos_out, npos);
  RP_TRY(dOps.err); RP_TRY(dO.err); RP_TRY(dP.err);
  hipLaunchKernelGGL(views_kernel, dim3(1), dim3(64), 0, nullptr, PhiloxKey{k0, k1, chain, stream}, pos0, dOps.ptr,
                     nops, total, dO.ptr, dP.ptr);
  RP_TRY(hipGetLastError());
  RP_TRY(hipDeviceSynchronize());
  RP_TRY(dO.back());
  return (int)dP.back();
}

// out: nout >= 4 * n; info: ninfo >= 12
int rp_slot(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t stream, uint64_t index, uint32_t stride, uint32_t serve,
            int64_t n, uint64_t *out, size_t nout, uint64_t *info, size_t ninfo) {
  if (!out || !info || n < 1 || n > (1 << 20) || (size_t)(4 * n) > nout || ninfo < 12 || serve > stride)
    return RP_BAD_REQUEST;
  Dev<uint64_t> dO(out, nout), dI(info, ninfo);
  RP_TRY(dO.err); RP_TRY(dI.err);
  hipLaunchKernelGGL(slot_kernel, dim3(1), dim3(64), 0, nullptr, PhiloxKey{k0, k1, chain, stream}, index, stride,
                     serve, n, dO.ptr, dI.ptr);
  RP_TRY(hipGetLastError());
  RP_TRY(hipDeviceSynchronize());
  RP_TRY(dO.back());
  return (int)dI.back();
}

// szz[szz_off + i] = draw i of the N that start at stream position bpos0; status: one word per thread
int rp_normals_in_order(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t stream, uint64_t bpos0, int N, int threads,
                        int one_wave, double *szz, size_t nszz, size_t szz_off, uint64_t *pos_out, int32_t *status,
                        size_t nstatus) {
  if (!szz || !pos_out || !status || N < 1 || N > (1 << 24) || !team_ok(threads, one_wave) ||
      nstatus < (size_t)threads || szz_off > nszz || (size_t)N > nszz - szz_off || bpos0 % STATE_SLOT_STRIDE != 0)
    return RP_BAD_REQUEST;
  const PhiloxKey key{k0, k1, chain, stream};
  return one_wave ? run_normals<true>(key, bpos0, N, NormalsInOrder{N}, threads, szz, nszz, szz_off, pos_out, status,
                                      nstatus)
                  : run_normals<false>(key, bpos0, N, NormalsInOrder{N}, threads, szz, nszz, szz_off, pos_out, status,
                                       nstatus);
}

// the same in the lane-major layout of a series of T steps: szz[szz_off + s], s < 2 LM_TP
int rp_normals_lm(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t stream, uint64_t bpos0, int T, int dI, int dL,
                  int dH, int threads, int one_wave, double *szz, size_t nszz, size_t szz_off, uint64_t *pos_out,
                  int32_t *status, size_t nstatus) {
  if (!szz || !pos_out || !status || T < 1 || T > LM_TP || (dI | dL | dH) & ~1 || !team_ok(threads, one_wave) ||
      nstatus < (size_t)threads || szz_off > nszz || (size_t)(2 * LM_TP) > nszz - szz_off ||
      bpos0 % STATE_SLOT_STRIDE != 0)
    return RP_BAD_REQUEST;
  const PhiloxKey key{k0, k1, chain, stream};
  const int nfirst = dI + dH, nper = dL + dH, N = nfirst + (T - 1) * nper;
  const LmSlots slots{T, nfirst, nper, dI, dL, dH};
  return one_wave ? run_normals<true>(key, bpos0, N, slots, threads, szz, nszz, szz_off, pos_out, status, nstatus)
                  : run_normals<false>(key, bpos0, N, slots, threads, szz, nszz, szz_off, pos_out, status, nstatus);
}

// the listed sub-chunks of a shared job; the normals land at scratch[(5 + 2 zbuf) TP + s], s < 2 LM_TP
// (the key is the product's: stream 2 of chain `chain`)
int rp_share(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t pos_lo, uint32_t pos_hi, int T, int dI, int dL, int dH,
             int zbuf, int TP, const int32_t *list, int nlist, double *scratch, size_t nscratch) {
  const int nsub = (LM_TP + SN_SUB - 1) / SN_SUB;
  if (!list || !scratch || T < 1 || T > LM_TP || (dI | dL | dH) & ~1 || zbuf < 0 || zbuf > 1 || TP < 0 ||
      TP > LM_TP || nlist < 1 || nlist > 4096)
    return RP_BAD_REQUEST;
  const size_t first = (size_t)(5 + 2 * zbuf) * (size_t)TP;
  if (first > nscratch || (size_t)(2 * LM_TP) > nscratch - first) return RP_BAD_REQUEST;
  for (int i = 0; i < nlist; ++i)
    if (list[i] < 0 || list[i] >= nsub) return RP_BAD_REQUEST;
  Dev<double> dZ(scratch, nscratch);
  Dev<int32_t> dL_(list, (size_t)nlist);
  RP_TRY(dZ.err); RP_TRY(dL_.err);
  SsParams P{};
  P.T = T;
  P.seed_lo = k0;
  P.seed_hi = k1;
  P.chain_offset = (int64_t)chain;
  P.scratch = dZ.ptr;
  P.scratch_stride = (int64_t)nscratch;
  P.zbuf = zbuf;
  P.TP = TP;
  hipLaunchKernelGGL(share_kernel, dim3(1), dim3(64), 0, nullptr, P, pos_lo, pos_hi, dI + dH, dL + dH, dI, dL, dH,
                     dL_.ptr, nlist);
  RP_TRY(hipGetLastError());
  RP_TRY(hipDeviceSynchronize());
  return (int)dZ.back();
}

}  // extern "C"
