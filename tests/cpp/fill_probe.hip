// Test-only probe of the table fill's triangular solves, for tests/test_fill_mfma_gpu.py.
//
// The kernels here instantiate the product's own device functions -- diag_inverses,
// mf_proposal_sums (ssvs_fill_mfma.h) and solve_blocks (ssvs_device.h) -- on a model block laid
// out by ssvs_scalar_layout, and restate none of them.  One wavefront per launch.  The factor
// and its reciprocal diagonal are read by diag_inverses from the model block in GLOBAL memory
// (the product reads them from the LDS copy the factorisation has just left; the function is a
// template over the pointer types and does the same arithmetic on either); the sorted index
// list is copied into LDS, where mf_proposal_sums expects it.
//
// Every exported wrapper takes host arrays with explicit lengths (in elements), checks ON THE
// HOST that every index the kernel will form is in range (FP_BAD_REQUEST instead of a launch
// where one is not), allocates device buffers of exactly those lengths, copies everything in
// -- outputs too, which the caller has filled with a sentinel and extended by guard bands --,
// launches on the null stream, synchronises, copies every writable buffer back whole and
// returns the hipError_t.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ssvs_device.h"

using namespace boom_amd;

namespace {

enum : int { FP_BAD_REQUEST = -1, FP_LIST = MF_ROWS * MF_MAX_BLOCK_ROWS };

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

#define FP_TRY(expr)                              \
  do {                                            \
    hipError_t e__ = (expr);                      \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)

// inv(L_II) of both factors of the block, into S.iv / S.ia
__device__ __forceinline__ void both_inverses(double *block, const SsvsScalarLayout &S, int k, int lane) {
  const double *cb = block;
  diag_inverses(cb + S.Lv, cb + S.rdv, block + S.iv, k, mf_block_rows(k), lane);
  diag_inverses(cb + S.La, cb + S.rda, block + S.ia, k, mf_block_rows(k), lane);
}

__global__ void __launch_bounds__(64) inverses_kernel(double *block, int kcap, int k) {
  const SsvsScalarLayout S = ssvs_scalar_layout(kcap);
  both_inverses(block, S, k, (int)(threadIdx.x & 63));
}

// the inverses as publish_model makes them (agent-scope fence included), then the sums of the
// 64 proposals jbase + lane: out[s * 64 + lane], s = 0 nv, 1 dv, 2 na, 3 ab
template <int MAXNI>
__global__ void __launch_bounds__(64) sums_kernel(const double *V, const double *A, int p, double sv, double sa,
                                                  double *block, int kcap, const int32_t *g, int k, int jbase,
                                                  const int32_t *flags, double *out) {
  __shared__ uint16_t list[FP_LIST];
  const int lane = (int)(threadIdx.x & 63);
  // (entries behind k are whatever an earlier model left in the product: here a valid index
  // that is none of the model's rows' business)
  for (int m = lane; m < FP_LIST; m += WAVE) list[m] = (uint16_t)(m < k ? g[m] : p - 1);
  __syncthreads();
  const SsvsScalarLayout S = ssvs_scalar_layout(kcap);
  both_inverses(block, S, k, lane);
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  const MfSums z = mf_proposal_sums<MAXNI>(V, A, p, sv, sa, block, S, S.iv, S.ia,
                                           to_lds<uint16_t>((unsigned char *)list), k, jbase, flags[lane], lane);
  out[0 * WAVE + lane] = z.nv;
  out[1 * WAVE + lane] = z.dv;
  out[2 * WAVE + lane] = z.na;
  out[3 * WAVE + lane] = z.ab;
}

// solve_blocks on 64 right-hand sides, lane l's at rhs[l * NB * 8 ..]; which = 0: the factor of
// V_g, 1: that of A_g.  The block is read through the constant address space, the pointer
// passed through an opaque asm as publish_model derives ch.sc.
template <int NB>
__global__ void __launch_bounds__(64) lane_solve_kernel(const double *block, int kcap, int k, int which, double *rhs) {
  const int lane = (int)(threadIdx.x & 63);
  const SsvsScalarLayout S = ssvs_scalar_layout(kcap);
  double x[NB * 8];
#pragma unroll
  for (int i = 0; i < NB * 8; ++i) x[i] = rhs[(size_t)lane * (NB * 8) + i];
  unsigned long long u = (unsigned long long)block;
  asm volatile("" : "+s"(u) : : "memory");
  c_f64 *sc = (c_f64 *)u;
  solve_blocks<NB>(sc + (which ? S.La : S.Lv), sc + (which ? S.rda : S.rdv), k, x);
#pragma unroll
  for (int i = 0; i < NB * 8; ++i) rhs[(size_t)lane * (NB * 8) + i] = x[i];
}

// a capacity the layout is defined for, a model that fits it and the rows the fill touches
bool model_ok(int kcap, int k, size_t nblock) {
  if (kcap < 16 || kcap > FP_LIST || kcap % 8 != 0 || k < 1 || k > kcap) return false;
  return nblock >= (size_t)ssvs_scalar_layout(kcap).total;
}
bool fill_ok(int kcap, int k, size_t nblock) {
  return model_ok(kcap, k, nblock) && MF_ROWS * mf_block_rows(k) <= kcap;
}

template <int MAXNI>
int run_sums(const double *V, const double *A, int p, double sv, double sa, double *block, size_t nblock, int kcap,
             const int32_t *g, int k, int jbase, const int32_t *flags, double *out, size_t nout) {
  Dev<double> dV(V, (size_t)p * p), dA(A, (size_t)p * p), dB(block, nblock), dO(out, nout);
  Dev<int32_t> dG(g, (size_t)k), dF(flags, WAVE);
  FP_TRY(dV.err); FP_TRY(dA.err); FP_TRY(dB.err); FP_TRY(dO.err); FP_TRY(dG.err); FP_TRY(dF.err);
  hipLaunchKernelGGL(sums_kernel<MAXNI>, dim3(1), dim3(64), 0, nullptr, dV.ptr, dA.ptr, p, sv, sa, dB.ptr, kcap,
                     dG.ptr, k, jbase, dF.ptr, dO.ptr);
  FP_TRY(hipGetLastError());
  FP_TRY(hipDeviceSynchronize());
  FP_TRY(dB.back());
  return (int)dO.back();
}

template <int NB>
int run_lane_solve(const double *block, size_t nblock, int kcap, int k, int which, double *rhs, size_t nrhs) {
  Dev<double> dB(block, nblock), dR(rhs, nrhs);
  FP_TRY(dB.err); FP_TRY(dR.err);
  hipLaunchKernelGGL(lane_solve_kernel<NB>, dim3(1), dim3(64), 0, nullptr, dB.ptr, kcap, k, which, dR.ptr);
  FP_TRY(hipGetLastError());
  FP_TRY(hipDeviceSynchronize());
  return (int)dR.back();
}

}  // namespace

extern "C" {

int fp_block_total(int kcap) { return (int)ssvs_scalar_layout(kcap).total; }
// offsets (doubles) of Lv, La, rdv, rda, w, bg, iv, ia in a block of capacity kcap
void fp_layout(int kcap, int32_t *out8) {
  const SsvsScalarLayout S = ssvs_scalar_layout(kcap);
  const uint32_t o[8] = {S.Lv, S.La, S.rdv, S.rda, S.w, S.bg, S.iv, S.ia};
  for (int i = 0; i < 8; ++i) out8[i] = (int32_t)o[i];
}
int fp_block_rows(int k) { return mf_block_rows(k); }

// block: nblock >= the layout's total (what is behind it is the caller's guard band)
int fp_inverses(int kcap, int k, double *block, size_t nblock) {
  if (!block || !fill_ok(kcap, k, nblock)) return FP_BAD_REQUEST;
  Dev<double> dB(block, nblock);
  FP_TRY(dB.err);
  hipLaunchKernelGGL(inverses_kernel, dim3(1), dim3(64), 0, nullptr, dB.ptr, kcap, k);
  FP_TRY(hipGetLastError());
  FP_TRY(hipDeviceSynchronize());
  return (int)dB.back();
}

// V, A: p x p; g: k sorted indices < p; flags: 64 words (bit 0 fast, bit 1 add); out: nout >= 256
int fp_sums(int maxni, const double *V, const double *A, int p, double sv, double sa, double *block, size_t nblock,
            int kcap, const int32_t *g, int k, int jbase, const int32_t *flags, double *out, size_t nout) {
  if (!V || !A || !block || !g || !flags || !out || nout < 4 * WAVE || p < 1 || p > 65535 || jbase < 0)
    return FP_BAD_REQUEST;
  if ((maxni != 3 && maxni != 4 && maxni != 8) || !fill_ok(kcap, k, nblock) || k > MF_ROWS * maxni ||
      mf_block_rows(k) > maxni)
    return FP_BAD_REQUEST;
  for (int i = 0; i < k; ++i)
    if (g[i] < 0 || g[i] >= p || (i > 0 && g[i] <= g[i - 1])) return FP_BAD_REQUEST;
  for (int l = 0; l < WAVE; ++l)   // a fast lane's proposal is a column of V and A
    if ((flags[l] & 1) && jbase + l >= p) return FP_BAD_REQUEST;
  switch (maxni) {
    case 3: return run_sums<3>(V, A, p, sv, sa, block, nblock, kcap, g, k, jbase, flags, out, nout);
    case 4: return run_sums<4>(V, A, p, sv, sa, block, nblock, kcap, g, k, jbase, flags, out, nout);
    default: return run_sums<8>(V, A, p, sv, sa, block, nblock, kcap, g, k, jbase, flags, out, nout);
  }
}

// rhs: 64 right-hand sides of nb * 8 doubles, solved in place; kcap = nb * 8 (the capacity the
// product's instance of solve_blocks<nb> lays its block out with)
int fp_lane_solve(int nb, const double *block, size_t nblock, int kcap, int k, int which, double *rhs, size_t nrhs) {
  if (!block || !rhs || (nb != 2 && nb != 6 && nb != 8) || kcap != nb * 8 || !model_ok(kcap, k, nblock) ||
      which < 0 || which > 1 || nrhs < (size_t)WAVE * (size_t)(nb * 8))
    return FP_BAD_REQUEST;
  switch (nb) {
    case 2: return run_lane_solve<2>(block, nblock, kcap, k, which, rhs, nrhs);
    case 6: return run_lane_solve<6>(block, nblock, kcap, k, which, rhs, nrhs);
    default: return run_lane_solve<8>(block, nblock, kcap, k, which, rhs, nrhs);
  }
}

}  // extern "C"
