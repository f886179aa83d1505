// Test-only probe of the large-model kernel's pieces, for tests/test_big_kernel_probe_gpu.py.
//
// This file includes the product's ssvs_big_kernel.hip itself -- the device functions launched
// here are the product's, compiled with the product's flags (FLAGS and FLAGS_ssvs_big_kernel),
// and nothing of them is restated:
//   chol_tile, chol_tile_regs      one 64 x 64 tile, one wavefront each
//   big_solve                      64 per-lane right-hand sides against a block's factor
//   big_build_body                 as ssvs_big_logp_kernel calls it (one wavefront, part -1) and
//                                  as ssvs_big_kernel's BCMD_BUILD does (two wavefronts, part =
//                                  wave, the exchange slots in the control block of the LDS)
//   big_eval<true>                 two wavefronts on the same window of 64 proposals
// The file's launchers refer to two functions of the product library (the kernel timer's); the
// probe never calls those launchers, and the two names are resolved by stubs below, so nothing
// of the product library is linked.
//
// Every exported wrapper takes host arrays with explicit lengths (in elements), checks ON THE
// HOST that every index the kernel will form is in range (BP_BAD_REQUEST instead of a launch
// where one is not), allocates device buffers of exactly those lengths, copies everything in
// -- outputs too, which the caller has filled with a sentinel and extended by guard bands --,
// launches on the null stream, synchronises, copies every writable buffer back whole and
// returns the hipError_t.
#include "../../boom_amd/csrc/ssvs_big_kernel.hip"

#include <cstddef>
#include <cstdint>

#include "probe_dev.h"

namespace boom_amd {
// (never called: the probe launches its kernels itself)
void kt_mark(hipStream_t, int, bool) {}
bool kt_active() { return false; }
}  // namespace boom_amd

using namespace boom_amd;

namespace {

enum : int { BP_BAD_REQUEST = -1, BP_KCAP_MAX = 1024, BP_LDS_MAX = 160 * 1024 };

// ---- one tile -----------------------------------------------------------------------------------
// in: 64 x 64 row-major.  t1 (chol_tile): entries (i, c), c <= i < kk, of the LDS tile;
// t2 (chol_tile_regs): the lane's whole register row; rd1, rd2: 64 each; scal: ok1, ok2, ld1, ld2
__global__ void __launch_bounds__(64) tiles_kernel(const double *in, int kk, double *t1, double *t2, double *rd1,
                                                   double *rd2, double *scal) {
  __shared__ __attribute__((aligned(16))) double T[36 * 64];
  __shared__ __attribute__((aligned(16))) double rdt[64];
  __shared__ __attribute__((aligned(16))) double col[128];
  const int lane = (int)(threadIdx.x & 63);
  lds_f64 *Tl = to_lds<double>((unsigned char *)T);
  lds_f64 *rl = to_lds<double>((unsigned char *)rdt);
  lds_f64 *cl = to_lds<double>((unsigned char *)col);
  // (whole 8 x 8 blocks of the lower block triangle, as the model rebuild leaves them)
  for (int c = 0; c < 64; ++c)
    if ((c >> 3) <= (lane >> 3)) Tl[bidx(lane, c)] = in[lane * 64 + c];
  rl[lane] = 0.0;
  wave_sync();
  bool ok1 = false, ok2 = false;
  double ld1 = 0.0, ld2 = 0.0, rdl = 0.0;
  chol_tile(Tl, rl, kk, lane, &ok1, &ld1);
  wave_sync();
  // (the row as big_build_body hands it over: zero above the diagonal and in rows >= kk)
  double acc[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) acc[c] = (lane < kk && c <= lane) ? in[lane * 64 + c] : 0.0;
  chol_tile_regs(acc, cl, kk, lane, &ok2, &ld2, &rdl);
  wave_sync();
  for (int c = 0; c <= lane; ++c)
    if (lane < kk) t1[lane * 64 + c] = Tl[bidx(lane, c)];
#pragma unroll
  for (int c = 0; c < 64; ++c) t2[lane * 64 + c] = acc[c];
  rd1[lane] = rl[lane];
  rd2[lane] = rdl;
  if (lane == 0) {
    scal[0] = ok1 ? 1.0 : 0.0;
    scal[1] = ok2 ? 1.0 : 0.0;
    scal[2] = ld1;
    scal[3] = ld2;
  }
}

// ---- the per-lane solve -------------------------------------------------------------------------
// rhs: lane l's right-hand side at rhs[l * npan * 64 ..]; the solutions are what big_solve parks
// in xs (park_all), element (row m, lane l) at m * 64 + l
__global__ void __launch_bounds__(64) solve_kernel(const double *block, int kcap, int k, int which, const double *rhs,
                                                   double *xs) {
  const int lane = (int)(threadIdx.x & 63);
  const SsvsScalarLayout S = ssvs_scalar_layout(kcap);
  const int npan = (k + 63) >> 6;
  c_f64 *sc = scalar_view(block);
  big_solve(sc + (which ? S.La : S.Lv), sc + (which ? S.rda : S.rdv), k, npan, true, xs, lane,
            [&](int I, double (&a)[64]) {
#pragma unroll
              for (int r = 0; r < 64; ++r) a[r] = rhs[(size_t)lane * (size_t)(npan * 64) + I * 64 + r];
            },
            [&](int, double (&)[64]) {});
}

// ---- the build ----------------------------------------------------------------------------------
struct BuildArgs {
  const double *V, *A, *b, *l1, *l0, *xty;
  const uint8_t *gamma;
  int64_t max_model_size;
  int p, kcap, mode, reuse;
  double DF, ss0q, sv, sa, sx;
  double *block, *xs;
  double *scal;        // logp, lp, ldv, lda, Q, c, SS, pd, bad, k
  double *w, *rdv;     // the LDS copies, kcap each
  uint64_t sentinel;
};

__device__ __forceinline__ void bind_big(Chain &ch, BigCtx &bx, unsigned char *smem, const SsvsBigLds &lay, int kcap,
                                         int lane) {
  ch.lane = lane;
  ch.k = 0;
  ch.Lv = ch.La = nullptr;
  ch.rda = nullptr;
  ch.bg = nullptr;
  ch.rdv = to_lds<double>(smem + lay.rd);
  ch.w = to_lds<double>(smem + lay.w);
  ch.g = to_lds<uint16_t>(smem + lay.g);
  ch.gam = to_lds<uint8_t>(smem + lay.gam);
  bx.kcap = kcap;
  bx.S = ssvs_scalar_layout(kcap);
  bx.tile = to_lds<double>(smem + lay.tile);
  bx.rdt = to_lds<double>(smem + lay.rdt);
  bx.y = to_lds<double>(smem + lay.y);
  bx.bst = to_lds<double>(smem + lay.bst);
  bx.gst = to_lds<uint16_t>(smem + lay.gst);
}

template <int W>
__global__ void __launch_bounds__(64 * W) build_kernel(BuildArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = (int)(threadIdx.x & 63);
  const int wave = uni((int)(threadIdx.x >> 6));
  const int p = a.p, kcap = a.kcap;
  const SsvsBigLds lay = ssvs_big_lds_layout(p, kcap);
  Chain ch;
  BigCtx bx;
  ch.p = p;
  bind_big(ch, bx, smem, lay, kcap, lane);
  bx.xs = a.xs + (size_t)wave * (size_t)kcap * 64;
  lds_f64 *ctl = to_lds<double>(smem + lay.ctrl);
  BigP BP;
  BP.V = a.V; BP.A = a.A; BP.b = a.b; BP.l1 = a.l1; BP.l0 = a.l0;
  BP.vdiag = nullptr;
  BP.max_model_size = a.max_model_size;
  ch.xty = a.xty;
  ch.DF = a.DF;
  ch.ss0q = a.ss0q;
  ch.mode = a.mode;
  ch.sv = a.sv; ch.sa = a.sa; ch.sx = a.sx;
  if (wave == 0) {
    for (int j = lane; j < p; j += WAVE) ch.gam[j] = a.gamma[j];
    // (what the build does not write of the two LDS vectors comes back as the sentinel)
    for (int m = lane; m < kcap; m += WAVE) {
      ch.w[m] = __builtin_bit_cast(double, a.sentinel);
      ch.rdv[m] = __builtin_bit_cast(double, a.sentinel);
    }
    rebuild_g(ch, kcap);
    if (lane == 0) ctl[BX_K] = (double)ch.k;
  }
  Model M;
  M.logp = M.lp = M.ldv = M.lda = M.Q = M.c = M.SS = 0.0;
  M.pd = true;
  M.bad = 0;
  const bool reuse = a.reuse != 0;
  if (W == 1) {
    if (reuse) load_scalars(a.block, bx.S, M);
    big_build_body(BP, ch, M, a.block, bx, reuse);
  } else {
    __syncthreads();
    if (wave != 0) ch.k = (int)ctl[BX_K];
    if (reuse && wave == 0) load_scalars(a.block, bx.S, M);
    if (wave == 0 || !reuse) big_build_body(BP, ch, M, a.block, bx, wave == 0 ? reuse : false, reuse ? -1 : wave, ctl);
    __syncthreads();
  }
  if (wave != 0) return;
  store_scalars(a.block, bx.S, M, lane);
  if (lane == 0) {
    a.scal[0] = M.logp; a.scal[1] = M.lp; a.scal[2] = M.ldv; a.scal[3] = M.lda;
    a.scal[4] = M.Q; a.scal[5] = M.c; a.scal[6] = M.SS; a.scal[7] = M.pd ? 1.0 : 0.0;
    a.scal[8] = (double)M.bad;
    a.scal[9] = (double)ch.k;
  }
  wave_sync();
  for (int m = lane; m < kcap; m += WAVE) {
    a.w[m] = ch.w[m];
    a.rdv[m] = ch.rdv[m];
  }
}

// ---- the proposals ------------------------------------------------------------------------------
struct EvalArgs {
  const double *V, *A, *b, *l1, *l0, *xty;
  const uint8_t *gamma;
  const int32_t *g;
  const double *model;   // logp, lp, ldv, lda, Q, c
  int64_t max_model_size;
  int p, kcap, k, mode, jbase;
  double DF, ss0q, sv, sa, sx;
  double *block, *xs;
  double *out;           // [wave][logp, slow, bad_ss][lane]
};

__global__ void __launch_bounds__(128) eval_kernel(EvalArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = (int)(threadIdx.x & 63);
  const int wave = uni((int)(threadIdx.x >> 6));
  const int p = a.p, kcap = a.kcap;
  const SsvsBigLds lay = ssvs_big_lds_layout(p, kcap);
  Chain ch;
  BigCtx bx;
  ch.p = p;
  bind_big(ch, bx, smem, lay, kcap, lane);
  bx.xs = a.xs + (size_t)wave * (size_t)kcap * 64;
  BigP BP;
  BP.V = a.V; BP.A = a.A; BP.b = a.b; BP.l1 = a.l1; BP.l0 = a.l0;
  BP.vdiag = nullptr;
  BP.max_model_size = a.max_model_size;
  ch.xty = a.xty;
  ch.DF = a.DF;
  ch.ss0q = a.ss0q;
  ch.mode = a.mode;
  ch.sv = a.sv; ch.sa = a.sa; ch.sx = a.sx;
  if (wave == 0) {
    for (int j = lane; j < p; j += WAVE) ch.gam[j] = a.gamma[j];
    // (entries behind k are whatever an earlier model left in the product: here a valid index
    // that is none of the model's rows' business)
    for (int m = lane; m < kcap; m += WAVE) ch.g[m] = (uint16_t)(m < a.k ? a.g[m] : p - 1);
  }
  __syncthreads();
  ch.k = a.k;
  ch.sc_store = a.block;
  Model Me;
  Me.logp = a.model[0]; Me.lp = a.model[1]; Me.ldv = a.model[2];
  Me.lda = a.model[3]; Me.Q = a.model[4]; Me.c = a.model[5];
  Me.SS = 0; Me.pd = true; Me.bad = 0;
  c_f64 *sc = scalar_view(ch.sc_store);
  const int idx = a.jbase + lane;   // (both wavefronts the same window)
  const bool valid = idx < p;
  const Proposal pr = big_eval<true>(BP, ch, Me, bx, sc, valid ? idx : 0, valid, idx - lane);
  double *o = a.out + (size_t)wave * 3 * WAVE;
  o[0 * WAVE + lane] = pr.logp;
  o[1 * WAVE + lane] = pr.slow ? 1.0 : 0.0;
  o[2 * WAVE + lane] = pr.bad_ss ? 1.0 : 0.0;
}

bool kcap_ok(int kcap) { return kcap >= 128 && kcap <= BP_KCAP_MAX && kcap % 64 == 0; }

template <class K, class Args>
int launch_lds(K kernel, int threads, size_t lds, const Args &args) {
  IP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(1), dim3(threads), lds, nullptr, args);
  IP_TRY(hipGetLastError());
  return (int)hipDeviceSynchronize();
}

}  // namespace

extern "C" {

int bp_block_total(int kcap) { return (int)ssvs_scalar_layout(kcap).total; }
// offsets (doubles) of Lv, La, rdv, rda, w, bg, g, scal, iv, ia in a block of capacity kcap
void bp_layout(int kcap, int32_t *out10) {
  const SsvsScalarLayout S = ssvs_scalar_layout(kcap);
  const uint32_t o[10] = {S.Lv, S.La, S.rdv, S.rda, S.w, S.bg, S.g, S.scal, S.iv, S.ia};
  for (int i = 0; i < 10; ++i) out10[i] = (int32_t)o[i];
}
// byte offsets of the large-model kernel's LDS: tile, rdt, w, y, rd, bst, ctrl, g, gst, perm0, perm1, oth,
// last, pred, gam, gam0, nbr, total
void bp_lds_layout(int p, int kcap, int32_t *out18) {
  const SsvsBigLds L = ssvs_big_lds_layout(p, kcap);
  const uint32_t o[18] = {L.tile, L.rdt, L.w, L.y, L.rd, L.bst, L.ctrl, L.g, L.gst, L.perm0, L.perm1, L.oth,
                          L.last, L.pred, L.gam, L.gam0, L.nbr, L.total};
  for (int i = 0; i < 18; ++i) out18[i] = (int32_t)o[i];
}

// tile_in, t1, t2: >= 4096; rd1, rd2: >= 64; scal: >= 4
int bp_chol_tiles(int kk, const double *tile_in, size_t nin, double *t1, double *t2, size_t nt, double *rd1, double *rd2,
                  size_t nrd, double *scal, size_t nscal) {
  if (!tile_in || !t1 || !t2 || !rd1 || !rd2 || !scal || kk < 1 || kk > 64 || nin < 4096 || nt < 4096 || nrd < 64 ||
      nscal < 4)
    return BP_BAD_REQUEST;
  Dev<double> dI(tile_in, nin), d1(t1, nt), d2(t2, nt), dr1(rd1, nrd), dr2(rd2, nrd), dS(scal, nscal);
  IP_TRY(dI.err); IP_TRY(d1.err); IP_TRY(d2.err); IP_TRY(dr1.err); IP_TRY(dr2.err); IP_TRY(dS.err);
  hipLaunchKernelGGL(tiles_kernel, dim3(1), dim3(64), 0, nullptr, dI.ptr, kk, d1.ptr, d2.ptr, dr1.ptr, dr2.ptr, dS.ptr);
  IP_TRY(hipGetLastError());
  IP_TRY(hipDeviceSynchronize());
  IP_TRY(d1.back()); IP_TRY(d2.back()); IP_TRY(dr1.back()); IP_TRY(dr2.back());
  return (int)dS.back();
}

// block: >= the layout's total; rhs: >= 64 * npan * 64; xs: >= kcap * 64 (the product's parking space of one wave)
int bp_solve(int kcap, int k, int which, const double *block, size_t nblock, const double *rhs, size_t nrhs, double *xs,
             size_t nxs) {
  if (!block || !rhs || !xs || !kcap_ok(kcap) || k < 1 || k > kcap || which < 0 || which > 1) return BP_BAD_REQUEST;
  const size_t npan = (size_t)((k + 63) >> 6);
  if (nblock < (size_t)ssvs_scalar_layout(kcap).total || nrhs < 64 * npan * 64 || nxs < (size_t)kcap * 64)
    return BP_BAD_REQUEST;
  Dev<double> dB(block, nblock), dR(rhs, nrhs), dX(xs, nxs);
  IP_TRY(dB.err); IP_TRY(dR.err); IP_TRY(dX.err);
  hipLaunchKernelGGL(solve_kernel, dim3(1), dim3(64), 0, nullptr, dB.ptr, kcap, k, which, dR.ptr, dX.ptr);
  IP_TRY(hipGetLastError());
  IP_TRY(hipDeviceSynchronize());
  return (int)dX.back();
}

// V, A: p x p; b, l1, l0, xty, gamma: p; block: >= the layout's total; xs: >= waves * kcap * 64;
// scal: >= 10; w, rdv: >= kcap
int bp_build(int waves, int reuse, const double *V, const double *A, size_t nmat, const double *b, const double *l1,
             const double *l0, const double *xty, const uint8_t *gamma, size_t nvec, int64_t max_model_size, int p,
             int kcap, int mode, double DF, double ss0q, double sv, double sa, double sx, double *block, size_t nblock,
             double *xs, size_t nxs, double *scal, size_t nscal, double *w, double *rdv, size_t nk, uint64_t sentinel) {
  if (!V || !A || !b || !l1 || !l0 || !xty || !gamma || !block || !xs || !scal || !w || !rdv) return BP_BAD_REQUEST;
  if ((waves != 1 && waves != 2) || p < 1 || p > 65535 || !kcap_ok(kcap) || mode < 0 || mode > 2) return BP_BAD_REQUEST;
  if (nmat < (size_t)p * p || nvec < (size_t)p || nblock < (size_t)ssvs_scalar_layout(kcap).total ||
      nxs < (size_t)waves * kcap * 64 || nscal < 10 || nk < (size_t)kcap)
    return BP_BAD_REQUEST;
  int k = 0;
  for (int j = 0; j < p; ++j) k += gamma[j] != 0;
  const size_t lds = ssvs_big_lds_layout(p, kcap).total;
  if (k > kcap || lds > BP_LDS_MAX) return BP_BAD_REQUEST;
  Dev<double> dV(V, nmat), dA(A, nmat), db(b, nvec), d1(l1, nvec), d0(l0, nvec), dx(xty, nvec), dB(block, nblock),
      dX(xs, nxs), dS(scal, nscal), dW(w, nk), dR(rdv, nk);
  Dev<uint8_t> dG(gamma, nvec);
  IP_TRY(dV.err); IP_TRY(dA.err); IP_TRY(db.err); IP_TRY(d1.err); IP_TRY(d0.err); IP_TRY(dx.err); IP_TRY(dB.err);
  IP_TRY(dX.err); IP_TRY(dS.err); IP_TRY(dW.err); IP_TRY(dR.err); IP_TRY(dG.err);
  BuildArgs a{dV.ptr, dA.ptr, db.ptr, d1.ptr, d0.ptr, dx.ptr, dG.ptr, max_model_size, p, kcap, mode, reuse,
              DF, ss0q, sv, sa, sx, dB.ptr, dX.ptr, dS.ptr, dW.ptr, dR.ptr, sentinel};
  const int e = waves == 1 ? launch_lds(build_kernel<1>, 64, lds, a) : launch_lds(build_kernel<2>, 128, lds, a);
  if (e) return e;
  IP_TRY(dB.back()); IP_TRY(dX.back()); IP_TRY(dS.back()); IP_TRY(dW.back());
  return (int)dR.back();
}

// as bp_build; g: k sorted indices, the set bytes of gamma; model: >= 6; xs: >= 2 * kcap * 64; out: >= 384
int bp_eval(const double *V, const double *A, size_t nmat, const double *b, const double *l1, const double *l0,
            const double *xty, const uint8_t *gamma, size_t nvec, int64_t max_model_size, int p, int kcap, int mode,
            double DF, double ss0q, double sv, double sa, double sx, const int32_t *g, int k, const double *model,
            size_t nmodel, int jbase, double *block, size_t nblock, double *xs, size_t nxs, double *out, size_t nout) {
  if (!V || !A || !b || !l1 || !l0 || !xty || !gamma || !g || !model || !block || !xs || !out) return BP_BAD_REQUEST;
  if (p < 1 || p > 65535 || !kcap_ok(kcap) || mode < 0 || mode > 2 || k < 1 || k > kcap || jbase < 0 || jbase > p ||
      jbase % 64 != 0)
    return BP_BAD_REQUEST;
  if (nmat < (size_t)p * p || nvec < (size_t)p || nblock < (size_t)ssvs_scalar_layout(kcap).total ||
      nxs < (size_t)2 * kcap * 64 || nmodel < 6 || nout < 6 * WAVE)
    return BP_BAD_REQUEST;
  int count = 0;
  for (int j = 0; j < p; ++j) count += gamma[j] != 0;
  if (count != k) return BP_BAD_REQUEST;
  for (int i = 0; i < k; ++i)
    if (g[i] < 0 || g[i] >= p || !gamma[g[i]] || (i > 0 && g[i] <= g[i - 1])) return BP_BAD_REQUEST;
  const size_t lds = ssvs_big_lds_layout(p, kcap).total;
  if (lds > BP_LDS_MAX) return BP_BAD_REQUEST;
  Dev<double> dV(V, nmat), dA(A, nmat), db(b, nvec), d1(l1, nvec), d0(l0, nvec), dx(xty, nvec), dM(model, nmodel),
      dB(block, nblock), dX(xs, nxs), dO(out, nout);
  Dev<uint8_t> dG(gamma, nvec);
  Dev<int32_t> dL(g, (size_t)k);
  IP_TRY(dV.err); IP_TRY(dA.err); IP_TRY(db.err); IP_TRY(d1.err); IP_TRY(d0.err); IP_TRY(dx.err); IP_TRY(dM.err);
  IP_TRY(dB.err); IP_TRY(dX.err); IP_TRY(dO.err); IP_TRY(dG.err); IP_TRY(dL.err);
  EvalArgs a{dV.ptr, dA.ptr, db.ptr, d1.ptr, d0.ptr, dx.ptr, dG.ptr, dL.ptr, dM.ptr, max_model_size,
             p, kcap, k, mode, jbase, DF, ss0q, sv, sa, sx, dB.ptr, dX.ptr, dO.ptr};
  const int e = launch_lds(eval_kernel, 128, lds, a);
  if (e) return e;
  IP_TRY(dB.back()); IP_TRY(dX.back());
  return (int)dO.back();
}

}  // extern "C"
