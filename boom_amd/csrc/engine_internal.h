// What the host side's translation units share: the engine itself, the launchers of the
// kernel files, the entry points' prologues and the host helpers that cross files.
//   engine.hip      creation, timing, regression data, priors, state, the BregVs / SpikeSlab /
//                   adaptive sweeps, pipelined launches, ba_draw_next's look-ahead, summaries,
//                   traces, prediction, check_chain_status
//   engine_glm.hip  probit, logit, Poisson, Student-t, quantile, multinomial logit (the
//                   latent-data families)
//   engine_ss.hip            state space, the core: launch parameters, ss_prepare, data and local level,
//                            the rounds of a call and the round kernel's launches, the plain accessors
//   engine_ss_models.hip     the list of state models (its arithmetic: ssg_spec.h, host only), the
//                            calendars, the Student trend's and the spike-and-slab autoregression's entry points
//   engine_ss_lookahead.hip  ba_ss_draw_next's look-ahead: record, snapshots, settle
//   engine_ss_observe.hip    forecasts and one-step prediction errors
//   engine_ss_family.hip     bsts family = "student", "poisson", "logit"
// The launchers' declarations: of the products in products.h, of the rest below.  The
// imputation kernels' parameters are latent_params.h (the common head) and one header per
// family; their shared device code is latent_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/boom_amd.h"
#include "kalman_params.h"
#include "ktimer.h"
#include "mlogit_params.h"
#include "probit_params.h"
#include "products.h"
#include "quantile_params.h"
#include "ss_filter_params.h"
#include "ssg_regholiday.h"
#include "ssg_spec.h"
#include "ssvs_params.h"
#include "student_params.h"

namespace boom_amd {
// ssvs_kernel.hip
hipError_t launch_ssvs_sweep(hipStream_t stream, const SsvsParams &P, int nsweeps);
// ssvs_big_kernel.hip
hipError_t launch_ssvs_big(hipStream_t stream, const SsvsParams &P, int nsweeps);
// ssvs_adaptive_kernel.hip
hipError_t launch_ssvs_adaptive(hipStream_t stream, const SsvsParams &P, int nsweeps);
hipError_t launch_ssvs_logp(hipStream_t stream, const SsvsParams &P,
                            const uint8_t *gammas, int ngamma, double *out,
                            int *status_out);
hipError_t launch_lds_exchange_order(hipStream_t stream, int *bad_device);
hipError_t launch_ssvs_reduce_summaries(hipStream_t stream, const SsvsParams &P,
                                        double *out);
// suf_kernel.hip
int suf_row_slices(int64_t n, int p);
int launch_suf_from_xy(hipStream_t stream, int64_t n, int p, const double *X,
                       const double *y, double *xtx, double *xty,
                       double *scalars /* yty, sumy */, double *xsum,
                       double *planes /* suf_row_slices(n, p) * p * p doubles, or null */);
// kalman_kernel.hip
hipError_t launch_ssm_simsmooth(hipStream_t stream, const SsParams &P, int draw_variances);
hipError_t launch_ssm_forecast(hipStream_t stream, const SsParams &P, const RhParams &R, int horizon, const double *newX,
                               uint64_t *pos_forecast, double *out);
// slt_kernel.hip: the Student local linear trend's sampler (before a state draw) and its observe_state (after it)
hipError_t launch_slt_params(hipStream_t stream, const SsParams &P, const SltParams &U);
hipError_t launch_slt_weights(hipStream_t stream, const SsParams &P, const SltParams &U);
// ar_spike_kernel.hip: the ArSpikeSlabSampler of every spike-and-slab autoregression block (before a state draw)
hipError_t launch_ar_spike(hipStream_t stream, const SsParams &P, const ArSpikeParams &U);
// reg_holiday_kernel.hip: the regression holiday models' sampler and the chains' series (before a state draw;
// draw = 0: the series alone), their observe_state (after it), and y_c = y for every chain
hipError_t launch_rh_draw(hipStream_t stream, const SsParams &P, const RhParams &R, int draw, int hier = 0);
hipError_t launch_rhh_draw(hipStream_t stream, const SsParams &P, const RhParams &R, const RhhParams &Q);
hipError_t launch_rh_observe(hipStream_t stream, const SsParams &P, const RhParams &R);
hipError_t launch_rh_fill(hipStream_t stream, const RhParams &R, int T, int chains);
// ss_family_forecast_kernel.hip: family = SS_FORECAST_*; scale = the horizon's exposures / rounded trial
// counts (Poisson, logit), nu = every chain's degrees of freedom (Student-t); the other is not read
hipError_t launch_ss_family_forecast(hipStream_t stream, const SsParams &P, int family, int horizon,
                                     const double *newX, const double *scale, const double *nu,
                                     uint64_t *pos_forecast, double *out);
hipError_t launch_probit_impute(hipStream_t stream, const ProbitParams &P, double *planes);
hipError_t launch_student_impute(hipStream_t stream, const StudentParams &P, const double *Xsq,
                                 const double *slab_precision, double *xtz, double *v_diag, double *planes);
hipError_t launch_student_sigma_nu(hipStream_t stream, const StudentParams &P);
hipError_t launch_student_ss_weights(hipStream_t stream, const StudentParams &P, int draw);
hipError_t launch_student_ss_suf(hipStream_t stream, const StudentParams &P, const double *Xsq,
                                 const double *slab_precision, double *xtz, double *v_diag, double *planes);
// probit_kernel.hip: the state space Poisson (family 0) and logit (family 1) families
hipError_t launch_latent_ss_h(hipStream_t stream, const ProbitParams &P, int family, int draw);
hipError_t launch_latent_ss_suf(hipStream_t stream, const ProbitParams &P, int family, const double *Xsq,
                                const double *slab_precision, double *v_diag, double *planes);
// quantile_kernel.hip
hipError_t launch_quantile_impute(hipStream_t stream, const QuantileParams &P, const double *Xsq,
                                  const double *slab_precision, double *xtz, double *v_diag, double *planes);
// mlogit_kernel.hip
hipError_t launch_mlogit_expand(hipStream_t stream, int64_t n, int M, int psub, int pch, const double *Xs,
                                const double *Xc, double *X, double *Xsq);
hipError_t launch_mlogit_impute(hipStream_t stream, const MlogitParams &P, const double *Xsq,
                                const double *slab_precision, double *xtz, double *v_diag, double *planes);
hipError_t launch_logit_impute(hipStream_t stream, const ProbitParams &P, const double *Xsq,
                               const double *slab_precision, double *v_diag, double *planes,
                               int polya_gamma);
// xtwx_cols_kernel.hip (the products: products.h)
hipError_t launch_ssvs_big_logp(hipStream_t stream, const SsvsParams &P, int kcap, const uint8_t *gammas,
                                const int *which, int nwhich, double *model_ws, double *xs_ws, double *out,
                                int *status_out);
hipError_t launch_kalman_simsmooth(hipStream_t stream, const SsParams &P,
                                   int draw_level);
hipError_t launch_kalman_main(hipStream_t stream, const SsParams &P, int draw_level);
hipError_t launch_kalman_xte(hipStream_t stream, const SsParams &P, bool planes_only);
hipError_t launch_kalman_prepare(hipStream_t stream, const SsParams &P, int draw_level);
hipError_t launch_ss_round(hipStream_t stream, const SsvsParams &P, const SsParams &S, const SsRoundParams &F,
                           int *max_resident);
size_t ss_round_lds(int p, int kcap);
hipError_t launch_ss_forecast(hipStream_t stream, const SsParams &P, int horizon, const double *newX,
                              uint64_t *pos_forecast, double *out);

// sets the text ba_last_error() returns (one thread_local string for the whole library,
// engine.hip) and returns `code`
int fail(int code, const std::string &msg);

#define HIP_TRY(expr)                                                       \
  do {                                                                      \
    hipError_t err__ = (expr);                                              \
    if (err__ != hipSuccess) {                                              \
      return fail(BA_E_HIP, std::string(#expr) + ": " +                     \
                                hipGetErrorString(err__));                  \
    }                                                                       \
  } while (0)

template <class T>
struct DevBuf {
  T *ptr = nullptr;
  size_t count = 0;
  ~DevBuf() { release(); }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    count = 0;
  }
  hipError_t resize(size_t n) {
    if (n == count && ptr) return hipSuccess;
    release();
    if (n == 0) return hipSuccess;
    hipError_t e = hipMalloc((void **)&ptr, n * sizeof(T));
    if (e == hipSuccess) count = n;
    return e;
  }
};

// Which data the engine holds: one kind at a time.  A data setter installs its kind as its
// last step; DATA_REGRESSION is also the state of a fresh engine (have_suf says whether
// anything was uploaded).  Every sweep entry point serves one kind and refuses the others
// (sweep_refusal, engine.hip).
enum DataKind { DATA_REGRESSION, DATA_STATE_SPACE, DATA_PROBIT, DATA_LOGIT, DATA_POISSON, DATA_STUDENT, DATA_QUANTILE,
                DATA_MLOGIT,
                // bsts family = "student": the state space data with the Student-t observation model
                // (StateSpaceStudentRegressionModel); the Student path's buffers with n = T
                DATA_SS_STUDENT,
                // bsts family = "poisson": the state space data with the Poisson observation model
                // (StateSpacePoissonModel); the Poisson path's buffers with n = T
                DATA_SS_POISSON,
                // bsts family = "logit": the state space data with the binomial logit observation model
                // (StateSpaceLogitModel); the logit path's buffers with n = T
                DATA_SS_LOGIT };
// the two state space families whose latent data are a value and a precision per step
inline bool latent_ss_kind(DataKind k) { return k == DATA_SS_POISSON || k == DATA_SS_LOGIT; }
// the state space data under one of the three observation families with latent data ...
inline bool ss_family_kind(DataKind k) { return k == DATA_SS_STUDENT || k == DATA_SS_POISSON || k == DATA_SS_LOGIT; }
// ... as the rule book of the state models names them (ssg_refusal)
inline SsFamily ss_family(DataKind k) {
  return k == DATA_SS_STUDENT ? SS_FAMILY_STUDENT : k == DATA_SS_POISSON ? SS_FAMILY_POISSON : k == DATA_SS_LOGIT ? SS_FAMILY_LOGIT : SS_FAMILY_GAUSSIAN;
}
// the kinds that hold a series and a state (the Gaussian, the Student-t, the Poisson and the logit observation model)
inline bool ss_kind(DataKind k) { return k == DATA_STATE_SPACE || ss_family_kind(k); }
// the latent-data families: the regression runs on every chain's own imputed responses
inline bool latent_data(DataKind k) { return k == DATA_PROBIT || k == DATA_LOGIT || k == DATA_POISSON || k == DATA_STUDENT || k == DATA_QUANTILE || k == DATA_MLOGIT || ss_family_kind(k); }
// ... and those of them whose V = slab precision + X'WX is every chain's own, built a vector
// at a time (serve_columns, engine_glm.hip)
inline bool column_service(DataKind k) { return k == DATA_LOGIT || k == DATA_POISSON || k == DATA_STUDENT || k == DATA_QUANTILE || k == DATA_MLOGIT || ss_family_kind(k); }
// the two families whose sigma^2 is every chain's own draw on latent data
inline bool student_kind(DataKind k) { return k == DATA_STUDENT || k == DATA_SS_STUDENT; }

}  // namespace boom_amd

using namespace boom_amd;   // (this header is the three host files' own)

// ba_set_kernel_timing: the event pairs of the launches since the last read
struct KtSpan { int cls; hipEvent_t a, b; };
struct KTimer {
  std::vector<KtSpan> spans;
  std::vector<hipEvent_t> open;   // begin events by class (launches do not nest within a class)
  std::vector<hipEvent_t> pool;
  double ms[KT_CLASSES] = {};
  int64_t launches[KT_CLASSES] = {};
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  // fold the finished spans into the totals (the caller has synchronised the stream)
  void collect() {
    for (const KtSpan &sp : spans) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, sp.a, sp.b) == hipSuccess) { ms[sp.cls] += t; ++launches[sp.cls]; }
      pool.push_back(sp.a);
      pool.push_back(sp.b);
    }
    spans.clear();
  }
  ~KTimer() {
    for (const KtSpan &sp : spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    for (hipEvent_t e : open) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
  }
};

struct ba_engine {
  ba_config cfg{};
  bool kt_enabled = false;
  bool kt_overlap = false;   // (timing on, consecutive sweep launches still overlap: ba_set_kernel_timing(e, 2))
  KTimer kt;
  hipStream_t stream = nullptr;
  int p = 0;
  int cu_count = 256;
  size_t lds_per_cu = 160 * 1024;

  DataKind data_kind = DATA_REGRESSION;   // which data are installed (one kind at a time)
  // ---- host copies (RegSuf + priors)
  bool have_suf = false, have_slab = false, have_spike = false,
       have_sigma = false;
  std::vector<double> xtx, xty, xsum;
  double yty = 0, n = 0, sumy = 0;
  std::vector<double> b, ominv, pi;
  int64_t max_model_size = -1;
  double prior_df = 0, prior_ss = 0, sigma_guess = 0;
  double sigma_max = std::numeric_limits<double>::infinity();
  int max_flips = -1;  // < 0: p
  double swap_threshold = 0.8;
  int draw_beta = 1, draw_sigma = 1;
  bool device_dirty = true;   // V/A/b/logpi/cm need (re)upload
  bool state_ready = false;

  // ---- device: shared
  DevBuf<double> dV, dA, db, dl1, dl0, dpi, dxty, dscal /* yty, n */;
  DevBuf<int32_t> dcm_start, dcm_idx;
  DevBuf<double> dcm_cor;
  bool cm_enabled = false;
  // ---- device: per chain
  DevBuf<uint8_t> dgamma;
  DevBuf<double> dbeta, dsigsq;
  DevBuf<uint16_t> dperm;
  DevBuf<uint64_t> dpos;
  DevBuf<int32_t> dstatus, dfail, dtodo, dmaxk, dtrace_idx;
  DevBuf<uint32_t> dinc;
  DevBuf<double> dbsum, dbsumsq, dacc, dsummary;
  DevBuf<double> dtr_sig, dtr_logp, dtr_k;
  DevBuf<uint16_t> drec_idx;  // recorded draws (ba_enable_draws)
  DevBuf<double> drec_beta;
  DevBuf<double> dmodel;  // per-chain model scratch (scalar-cache reads)
  DevBuf<double> dtab_lp;   // per-chain proposal table
  DevBuf<uint8_t> dtab_kind;
  DevBuf<int32_t> dtab_tag, dmodel_tag;
  DevBuf<int32_t> dran;  // catch-up launches of the state-space path: sweeps done per chain
  bool table_ok = false;  // nothing but ba_sweep launches since the tables were built
  bool model_ok = false;  // nothing that changes a model's factors since the last sweep launch
  int trace_stride = 0;
  // scratch for suf build
  DevBuf<double> dX, dy, dxtx, dxsum, dsufscal;

  int kcap = 0;
  int waves = 1;  // wavefronts per chain
  // ba_draw_next: the look-ahead batch.  `avail` draws are recorded on the
  // device, `served` of them have been handed out; the snapshot is the chains'
  // state (and the running summaries) at the start of the batch, which is what
  // a rewind restores before replaying the `served` draws already seen.
  struct La {
    int len = 1, avail = 0, served = 0;
    // host copies of the batch's record for the chains the caller reads (the
    // per-iteration loop reads chain 0 after every draw: one set of copies per
    // batch instead of per call); synced: the batch's launch has been waited for
    // and its chain statuses checked
    struct Rows { std::vector<double> k, sig, beta; std::vector<uint16_t> idx; };
    std::unordered_map<int64_t, Rows> cache;
    bool synced = false;
    // Overlapping look-ahead batches: the record holds two batches (halves slot and
    // slot ^ 1 of 2 len rows), the batch after the one being served is launched as soon
    // as serving starts (ahead) and the launches hand chains over (pipelined sweeps); each
    // batch's workgroups save their chain's state on entry (snapshot set = half) for rewinds.
    bool pipe = true;        // allowed (off for good after a batch had to be redone the old way)
    bool cur_piped = false;  // the batch being served was launched that way
    bool ahead = false;
    int slot = 0;
    hipEvent_t done[2] = {nullptr, nullptr};
    // two sets of every per-chain array a sweep changes; which live array, how many elements
    // per chain and which SsvsParams member each goes with: la_snap_fields (engine.hip)
    struct Snap {
      DevBuf<uint8_t> gamma;
      DevBuf<double> beta, sigsq, bsum, bsumsq, acc;
      DevBuf<uint16_t> perm;
      DevBuf<uint64_t> pos;
      DevBuf<int32_t> fail;
      DevBuf<uint32_t> inc;
    } snap;
  } la;
  int rec_cap = 64;  // variables per recorded draw (ba_enable_draws)
  // HBM-resident path for models of more than 64 variables (ssvs_big_kernel.hip):
  // active once a chain has outgrown the LDS kernel, capacity grows on demand
  bool big_active = false;
  int big_kcap = 0;
  DevBuf<double> dbig_model, dbig_xs;
  // ba_set_tuning overrides (0 / -1: the engine chooses)
  int tune_waves = 0, tune_walk_policy = -1, tune_kcap_start = 0;
  int tune_rebuild_policy = 0;   // SsvsParams::rebuild_policy (ba_set_rebuild_policy)
  // SpikeSlabSampler (sigma^2 given) mode
  int cur_mode = 0;          // mode of the launches in flight (0 BregVs, 1 SSS)
  int sss_slab_scales = 1;   // slab precision = Omega^{-1} / sigma^2
  int sss_max_flips = -1;    // limits only when > 0 (SpikeSlabSampler.cpp:77)
  double v_scale = 1.0;      // V = Omega^{-1} + v_scale * XtX currently on the device
  double v_scale_want = 1.0;
  DevBuf<uint64_t> dpos_sss;
  uint64_t seed = 0;
  // AdaptiveSpikeSlabRegressionSampler (mode 2): rates, iteration counts, options
  DevBuf<double> dada_birth, dada_death, dada_ws;
  DevBuf<uint64_t> dada_iter, dpos_ada;
  int ada_max_flips = 100;
  double ada_step = .001, ada_target = .345;

  // ---- state space (bsts local level + regression)
  bool ss_level_set = false, ss_initialized = false;
  int T = 0;
  DevBuf<double> dss_y, dss_X, dss_scratch;
  // The callers' loop is "one round, then read chain 0": what the accessors copy goes
  // through ONE pinned staging buffer per call (a batch of asynchronous copies, one
  // synchronisation) instead of one blocking copy per field, and a ba_sync() that follows
  // a clean ba_sync() with no call in between that could have enqueued or changed anything
  // is free (api_seq counts such calls, clean_seq remembers the last clean check).
  void *pinned = nullptr;
  size_t pinned_bytes = 0;
  uint64_t api_seq = 1, clean_seq = 0;
  int api_depth = 0;   // calls other than accessors in progress (they may enqueue after an inner ba_sync)
  // lane-major copies for kalman_lm_kernel (kalman_params.h): local level, T <= LM_TP
  DevBuf<double> dss_yt, dss_Xt;
  DevBuf<uint32_t> dss_obs_mask;
  DevBuf<uint8_t> dss_obs;
  DevBuf<double> dxty_c, dyty_c, dnobs_c;       // per-chain regression suf
  DevBuf<double> dlev_sigsq, dlev_n, dlev_sumsq;
  DevBuf<uint64_t> dpos_level, dpos_state, dpos_forecast;
  // kalman_prepare_kernel (level variance + normals of the next state draw) runs on a
  // second stream beside the X'e GEMM and the SSVS launch
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_state = nullptr, ev_prep[2] = {nullptr, nullptr};
  int ss_zbuf = 0;   // the normals buffer the next state draw reads
  // pipelined sweeps: consecutive ba_sweep launches alternate between `stream` and
  // pipe.stream and hand chains over through a ring of four queues (ssvs_kernel.hip)
  struct Pipe {
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {}, join_ev = nullptr;
    DevBuf<int32_t> q, err;
    bool on = false;         // the last thing enqueued was a pipelined sweep launch
    bool unchecked = false;  // a pipelined launch has gone out since the error word was last read
    int k = 0;               // launches in the current pipeline
    bool groups = false;     // ... which are the chain GROUPS of an engine of more chains than the machine holds
  } pipe;
  DevBuf<int32_t> dprep_n;
  DevBuf<uint64_t> dprep_pos_state, dprep_pos_level;
  DevBuf<double> dprep_level;
  DevBuf<double> dxte_planes;   // split-K planes of the X'e GEMM
  double level_prior_df = 0, level_prior_ss = 0;
  double level_sigma_max = std::numeric_limits<double>::infinity();
  double ss_a0 = 0, ss_P0 = 1, ss_initial_level_sigsq = 1;
  // ---- the latent-data families (latent_data(data_kind), engine_glm.hip; DATA_SS_STUDENT
  // borrows the same buffers with n = T).  What every family holds:
  struct LatentData {
    int64_t n = 0;          // rows of X (MLVS: subjects x choices; the state space Student family: T)
    int clt = 5;            // the binomial imputers' central-limit threshold
    uint64_t draws = 0;     // imputations done so far (positions the imputers' substreams)
    DevBuf<double> X, y;    // the design (n x p column-major) and the response (MLVS keeps its own, dml_y)
    DevBuf<double> aux;     // trial counts (probit, logit) or exposures (Poisson)
    DevBuf<double> z, w;    // chains x n: every chain's latent responses and weights (probit: z alone)
    DevBuf<double> Xsq;     // X squared element-wise, for the diagonal of X'WX (the column service's families)
  } lat;
  // The column service (column_service(data_kind), xtwx_cols_kernel.hip): every chain's own
  // V = slab precision + X'WX, built a vector at a time as the sweep asks for it.
  struct ColumnService {
    DevBuf<double> V, vdiag;     // chains x p x p, and the diagonals (chains x p)
    DevBuf<double> planes;       // the split-K planes of the column and rows products (the probit sampler's X'z too)
    DevBuf<uint32_t> valid;      // which vectors hold this sweep's values: bits, `words` words per chain
    DevBuf<int32_t> req, count;  // the request list (chain, variable) and its length
    DevBuf<int32_t> wanted;      // the variable a parked chain waits for
    int words = 0;
    int64_t batch = 0;           // requests per GEMM launch (bounds the planes)
  } cols;
  int slot_limit = 0;              // (ba_set_slot_limit)
  // BinomialLogitSpikeSlabSampler
  int logit_imputer = 0;           // 0: the reference's auxiliary mixture, 1: Polya-Gamma
  // PoissonRegressionSpikeSlabSampler: its own imputation kernel and SpikeSlabSampler's shuffle;
  // the reference table's mixtures by count
  bool poisson_mix_set = false;
  std::vector<int64_t> poisson_y;             // host copy of the counts (to map them to mixtures)
  DevBuf<int32_t> dpois_off, dpois_obs;
  DevBuf<double> dpois_mu, dpois_sigma, dpois_logw;
  int poisson_mix_one = -1;
  // TRegressionSpikeSlabSampler (student_kernel.hip): its own imputation, sigma^2 per chain and
  // the nu draw; per chain nu, the slice sampler's suggested_dx, the smallest slice margin, the
  // recorded nu path; the u_i = (r_i / sigma)^2 of the last draw (chains x n)
  bool student_allow_selection = true;   // (ba_student_allow_model_selection)
  int student_nu_kind = STUDENT_NU_UNIFORM;
  double student_nu_a = 0.1, student_nu_b = 100.0;
  DevBuf<double> dstu_nu, dstu_dx, dstu_margin, dstu_u, dstu_nu_rec;
  // StateSpaceStudentPosteriorSampler (DATA_SS_STUDENT): the filter's H_t = sigma^2 / w_t
  // (chains x T); rounds done (positions the sigma^2 / nu substream; lat.draws counts the
  // weight imputations); the weights and statistics in hand are those of a state draw
  DevBuf<double> dsst_h;
  uint64_t sst_round = 0;
  bool sst_ready = false;
  // StateSpacePoissonPosteriorSampler and StateSpaceLogitPosteriorSampler (DATA_SS_POISSON,
  // DATA_SS_LOGIT; the names are the first family's): every chain's latent values v_t (the
  // series the filter reads; lat.w holds their precisions q_t) and H_t = 1 / q_t, chains x T
  // each; which steps are observed (host copy); the latent data and statistics in hand are those
  // of a state draw (lat.draws counts the imputations)
  DevBuf<double> dssp_value, dssp_h;
  std::vector<uint8_t> ssp_observed;
  std::vector<double> ssp_trials;   // (DATA_SS_LOGIT: n_t, the new model's q_t = 4 / n_t; 1 at a missing step)
  bool ssp_ready = false;
  // QuantileRegressionSpikeSlabSampler (quantile_kernel.hip): the model's quantile
  double quantile_q = 0.5;
  // MLVS (mlogit_kernel.hip): the expanded design (lat.n = N = n M rows, p = D columns), its
  // own imputation and the sweep's mode 3
  int64_t mlogit_n = 0;
  int32_t mlogit_choices = 0, mlogit_psub = 0, mlogit_pch = 0;
  bool mlogit_select = true;       // (ba_mlogit_allow_model_selection)
  DevBuf<int32_t> dml_y;
  DevBuf<uint16_t> dml_order;      // the sweep's visiting order, D entries
  DevBuf<double> dml_u, dml_wss_part, dml_wss;
  // structural state (a list of state models, ssm_kernel.hip) instead of the local level
  bool ssm_set = false;
  SsgSpec ssg{};                   // the host's copy of the specification
  DevBuf<uint8_t> dssg_spec;       // ... and the device's
  double ssg_initial_sigsq[SSG_MAX_VAR] = {};
  double ssg_initial_phi[SSG_MAX_AR][AR_MAX] = {};
  // the template of ba_ss_set_structural (level / slope / seasonal -> variance index, -1: none)
  int ssg_template_var[3] = {-1, -1, -1};
  int ssg_template_ar = -1;        // ... and the block ba_ss_add_ar appended
  int ssg_kernel_choice = 1;       // (ba_ss_set_tuning: 0 general, 1 the default choice, 3 shape-specialised)
  // the local-level rounds of a call as one persistent launch (ss_round_kernel.hip); the
  // tile words of its X'e step, zeroed before every launch; how many chains' workgroups the
  // device holds at once, by launch capacity (0: not asked yet, < 0: the kernel does not fit)
  bool ss_round_enabled = true;    // (ba_ss_set_tuning 4 / 5: the separate launches of rounds 1-4 / this)
  DevBuf<int32_t> dround_ctl, dround_members, dround_reg;
  int ss_round_resident[4] = {0, 0, 0, 0};
  bool round_debug = false;        // (ba_ss_set_tuning 6 / 7: the round kernel's notes of a debugging session on / off)
  DevBuf<int32_t> dround_debug;    // ... on this engine's device
  DevBuf<double> dssm_sigsq, dssm_n, dssm_ss, dssm_work;   // chains x SSG_MAX_VAR (sigsq, n, ss)
  DevBuf<double> dar_phi, dar_suf;                         // chains x SSG_MAX_AR x (AR_MAX | AR_SUF_STRIDE)
  DevBuf<uint64_t> dpos_var;                               // chains x SSG_MAX_VAR
  // ArStateModel + ArSpikeSlabSampler (SsgBlock::ar_spike; ar_spike_kernel.hip): the priors by
  // autoregression slot, their device copy, and every chain's inclusion indicators (chains x
  // SSG_MAX_AR x AR_MAX bytes, held as 64-bit words so that a snapshot takes them as it takes the rest)
  ArSpikePrior ar_spike_prior[SSG_MAX_AR] = {};
  DevBuf<uint8_t> dar_spike_prior;
  DevBuf<uint64_t> dar_gamma;
  // StudentLocalLinearTrendStateModel (ssg.student_block; slt_kernel.hip): the nu priors (kind, a, b)
  // and initial values of level and slope; per chain the weights and the kept residuals (2 x T each),
  // nu (2), the weights' GammaSuf (6), the sampler's stream position and the state draws observed
  int slt_nu_kind[2] = {STUDENT_NU_UNIFORM, STUDENT_NU_UNIFORM};
  double slt_nu_a[2] = {1.0, 1.0}, slt_nu_b[2] = {500.0, 500.0}, slt_initial_nu[2] = {10.0, 10.0};
  DevBuf<double> dslt_w, dslt_res, dslt_nu, dslt_wsuf;
  DevBuf<uint64_t> dslt_pos, dslt_count;
  // RandomWalkHolidayStateModel (SsgBlock::holiday): every such block's calendar as the caller gave it
  // (entry t: -1 or the position at time t; empty: not set yet), and the list's packed table on the
  // device (SsParams::cal; hol_cal_count entries -- the shortest calendar's --, 0: to be packed again)
  std::vector<int32_t> hol_calendar[SSG_MAX_BLOCKS];
  DevBuf<uint64_t> dhol_cal;
  int64_t hol_cal_count = 0;
  // the calendar seasonals (ssg_is_calendar): every such block's flags as the caller gave them
  // (entry t: 1 where time t starts a new season; empty: not set yet) -- packed into dhol_cal beside the
  // holidays' positions, with their prefix counts behind the table (SsParams::cal)
  std::vector<uint8_t> season_calendar[SSG_MAX_BLOCKS];
  // DynamicRegressionStateModel (SsgBlock::dynreg): every such block's predictors as the caller gave
  // them (rows x dim, row-major; a block of an AR dynamic regression: its one column), and the list's table on the device (SsParams::dyn; dyn_rows rows -- the
  // shortest block's --, 0: to be packed again)
  std::vector<double> dyn_predictors[SSG_MAX_BLOCKS];
  // DynamicRegressionArStateModel (SSG_DYNAMIC_REGRESSION_AR): which blocks form one model -- block b of such
  // a model: the model's first block and its coefficients (0: block b is of no such model).  Each of its
  // blocks keeps its own column in dyn_predictors (rows x 1).
  int32_t dynar_first[SSG_MAX_BLOCKS] = {}, dynar_xdim[SSG_MAX_BLOCKS] = {};
  DevBuf<double> ddyn;
  int64_t dyn_rows = 0;
  // RegressionHolidayStateModel (ssg_regholiday.h; reg_holiday_kernel.hip): the list's models -- no blocks
  // of ssg: they belong to the list and are dropped with it --, what follows from their calendars and the
  // observed flags on the device (rh_count entries of the table, 0: to be packed again), and per chain the
  // coefficients, the totals of the last state draw (RH_MAX_COEF each), the sampler's stream position and
  // the series less the models' effects (T)
  std::vector<RhModel> rh_models;
  std::vector<uint8_t> ss_observed;   // the data's observed flags, host side (the counts)
  DevBuf<int32_t> drh_table, drh_steps;
  DevBuf<double> drh_counts, drh_coef, drh_totals, drh_y;
  DevBuf<uint64_t> drh_pos;
  // the hierarchical ones among them: the hyperparameters (RH_MAX_MODELS x RHH_HYPER_STRIDE), and per
  // chain and model the hyper-mean and hyper-precision, per chain the position in RHH_STREAM
  DevBuf<double> drhh_hyper, drhh_mu, drhh_omega;
  DevBuf<uint64_t> drhh_pos;
  int64_t rh_count = 0;
  int32_t rh_nsteps = 0;
  int32_t rh_first[RH_MAX_MODELS + 1] = {};
  std::vector<double> rh_counts;      // the counts per flat coefficient, host side (ba_ss_get_regression_holiday)
  // ba_ss_prediction_errors (ss_filter_kernel.hip): its outputs on the device (errors, forecast
  // variances, log likelihoods, the forecast-variance flag), the local-level path's one-block
  // list, and the stream the filter of a look-ahead's recorded draw runs on beside the batch
  // that is running ahead
  DevBuf<double> dssf_err, dssf_var, dssf_ll;
  DevBuf<int32_t> dssf_flag;
  DevBuf<uint8_t> dssf_spec;
  hipStream_t ssf_stream = nullptr;
  // ba_ss_holdout_prediction_errors: the caller's holdout rows on the device (the outputs are the arrays above)
  DevBuf<double> dssf_newx, dssf_newy;
  // ---- look-ahead on the bsts path (ba_ss_set_lookahead / ba_ss_draw_next): a batch of
  // `len` sweep rounds per enqueue, every round's draw recorded on the device -- gamma,
  // beta, sigma^2, the state models' variances and coefficients for EVERY chain, the
  // state path for the registered chains -- and handed out one per call.  Two halves:
  // the batch after the one being served is enqueued as soon as serving starts.  Any
  // entry point that is not served from the record first puts the chains where the
  // caller has seen them (ss_la_settle: the snapshot of the batch's start, replayed up
  // to the draw being served), so the look-ahead is unobservable.
  struct SsLa {
    int len = 0;                // rounds per batch at most (<= 1: off)
    // rounds per batch NOW.  A caller whose loop reads something the record does not hold
    // (another chain's state path, sufficient statistics, a forecast) or changes something
    // (priors under the sampler) after every draw pays a rewind + replay of the batch each
    // time: so a settle halves the batch, a batch served to its end doubles it again (up to
    // len); at one round per call the look-ahead is off and is tried again after
    // `probe_wait` calm draws (16, doubling while the tries keep failing).
    int cur = 0, calm = 0, probe_wait = 16;
    bool clean = true;          // nothing has settled the batch being served
    int ahead_len = 0;          // rounds of the batch that is running ahead
    int avail = 0, served = 0, slot = 0;
    bool ahead = false;         // the next batch is enqueued (half slot ^ 1)
    bool synced = false;        // the batch being served is complete and its chains sound
    bool busy = false;          // (a settle in progress: entry points it calls do not settle again)
    hipEvent_t done[2] = {nullptr, nullptr};
    std::vector<int32_t> reg{0};            // chains whose state path is recorded (always the size of dreg / rstate's rows)
    std::vector<int32_t> want;              // ... and the ones asked for since: ss_la_alloc takes them into reg, as far as the record has room
    DevBuf<int32_t> dreg;
    DevBuf<double> lev_used;                // the level variance every chain's last state draw used
    size_t nvar = 0, nphi = 0, state_doubles = 0;   // per chain and round
    DevBuf<uint8_t> rgamma;                 // [slot][chain][round][p]
    DevBuf<double> rbeta, rsig, rvar, rphi; // [slot][chain][round][...]
    DevBuf<double> rstate;                  // [slot][registered chain][round][state_doubles]
    DevBuf<double> snap;                    // the state-space half of the chain state, two sets
    DevBuf<uint64_t> snap_pos;
    size_t snap_doubles = 0, snap_words = 0;
    struct Rows { std::vector<uint8_t> gamma; std::vector<double> beta, sig, var, phi, state; bool has_state = false; };
    std::unordered_map<int64_t, Rows> cache;
  } ssla;
};

// ---- host helpers that cross files ---------------------------------------------------
namespace boom_amd {
// the timer of the engine whose entry point this thread is in (engine.hip)
extern thread_local KTimer *g_kt;

// engine.hip
int set_device(const ba_engine *e);
int upload_shared(ba_engine *e);
int alloc_chain_state(ba_engine *e);
void fill_params(ba_engine *e, SsvsParams &P);
hipError_t launch_sweeps(ba_engine *e, const SsvsParams &P, int nsweeps);
int cap_limit(const ba_engine &e);
int choose_waves(const ba_engine &e, int kcap);
int grow_big(ba_engine *e, int *stuck);
int check_chain_status(ba_engine *e);
int switch_mode(ba_engine *e, int mode, double v_scale);
hipError_t pinned_reserve(ba_engine *e, size_t bytes);
int concurrent_stream(ba_engine *e, hipStream_t *out);
int pipe_join(ba_engine *e);
int la_rewind(ba_engine *e);
int la_copy(ba_engine *e, bool save, int set = 0);
// what both look-aheads do with launches that ran ahead of the caller: read every chain's
// status word (*ok: all CHAIN_OK), and forget what dropped launches left behind
int all_chains_ok(ba_engine *e, bool *ok);
int drop_launched_ahead(ba_engine *e);
// BA_OK when the engine holds the data the entry point samples (`wants`; sss: ba_sss_sweep,
// the other sweep of plain regression data), else the entry point's refusal for the kind held
int sweep_refusal(const ba_engine *e, DataKind wants, bool sss = false);
const char *set_data_first(DataKind wants);   // "call ba_<family>_set_data first"
// one double per chain, chain == -1: all of them (the caller has validated `chain`); both
// wait for the stream first
int write_per_chain(ba_engine *e, double *dev, int64_t chain, double value);
int read_per_chain(ba_engine *e, const double *dev, int64_t chain, double *out);
// One chain's row of a chains x n buffer to the host, for the getters of weights and latent
// data: validates `chain`, lets `ready` refuse or prepare (BA_OK to go on), waits for the
// stream and copies.
template <class Ready>
int read_chain_row(ba_engine *e, int64_t chain, const DevBuf<double> &buf, size_t n, double *out, Ready ready) {
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = ready();
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, buf.ptr + (size_t)chain * n, n * 8, hipMemcpyDeviceToHost));
  return BA_OK;
}
// engine_glm.hip
int serve_columns(ba_engine *e, std::vector<int32_t> &st, bool *served);
int student_prepare(ba_engine *e);
void fill_student_params(ba_engine *e, StudentParams &T);
void fill_probit_params(ba_engine *e, ProbitParams &Q);
int set_unit_sigsq(ba_engine *e);
int build_columns(ba_engine *e, int64_t R);
int column_buffers(ba_engine *e);
int upload_latent_data(ba_engine *e, int64_t n, int32_t p, const double *X, const double *y,
                       const double *third, bool squared, int clt_threshold);
// The rows of chain `chain` of a chains x n buffer from the host, or of every chain when chain == -1
// (the caller has validated `chain` and waited for the stream).
inline int write_chain_rows(ba_engine *e, double *buf, int64_t chain, size_t n, const double *src) {
  const size_t C = (size_t)e->cfg.chains;
  for (size_t c = chain < 0 ? 0 : (size_t)chain; c < (chain < 0 ? C : (size_t)chain + 1); ++c)
    HIP_TRY(hipMemcpy(buf + c * n, src, n * 8, hipMemcpyHostToDevice));
  return BA_OK;
}
// the local-level path of a series of at most LM_TP steps runs lane-major
// (kalman_lm_kernel): its scratch arrays have pitch LM_TP
inline bool ss_lane_major(const ba_engine &e) { return !e.ssm_set && e.T <= LM_TP; }
inline size_t ss_pitch(const ba_engine &e) { return ss_lane_major(e) ? (size_t)LM_TP : (size_t)e.T; }
// the rule book of the state models on this engine's list (ssg_refusal, ssg_spec.h): BA_OK, or the refusal
inline int ss_refused(const ba_engine *e, DataKind kind, SsgUse use) {
  const char *text = ssg_refusal(e->ssm_set ? &e->ssg : nullptr, ss_family(kind), use, 0, e->ssm_set ? (int)e->rh_models.size() : 0);
  return text ? fail(BA_E_STATE, text) : BA_OK;
}
// engine_ss.hip
int64_t ssm_work_stride(const ba_engine &e);
void fill_ss_params(ba_engine *e, SsParams &S);
bool fill_ar_spike_params(ba_engine *e, ArSpikeParams &U);
void fill_slt_params(ba_engine *e, SltParams &U);
bool fill_rh_params(ba_engine *e, RhParams &R);
bool fill_rhh_params(ba_engine *e, RhhParams &Q);   // (false: no hierarchical model)
int ss_prepare(ba_engine *e, DataKind kind = DATA_STATE_SPACE);
int ss_sweep_impl(ba_engine *e, int32_t nsweeps, int rec_slot);
int ss_escalate(ba_engine *e, std::vector<int32_t> &st);
// engine_ss_models.hip
int hol_prepare(ba_engine *e, int64_t extra = 0);
// engine_ss_lookahead.hip
int ss_la_settle(ba_engine *e);
bool ss_la_serving(const ba_engine *e);
int ss_la_wait(ba_engine *e);
int ss_la_rows(ba_engine *e, int64_t c, bool want_state, const ba_engine::SsLa::Rows **out);
hipError_t ss_la_record(ba_engine *e, int slot, int round);
bool ss_la_registered(const ba_engine *e, int64_t c);
void ss_la_want_state(ba_engine *e, int64_t c);
}  // namespace boom_amd

struct ApiScope {
  ba_engine *e;
  explicit ApiScope(ba_engine *en) : e(en) { e->api_seq++; e->api_depth++; }
  ~ApiScope() { e->api_depth--; }
  ApiScope(const ApiScope &) = delete;
};

// (a mutator changes what the next launch reads -- priors, data, options -- through copies
// on the main stream: a pipelined sweep launch still running on the other stream must be
// behind the main stream first, or it would see half of the new values)
#define MUTATE(e)                        \
  do {                                   \
    (e)->api_seq++;                      \
    int rc_m__ = set_device(e);          \
    if (!rc_m__) rc_m__ = pipe_join(e);  \
    if (!rc_m__) rc_m__ = ss_la_settle(e); \
    if (!rc_m__) rc_m__ = la_rewind(e);  \
    if (rc_m__) return rc_m__;           \
    (e)->table_ok = false;               \
    (e)->model_ok = false;               \
  } while (0)

// (accessors that enqueue nothing and change nothing: they do not count as a call
// between two ba_sync()s)
#define ENGINE_ACCESSOR_NOJOIN(e)                              \
  if (!(e)) return fail(BA_E_INVALID, "null engine");          \
  g_kt = (e)->kt_enabled ? &(e)->kt : nullptr;                 \
  {                                                            \
    int rc__ = set_device(e);                                  \
    if (rc__) return rc__;                                     \
  }
#define ENGINE_PROLOGUE_NOJOIN(e)                              \
  ENGINE_ACCESSOR_NOJOIN(e)                                    \
  ApiScope api_scope__(e);
// (everything but ba_sweep itself first lets the main stream catch up with a pipeline
// of sweep launches)
#define ENGINE_PROLOGUE(e)                                     \
  ENGINE_PROLOGUE_NOJOIN(e)                                    \
  {                                                            \
    int rc__ = pipe_join(e);                                   \
    if (!rc__) rc__ = ss_la_settle(e);                         \
    if (rc__) return rc__;                                     \
  }
#define ENGINE_ACCESSOR(e)                                     \
  ENGINE_ACCESSOR_NOJOIN(e)                                    \
  {                                                            \
    int rc__ = pipe_join(e);                                   \
    if (!rc__) rc__ = ss_la_settle(e);                         \
    if (rc__) return rc__;                                     \
  }
// (the entry points that serve the draw of ba_ss_draw_next from the device's record)
#define ENGINE_ACCESSOR_SERVED(e)                              \
  ENGINE_ACCESSOR_NOJOIN(e)                                    \
  {                                                            \
    int rc__ = pipe_join(e);                                   \
    if (rc__) return rc__;                                     \
  }
