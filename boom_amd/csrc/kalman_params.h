// Launch parameters of the Kalman filter / simulation smoother kernel
// (kalman_kernel.hip), shared with the host side (engine_ss.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssvs_params.h"

namespace boom_amd {

// Structural state (ssm_kernel.hip): BOOM's block-diagonal state -- any list of state
// models in the order they were added (StateSpaceModelBase::add_state): local level,
// local linear trend, seasonal (nseasons, season duration), autoregression, static intercept
// (StaticInterceptStateModel: on the device a local level whose variance is 0 and has no
// sampler -- nvar = 0, one variance SLOT that stays 0), trig (TrigStateModel: a 2 x 2 rotation
// per frequency, one variance for all 2 nfreq components).  State
// dimension m <= SSG_MAX_STATE (one lane per component), at most SSG_MAX_BLOCKS blocks,
// SSG_MAX_VAR variance parameters (two for a local linear trend, one otherwise; an
// autoregression block's error variance is one of them), SSG_MAX_AR autoregression
// blocks of at most AR_MAX lags.
enum { SSG_MAX_STATE = 64, SSG_MAX_BLOCKS = 8, SSG_MAX_VAR = 16, SSG_MAX_AR = 4, AR_MAX = 16 };
enum { SSG_LOCAL_LEVEL = 1, SSG_LOCAL_LINEAR_TREND = 2, SSG_SEASONAL = 3, SSG_AR = 4,
       SSG_STATIC_INTERCEPT = 5 /* (the C-ABI's number; stored as SSG_LOCAL_LEVEL with nvar = 0) */, SSG_TRIG = 6,
       // SemilocalLinearTrendStateModel: (level, slope, the slope's long-run mean mu); T = [[1, 1, 0],
       // [0, phi, 1 - phi], [0, 0, 1]]; its (phi, mu) and the slope's Ar1Suf take one of the chain's
       // autoregression slots (ar_phi[0 .. 1]; ar_suf[0 .. 5] = sumsq, sum, cross, n, first, last)
       SSG_SEMILOCAL = 7,
       // StudentLocalLinearTrendStateModel (the C-ABI's number): a local linear trend whose two state
       // errors have the per-step variances sigma^2 / w_t.  Stored as SSG_LOCAL_LINEAR_TREND --
       // SsgSpec::student_block says which block it is -- and served by the QT instances of the
       // general kernel and the two kernels of slt_kernel.hip
       SSG_STUDENT_TREND = 8,
       // ArStateModel with an ArSpikeSlabSampler (bsts AddAutoAr; the C-ABI's number): stored as SSG_AR
       // with SsgBlock::ar_spike set -- an autoregression whose excluded coefficients are 0; its sampler
       // is ar_spike_kernel.hip's, the state kernel passes it by
       SSG_AUTO_AR = 9,
       // RandomWalkHolidayStateModel (the C-ABI's number): `width` components, T = I; the step into time
       // t adds N(0, sigma^2) to component k(t) and Z_t = e_k(t) where the block's calendar says t is
       // active at position k(t), nothing otherwise.  Stored as SSG_LOCAL_LEVEL of dimension width with
       // SsgBlock::holiday set; the calendars of a list are one packed table (SsParams::cal), and such a
       // list is served by the HD instances of the general kernel
       SSG_HOLIDAY = 10,
       // The calendar seasonal (the C-ABI's number; MonthlyAnnualCycle is the one of 12 seasons whose
       // seasons start on the first day of a month): SSG_SEASONAL in everything but this -- whether time
       // t starts a new season is read from the block's calendar, not computed from a duration.  Stored
       // as SSG_SEASONAL with duration 1 and phase SSG_PHASE_CALENDAR (ssg_is_calendar; no field of its own);
       // its flags share the packed table of the holidays (bit SSG_CAL_SEASON of byte b), their prefix
       // counts sit behind the table (see SsParams::cal), and such a list is served by the HD instances
       SSG_CALENDAR_SEASONAL = 11 };
// DynamicRegressionStateModel with the independent random-walk sampler (bsts AddDynamicRegression): no
// kind of ba_ss_add_state_model -- it comes through ba_ss_add_dynamic_regression with its predictors --
// but ssg_abi_kind names such a block by this number.  d coefficients, T = I, RQR = diag(sigma_i^2),
// Z_t = x_t: a row of data.  Stored as SSG_LOCAL_LEVEL of dimension d with SsgBlock::dynreg set, d
// variance slots and d state-error rows; the predictors of a list are one table for all chains
// (SsParams::dyn), and such a list is served by the DR instances of the general kernel.
enum { SSG_DYNAMIC_REGRESSION = 12 };
// DynamicRegressionArStateModel with DynamicRegressionArPosteriorSampler (bsts AddDynamicRegression with
// DynamicRegressionArOptions(lags)): every coefficient an autoregression of `lags` lags.  It comes through
// ba_ss_add_dynamic_regression_ar; ssg_abi_kind names each of its blocks by this number.  Stored as xdim
// consecutive blocks of kind SSG_AR and dimension lags with SsgBlock::dynreg set: block i's first component is
// coefficient i (Z_t = x_{t,i} there, 0 on its lags), T = the autoregression's, RQR = sigma_i^2 at the first
// component; each block has an autoregression slot, a variance slot and an error row as kind 4 has.  Which
// blocks form one model is the engine's knowledge.  Served by the DR instances.
enum { SSG_DYNAMIC_REGRESSION_AR = 14 };
// the packed calendar: entry t holds block b's position at time t in byte b, SSG_CAL_OFF where the
// block is inactive at t (or is no holiday block).  A calendar seasonal's byte: SSG_CAL_SEASON where
// time t starts a new season (its other bits are not read).
enum : uint64_t { SSG_CAL_NONE = 0x8080808080808080ull };
enum { SSG_CAL_OFF = 0x80, SSG_CAL_SEASON = 0x01 };
// a calendar seasonal's SsgBlock::phase: no time u has u % 1 == -1, so the closed forms never fire for it
enum { SSG_PHASE_CALENDAR = -1 };
// ar_spike_kernel's own chain status: a coefficient or variance draw that is not finite
enum { AR_SPIKE_BAD_DRAW = 14 };
// the Student trend's streams: its sampler's four draws (read in sequence) and the weights' slots
enum : uint32_t { SLT_PARAM_STREAM = 160u, SLT_WEIGHT_STREAM = 161u };
enum { SLT_WEIGHT_STRIDE = 256, SLT_BLOCK = 256 };
// RegressionHolidayStateModel (bsts AddRegressionHoliday; ba_ss_add_regression_holiday): no block of the
// list -- its state is the constant 1 with variance 0 -- but an offset on the observation series: a list
// carries up to RH_MAX_MODELS such models of RH_MAX_COEF coefficients together (reg_holiday_kernel.hip).
// ssg_refusal names the model by this number.  Its coefficient sampler reads a stream of its own.
enum { SSG_REGRESSION_HOLIDAY = 13, RH_MAX_MODELS = 4, RH_MAX_COEF = 256 };
enum : uint32_t { RH_COEF_STREAM = 162u };
// rh_draw_kernel's own chain status: a coefficient draw that is not finite
enum { RH_BAD_DRAW = 15 };
// HierarchicalRegressionHolidayStateModel (bsts AddHierarchicalRegressionHoliday;
// ba_ss_add_hierarchical_regression_holiday): a regression holiday model whose holidays share one window
// width d <= RHH_MAX_WIDTH and whose coefficient vectors share the prior N(mu, Omega^-1), mu and Omega drawn
// too (hier_holiday_kernel.hip).  One of the list's RH_MAX_MODELS models; all of a chain's hierarchical
// models read one position of the sampler id RHH_STREAM.  RHH_BAD_DRAW: a factor that is not positive
// definite or a number that is not finite in rhh_draw_kernel.
enum { RHH_MAX_WIDTH = 16 };
enum : uint32_t { RHH_STREAM = 163u };
enum { RHH_BAD_DRAW = 16 };
// a model's hyperparameters on the device, d x d matrices row-major at leading dimension RHH_MAX_WIDTH:
// Sigma0^-1 | S0 = nu0 x variance_guess | Sigma0^-1 mu0
enum { RHH_HYPER_SINV0 = 0, RHH_HYPER_S0 = RHH_MAX_WIDTH * RHH_MAX_WIDTH, RHH_HYPER_SINV0MU0 = 2 * RHH_MAX_WIDTH * RHH_MAX_WIDTH,
       RHH_HYPER_STRIDE = RHH_HYPER_SINV0MU0 + RHH_MAX_WIDTH };
// the observation families of ss_family_forecast_kernel.hip (launch_ss_family_forecast)
enum { SS_FORECAST_STUDENT = 0, SS_FORECAST_POISSON = 1, SS_FORECAST_LOGIT = 2 };
// a chain's ArModel sufficient statistics (per autoregression block): xtx (lags x lags at
// leading dimension AR_MAX) | xty | yty | n
enum { AR_SUF_XTY = AR_MAX * AR_MAX, AR_SUF_YTY = AR_SUF_XTY + AR_MAX, AR_SUF_N = AR_SUF_YTY + 1,
       AR_SUF_STRIDE = AR_SUF_N + 1 };
struct SsgBlock {
  int32_t kind, first, dim, nvar;
  int32_t var0;        // index of the block's first variance parameter
  int32_t nseasons, duration, phase;   // seasonal: a new season starts at the times u with u % duration == phase
                                       // (phase SSG_PHASE_CALENDAR, duration 1: a calendar seasonal -- ssg_is_calendar)
  int32_t lags, ar_index;              // autoregression: which of the chain's coefficient / suf slots
  int32_t sid[2];      // Philox sampler ids of the variance samplers (autoregression: its ArPosteriorSampler's)
  int32_t nfreq;       // trig: frequencies (dim = 2 nfreq)
  int32_t err0;        // index of the block's first state-error row (a trig block has dim of them, a trend two, the others one)
  int32_t sl_truncate, sl_positive;   // semilocal: NonzeroMeanAr1Sampler::force_stationary / force_ar1_positive
  int32_t ar_spike;    // autoregression: its sampler is the ArSpikeSlabSampler of ar_spike_kernel.hip (0: ArPosteriorSampler, in the state kernel)
  int32_t holiday;     // local level of dimension dim: a random-walk holiday (SSG_HOLIDAY), its positions in the packed calendar
  // local level of dimension dim: a dynamic regression (SSG_DYNAMIC_REGRESSION): 1 + the column of the
  // list's predictor table its first coefficient reads (0: no such block).  Variance slot i of the
  // block reads Philox sampler id sid[0] + 16 i (sid[1] is not used).
  // An autoregression (kind SSG_AR) with the field set: one coefficient of an AR dynamic regression
  // (SSG_DYNAMIC_REGRESSION_AR) -- 1 + the column its first component reads; its sampler id is sid[0] as kind 4's.
  int32_t dynreg;
};
// is the block a calendar seasonal (SSG_CALENDAR_SEASONAL: its season starts are read from the packed calendar)?
__host__ __device__ inline bool ssg_is_calendar(const SsgBlock &k) { return k.kind == SSG_SEASONAL && k.phase == SSG_PHASE_CALENDAR; }
// A block as one 32-bit word, for the kernels that keep block b's word in lane b of a register and
// fetch it with v_readlane: kind (3 bits) | first (7) | dim (7) | index of its first variance
// parameter (5) | autoregression slot (3).  Bits 25 and up belong to the kernel that holds the word
// (Blocks of ssg_device.h, SsfBlocks of ss_filter_kernel.hip: each says what it keeps there).
struct SsgBlockWord {
  static __host__ __device__ __forceinline__ int kind_of(unsigned d) { return (int)(d & 7u); }
  static __host__ __device__ __forceinline__ int first_of(unsigned d) { return (int)((d >> 3) & 127u); }
  static __host__ __device__ __forceinline__ int dim_of(unsigned d) { return (int)((d >> 10) & 127u); }
  static __host__ __device__ __forceinline__ int var0_of(unsigned d) { return (int)((d >> 17) & 31u); }
  static __host__ __device__ __forceinline__ int arx_of(unsigned d) { return (int)((d >> 22) & 7u); }
  static __host__ __device__ __forceinline__ unsigned pack(const SsgBlock &K) {
    const unsigned lo = (unsigned)K.kind | ((unsigned)K.first << 3) | ((unsigned)K.dim << 10) | ((unsigned)K.var0 << 17);
    const int arx = K.ar_index;   // (-1: the block has no autoregression slot)
    return lo | ((unsigned)(arx < 0 ? 0 : arx) << 22);
  }
};
// the specification, in device memory (read through the scalar cache)
struct SsgSpec {
  int32_t m, nblocks, nvar, nar;
  int32_t ld;          // leading dimension of the state variance in LDS (odd)
  int32_t bl;          // steps per block of the passes (64 for m <= 16, ... 16 for m <= 64)
  int32_t nerr;        // rows of the state that carry state error (one per variance slot; a trig block: every component)
  int32_t student_block;   // 1 + the index of the Student local linear trend block (0: the list has none)
  SsgBlock blk[SSG_MAX_BLOCKS];
  double prior_df[SSG_MAX_VAR], prior_ss[SSG_MAX_VAR], sigma_max[SSG_MAX_VAR];
  double a0[SSG_MAX_STATE], P0[SSG_MAX_STATE];   // initial state mean, variance (diagonal)
  // trig: the rotation [[c, s], [-s, c]] of the pair a component belongs to (by state component)
  double trig_c[SSG_MAX_STATE], trig_s[SSG_MAX_STATE];
  // semilocal (by autoregression slot): the slope's mean prior N(mu, sigma), its AR(1) coefficient's prior N(mu, sigma)
  double sl_prior[SSG_MAX_AR][4];
};
struct SsmParams {
  const SsgSpec *spec;                  // device copy
  int32_t m, nblocks, nvar, nar, ld, bl, nerr;   // (the launch's copies of the scalars)
  int32_t ndyn;                         // the columns of the dynamic regressions' predictor table (0: the list has none)
  // the block list is [local level | local linear trend] [+ seasonal of duration 1] [+ one
  // autoregression] with m <= 16: the shape-specialised kernel runs (ssm_template_kernel.hip);
  // tpl_trend = 0: the general kernel
  int32_t tpl_trend, tpl_nseasons, tpl_ar_lags;
  int32_t glob;                         // the list holds a trig or a semilocal-linear-trend block: the kernel instance that carries their code
  double *var_sigsq, *var_n, *var_ss;   // chains x SSG_MAX_VAR
  uint64_t *pos_var;                    // chains x SSG_MAX_VAR: the variance samplers' stream positions
  double *ar_phi;                       // chains x SSG_MAX_AR x AR_MAX
  double *ar_suf;                       // chains x SSG_MAX_AR x AR_SUF_STRIDE
  // per chain: gains K (m x T) | state (m x T) | smoothed disturbances (nerr x T) | normals
  double *work;
  int64_t work_stride;
};

struct SsParams {
  int32_t T, p, chains;
  int32_t slot_limit;     // > 0: uniforms a slot of the state stream serves before its spill stream (default: the stride)
  int32_t chain_first, chain_count;  // this launch: chains [chain_first, chain_first + chain_count)
  int64_t chain_offset;
  // shared data: StateSpaceRegressionModel(y, X, observed)
  const double *y;          // T
  const double *X;          // T x p column-major
  const uint8_t *observed;  // T
  // Lane-major copies for kalman_lm_kernel (local level, T <= LM_TP): step t of a series
  // sits at lm_at(t) = (t % 16) * 128 + t / 16 -- thread i of the chain's 128 owns steps
  // 16 i .. 16 i + 15 and its j-th step is element 128 j + i, so every per-step array
  // is read and written with plain coalesced accesses, no transposes.  Xt: p columns of
  // LM_TP (zero where unobserved -- never: as X -- and past T), yt: LM_TP, obs_mask[i]:
  // bit j = step 16 i + j observed.  lane_major = 1: the chains' scratch arrays
  // (residuals, state draw, normals) have pitch TP = LM_TP and that layout too.
  const double *Xt;
  const double *yt;
  const uint32_t *obs_mask;
  int32_t TP, lane_major;
  // regression parameters of every chain (written by the SSVS kernel)
  const uint8_t *gamma;     // chains x p
  const double *beta;       // chains x p
  const double *sigsq;      // chains
  // local level state model + its sampler
  double *level_sigsq;      // chains
  double *level_n;          // chains  (ZeroMeanGaussianModel suf)
  double *level_sumsq;      // chains
  double level_prior_df, level_prior_ss, level_sigma_max;
  double a0, P0;            // initial state mean / variance
  // RNG: stream 1 = level sampler, stream 2 = state imputation
  uint32_t seed_lo, seed_hi;
  uint64_t *pos_level, *pos_state;
  int32_t *status;
  const int32_t *only_ran;  // catch-up launches: skip chains whose entry is 0 (nullptr: all)
  // per-chain work arrays in HBM: v, F, K, v_sim, state, r, r_sim (T each)
  double *scratch;
  int64_t scratch_stride;   // SS_SCRATCH_ARRAYS x TP
  // per-chain regression sufficient statistics rebuilt by impute_state
  double *xty;              // chains x p
  double *yty;              // chains
  double *nobs;             // chains
  double *xte_planes;       // workspace of the X'e GEMM: xte_planes(T) x chains x p doubles
  // The part of a state draw that depends on nothing the same round's regression sweep
  // produces -- the level-variance draw and the sweep's standard normals -- is done ahead
  // by kalman_prepare_kernel on a second stream (see there).  zbuf = which of the chain's
  // two normals buffers this launch reads (main) or writes (prepare); prepared = 1: the
  // main kernel finds prep_n[zbuf][chain] normals there and level_sigsq drawn (0: not
  // prepared -- it does both itself; negative: the prepare step failed with that status)
  // and checks the count.  A chain the main kernel skips (parked by the sweep for want of
  // capacity) gets the prepare step rolled back from the prep_* copies, so that its
  // catch-up draws the same numbers.
  int32_t prepared, zbuf;
  int32_t *prep_n;             // 2 x chains
  uint64_t *prep_pos_state;    // 2 x chains: stream positions / level variance before the prepare step
  uint64_t *prep_pos_level;
  double *prep_level_sigsq;
  // the level variance THIS state draw used (the live value may already be the next round's:
  // the prepare step draws ahead); nullptr: not wanted.  Read by the look-ahead's record.
  double *level_used;
  SsmParams ssm;            // (ssm_kernel.hip only)
  // the Student-t family (StateSpaceStudentRegressionModel): every chain's per-step observation
  // variance H_t = sigma^2 / w_t, h_stride doubles apart (nullptr: the scalar sigsq[chain]);
  // the general structural kernel's HT instances read it
  const double *h;
  int64_t h_stride;
  // the Poisson family (StateSpacePoissonModel): the filtered series is every chain's own latent
  // value, y_stride doubles apart (0: the one series shared by all chains).  A list with regression
  // holiday models (RhParams) passes every chain's series less the models' effects the same way.  Read by
  // every instance of the general kernel; the template kernel reads the shared series only
  // (ssg_choose_kernel never picks it for a launch with a stride).
  int64_t y_stride;
  // the Student local linear trend (SsgSpec::student_block): every chain's weights, qw_stride doubles
  // apart -- the level's T, then the slope's T; entry t scales the state error of the step t -> t + 1
  // (nullptr: no such block).  Read by the QT instances only.
  const double *qw;
  int64_t qw_stride;
  // the random-walk holidays' packed calendar (SSG_CAL_NONE ...), cal_count >= T entries, one table
  // for all chains (nullptr: the list holds no such block).  Read by the HD instances and the forecast.
  // A list with a calendar seasonal keeps the blocks' prefix counts behind the table, in the same
  // allocation: int32 entry b * cal_count + t after the cal_count words = how many of the times 1 .. t
  // start a new season of block b (rows of other blocks are 0).
  const uint64_t *cal;
  int64_t cal_count;
  // the dynamic regressions' predictors: dyn_rows >= T rows of dyn_cols doubles, row t = the x_t of the
  // list's dynamic blocks side by side in state order, one table for all chains (nullptr: the list holds
  // no such block).  Read by the DR instances and the forecast (rows T .. T + horizon - 1).
  const double *dyn;
  int64_t dyn_rows;
  int32_t dyn_cols, dyn_pad;
};

// The Student local linear trend's own chain state (slt_kernel.hip).  c = 0 the level, 1 the slope.
struct SltParams {
  double *w;          // chains x 2 x T: the weights (SsParams::qw)
  double *res;        // chains x 2 x T: the residuals of the last state draw, entries 0 .. T - 2
  double *nu;         // chains x 2
  double *wsuf;       // chains x 6: the GammaSuf of the new weights (n, sum, sum of logs), level then slope
  uint64_t *pos;      // chains: position in SLT_PARAM_STREAM
  uint64_t *count;    // chains: state draws observed so far (the s of the weights' slots)
  int32_t nu_kind[2]; // the nu priors: STUDENT_NU_UNIFORM (a, b) / STUDENT_NU_GAMMA (a, b)
  double nu_a[2], nu_b[2];
};

// The regression holiday models of a list (reg_holiday_kernel.hip).  Coefficient j of model k is flat
// coefficient first[k] + j of the list (model order, then coefficient order).
struct RhParams {
  int32_t nmodels, ncoef;    // models of the list (0: none), their coefficients together
  int32_t nsteps;            // the steps of [0, T) at which a model is active
  int32_t pad;
  int64_t count;             // entries of the table (>= T; a forecast reads entries T .. T + horizon - 1)
  const int32_t *table;      // count x RH_MAX_MODELS: entry (t, k) = the flat coefficient of model k active at t, or -1
  const int32_t *steps;      // nsteps, ascending
  const double *counts;      // ncoef: the observed active steps of [0, T) per coefficient (every chain's)
  double *coef;              // chains x RH_MAX_COEF
  double *totals;            // chains x RH_MAX_COEF: the residual sums of the last state draw
  uint64_t *pos;             // chains: position in RH_COEF_STREAM
  double *y;                 // chains x T: the series less the models' effects (SsParams::y with y_stride = T)
  const double *y_shared;    // T: the data's series
  int32_t first[RH_MAX_MODELS + 1];
  double prior_mean[RH_MAX_MODELS], prior_sd[RH_MAX_MODELS];
};

// The hierarchical ones among them (hier_holiday_kernel.hip): model k is hierarchical where width[k] > 0,
// with nhol[k] holidays of that width; its coefficients, counts and totals are RhParams's.
struct RhhParams {
  int32_t nmodels;                 // the list's regression holiday models, plain ones included
  int32_t mask;                    // bit k: model k is hierarchical
  int32_t width[RH_MAX_MODELS], nhol[RH_MAX_MODELS];
  double nu0[RH_MAX_MODELS];       // the Wishart prior's degrees of freedom
  const double *hyper;             // RH_MAX_MODELS x RHH_HYPER_STRIDE
  double *mu;                      // chains x RH_MAX_MODELS x RHH_MAX_WIDTH
  double *omega;                   // chains x RH_MAX_MODELS x RHH_MAX_WIDTH^2 (row-major, leading dimension RHH_MAX_WIDTH)
  uint64_t *pos;                   // chains: position in RHH_STREAM
};

// The spike-and-slab autoregressions of a list (ar_spike_kernel.hip).  The prior of the block in
// autoregression slot a: the slab N(mu, siginv^-1) (siginv full storage at leading dimension AR_MAX),
// the spike's inclusion probabilities with their logs (VariableSelectionPrior), the sampler's flags.
struct ArSpikePrior {
  double mu[AR_MAX];
  double siginv[AR_MAX * AR_MAX];
  double pi[AR_MAX], log_pi[AR_MAX], log_1mpi[AR_MAX];
  int32_t truncate;    // accept stationary coefficients only
  int32_t max_flips;   // <= 0: every lag is tried in a sweep
  int32_t select;      // 0: the indicators are not drawn (allow_model_selection(false))
  int32_t pad;
};
struct ArSpikeParams {
  const ArSpikePrior *prior;   // device, SSG_MAX_AR entries (by autoregression slot)
  uint8_t *gamma;              // chains x SSG_MAX_AR x AR_MAX: the inclusion indicators
  int32_t nspike;              // such blocks in the list
  int32_t block[SSG_MAX_AR];   // ... and which they are
};

// The round kernel (ss_round_kernel.hip): every chain's workgroup loops over the rounds of a
// call by itself; the chains meet only in the X'e tiles -- up to SS_ROUND_TILE chains in the
// order they arrive.  Per round r: ticket[r] = the next place (tile * SS_ROUND_TILE + slot; a
// tile closed early moves it to the next tile's first place), members = the chain index in
// every place (-1: not yet written), sizes[tile] = members of a tile closed early (0: not).
// At most one tile per chain and round.  The host zeroes them (members: -1) before every launch.
enum { SS_ROUND_TILE = 16, SS_ROUND_MAX_ROUNDS = 64 };
struct SsRoundParams {
  int32_t rounds;           // rounds of this launch (<= SS_ROUND_MAX_ROUNDS)
  int32_t close_ticks;      // 100 MHz ticks a tile's first member waits for company
  int32_t *ticket;          // [rounds]
  int32_t *sizes;           // [rounds][chain_count]
  int32_t *members;         // [rounds][chain_count * SS_ROUND_TILE + 2 * SS_ROUND_TILE]
  double *planes;           // SS_ROUND_TILE x chains x p: a chain's partial products, by row of the series
  // the look-ahead's record of every round's draw (engine_ss.hip; rgamma == nullptr: none):
  // chain c's row of round r is (rec_slot * chains + c) * rec_len + rec_first + r
  uint8_t *rgamma;
  double *rbeta, *rsig, *rvar, *rstate;
  const int32_t *reg_of_chain;      // chains: index among the chains whose state path is recorded, or -1
  int32_t rec_slot, rec_len, rec_first, nreg;
  int32_t *debug;           // diagnostic (ba_ss_set_tuning(e, 6) in a debugging session): 16 x 16 words, else nullptr
  int32_t debug_seq;        // diagnostic build: a number per launch
  double *stamps;           // diagnostic build (-DBA_RSTAMPS): chains x 2 waves x 8 phases, 100 MHz ticks; else unused
};

enum { SS_SCRATCH_ARRAYS = 9, SS_STATE_ARRAY = 4 };   // (arrays 5-6 and 7-8: the two normals buffers)
enum { LM_BS = 16, LM_THREADS = 128, LM_TP = LM_BS * LM_THREADS };
inline __host__ __device__ int lm_at(int t) { return (t % LM_BS) * LM_THREADS + t / LM_BS; }

}  // namespace boom_amd
