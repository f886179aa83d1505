/* boom_amd -- C-ABI of the MI355X many-chain engine for BOOM's spike-and-slab
 * (BregVsSampler) and bsts local-level + regression (StateSpacePosteriorSampler)
 * hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch
 * types, no exceptions.  Every entry point names the reference interface it
 * stands in for (paths relative to the BOOM tree).  INTEGRATION.md shows the
 * binding a BOOM maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns BA_OK (0) or a negative BA_E_* code;
 *     ba_last_error() gives the message (same wording as the reference's
 *     report_error() text where one exists, cpputil/report_error.cpp:30-32);
 *   - matrices are column-major doubles exactly like BOOM::Matrix
 *     (LinAlg/Matrix.hpp:429); host pointers unless the name says _device;
 *   - caller owns every buffer it passes; the engine copies on call;
 *   - an engine lives on ONE HIP device and runs `chains` independent chains,
 *     global chain ids chain_offset .. chain_offset+chains-1 (the id keys the
 *     Philox stream, so a job sharded over ranks draws the same numbers as the
 *     same job on one device);
 *   - "chain = -1" addresses all chains at once.
 */
#ifndef BOOM_AMD_H
#define BOOM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  BA_OK = 0,
  BA_E_INVALID = -1,       /* bad argument / dimension mismatch */
  BA_E_HIP = -2,           /* HIP runtime failure (message has the HIP error) */
  BA_E_NOT_PD = -3,        /* "The posterior information matrix is not positive
                              definite..." BregVsSampler.cpp:339-350 */
  BA_E_NEGATIVE_SS = -4,   /* "Illegal data caused negative sum of squares..."
                              BregVsSampler.cpp:448-478 */
  BA_E_ILLEGAL_START = -5, /* "BregVsSampler did not start with a legal
                              configuration." BregVsSampler.cpp:364-370 */
  BA_E_RNG_BRANCH = -6,    /* a sigma^2 draw the reference itself reports as an
                              error: truncation point exactly at the gamma's mode
                              (BoundedAdaptiveRejectionSampler.cpp:50-59), or the
                              samplers' attempt limits (1000 rejections; 64 hull
                              points here) */
  BA_E_FORECAST_VARIANCE = -7, /* "Found a zero (or negative) forecast
                              variance!" ScalarKalmanFilter.cpp:48-52 */
  BA_E_MODEL_TOO_LARGE = -8,   /* model size exceeded the engine's capacity */
  BA_E_STATE = -9          /* call sequence error (e.g. sweep before priors) */
};

typedef struct ba_engine ba_engine;

typedef struct ba_config {
  int32_t device;        /* HIP device ordinal */
  int32_t chains;        /* chains resident on this device */
  int64_t chain_offset;  /* global id of local chain 0 */
  uint64_t seed;         /* sampler seed: PosteriorSampler::set_seed,
                            Models/PosteriorSamplers/PosteriorSampler.hpp:60 */
  int32_t max_model_size_hint; /* <=0: engine chooses its working capacity */
  int32_t reserved;
} ba_config;

/* message of the last failing call on this thread (never NULL) */
const char *ba_last_error(void);

/* ---- engine lifetime ---------------------------------------------------- */
int ba_engine_create(const ba_config *cfg, ba_engine **out);
void ba_engine_destroy(ba_engine *e);
/* device ordinal, chain count, predictors (0 until data are set) */
int ba_engine_info(const ba_engine *e, int32_t *device, int32_t *chains,
                   int32_t *p);

/* ---- data: RegressionModel / NeRegSuf ------------------------------------ */
/* NeRegSuf(X, y), Models/Glm/RegressionModel.cpp:309-328: builds XtX, Xty,
 * yty, n, sum(y), column sums of X on the device (f64 MFMA syrk).  X is n x p
 * column-major. */
int ba_build_suf_from_xy(ba_engine *e, int64_t n, int32_t p, const double *X,
                         const double *y);
/* same, X / y already resident in device memory of e's device */
int ba_build_suf_from_xy_device(ba_engine *e, int64_t n, int32_t p,
                                const void *X_device, const void *y_device);
/* The same build for a design matrix SHARDED BY ROWS over the ranks of a job
 * (config 4: X = 3.3 GB): every rank computes the statistics of its own rows
 * into a device block of ba_suf_block_size(p) doubles laid out as
 *   [ X'X (p x p, column-major) | X'y (p) | y'y, sum y | column sums of X (p) ],
 * the caller sums the blocks over ranks -- ONE all-reduce (RCCL over xGMI;
 * boom_amd/dist.py: build_suf_row_sharded) -- and every rank installs the total.
 * The sums are what NeRegSuf(X, y) holds (RegressionModel.cpp:309-328); every
 * rank ends up with bitwise the same statistics, so chains do not depend on
 * which rank runs them.  X_device is the shard, n_rows x p column-major. */
size_t ba_suf_block_size(int32_t p);
int ba_suf_partial_device(ba_engine *e, int64_t n_rows, int32_t p,
                          const void *X_device, const void *y_device,
                          void *block_device);
int ba_set_suf_from_block_device(ba_engine *e, int64_t n_total, int32_t p,
                                 const void *block_device);
/* NeRegSuf(XTX, XTY, YTY, n, ybar, xbar), RegressionModel.cpp:330-345 */
int ba_upload_regression_suf(ba_engine *e, int32_t p, const double *xtx,
                             const double *xty, double yty, double n,
                             double ybar, const double *xbar);
/* RegSuf accessors xtx()/xty()/yty()/n()/ybar()/xbar(),
 * RegressionModel.hpp:58-101.  Any output pointer may be NULL. */
int ba_get_regression_suf(ba_engine *e, double *xtx, double *xty, double *yty,
                          double *n, double *ybar, double *xbar);

/* ---- priors: BregVsSampler ctor #5 pieces -------------------------------- */
/* slab: MvnGivenScalarSigma(b, Omega^{-1}) (Models/MvnGivenScalarSigma.hpp:57-109;
 * BregVsSampler::set_slab, BregVsSampler.hpp:111-113) */
int ba_set_slab(ba_engine *e, const double *prior_mean,
                const double *unscaled_prior_precision);
/* spike: VariableSelectionPrior(pi) + set_max_model_size (< 0: none)
 * (VariableSelectionPrior.hpp:101,133; BregVsSampler::set_spike) */
int ba_set_spike(ba_engine *e, const double *prior_inclusion_probabilities,
                 int64_t max_model_size);
/* residual precision prior ChisqModel(df, sigma_guess) + set_sigma_upper_limit
 * (ChisqModel.cpp:56-57; BregVsSampler.cpp:264-266); sigma_upper_limit = +inf
 * for none */
int ba_set_sigma_prior(ba_engine *e, double prior_df, double sigma_guess,
                       double sigma_upper_limit);
/* convenience ctors #1 and #2 (BregVsSampler.cpp:48-85, :87-142): assemble the
 * three priors above from the current sufficient statistics */
int ba_set_priors_ctor1(ba_engine *e, double prior_nobs, double expected_rsq,
                        double expected_model_size,
                        int32_t first_term_is_intercept);
int ba_set_priors_ctor2(ba_engine *e, double prior_sigma_nobs,
                        double prior_sigma_guess, double prior_beta_nobs,
                        double diagonal_shrinkage,
                        double prior_inclusion_probability,
                        int32_t force_intercept);
/* read back the assembled priors (any pointer may be NULL) */
int ba_get_priors(ba_engine *e, double *prior_mean, double *ominv, double *pi,
                  double *prior_df, double *prior_ss);

/* limit_model_selection / suppress_model_selection (max_flips: <0 = p, 0 =
 * none), set_correlation_swap_threshold, suppress_beta_draw /
 * suppress_sigma_draw (BregVsSampler.hpp:131-161) */
int ba_set_options(ba_engine *e, int32_t max_flips, double swap_threshold,
                   int32_t draw_beta, int32_t draw_sigma);

/* Overrides of choices the engine otherwise makes itself; never needed for
 * correctness (every setting produces the same chains), used by the tests to
 * force every code path and by diagnostics:
 *   waves_per_chain  0 = engine chooses; 1, 2 or 4 wavefronts per chain
 *   walk_policy      -1 = default (adaptive); 0 batch mode only, 1 adaptive,
 *                    2 always the proposal table, 3 adaptive without forked
 *                    quiet sweeps, 4 adaptive with a fork at a sweep's start
 *                    only (under 1 and 2 a table walk resumed after a stop
 *                    runs beside the sweep's tail as well)
 *   kcap_start       0 = default; first model capacity tried (16, 32, ...) */
int ba_set_tuning(ba_engine *e, int32_t waves_per_chain, int32_t walk_policy,
                  int32_t kcap_start);
/* A further override of the same kind (same chains either way, bit for bit): how the sweep
 * kernels rebuild the two Cholesky factors when ONE variable enters or leaves the model.
 *   0 = keep the leading columns the flip leaves unchanged and compute the rest (default)
 *   1 = always factor from scratch
 * Drops nothing the engine keeps between calls; takes effect with the next launch. */
int ba_set_rebuild_policy(ba_engine *e, int32_t policy);
/* The samplers that give every draw its own slot of a stream (the bsts state draw's normals:
 * 256 positions a normal; the probit / logit / Polya-Gamma / Poisson imputers: 4096 / 256 /
 * 4096 / 256 positions an observation) let a draw that needs more uniforms than its slot
 * holds go on in the slot's SPILL stream (same chain, stream id | 0x80000000, position
 * slot << 20) -- an event of probability < 1e-40 at these strides.  For the tests of that
 * path: a slot hands out only `uniforms` numbers (even; 0 = the whole stride again), so
 * that the spill streams are read all the time.  The oracle's bo_set_slot_limit is the
 * same switch.  Changes the draws. */
int ba_set_slot_limit(ba_engine *e, int32_t uniforms);

/* ---- chain state: GlmCoefs (beta, inc) + sigsq ----------------------------- */
/* coef().set_inc / set_Beta / set_sigsq.  gamma: p bytes (0/1), beta: p
 * doubles (may be NULL = zeros).  chain = -1 sets every chain. */
int ba_set_state(ba_engine *e, int64_t chain, const uint8_t *gamma,
                 const double *beta, double sigsq);
/* coef().inc() / Beta() / sigsq() of one chain (local index).  While
 * ba_draw_next() is serving a look-ahead batch these are the draw being served,
 * not the end of the batch. */
int ba_get_state(ba_engine *e, int64_t chain, uint8_t *gamma, double *beta,
                 double *sigsq);
/* all chains at once: gamma chains x p, beta chains x p, sigsq chains */
int ba_get_states(ba_engine *e, uint8_t *gamma, double *beta, double *sigsq);
/* PosteriorSampler::logpri() of BregVsSampler (BregVsSampler.cpp:380-393) at the
 * current state of one chain (local index): log p(gamma) + log p(sigma^2) +
 * log N(beta_gamma | b_gamma, sigma^2 Omega_gamma) */
int ba_logpri(ba_engine *e, int64_t chain, double *out);
/* PosteriorSampler::set_seed: re-keys the streams of every sampler of every
 * chain (regression, SpikeSlab, level, state), all at position 0 */
int ba_seed(ba_engine *e, uint64_t seed);

/* ---- the hot path ---------------------------------------------------------- */
/* nsweeps x BregVsSampler::draw() (BregVsSampler.cpp:252-261) on every chain.
 * Asynchronous: returns after the launch.  Errors raised by chains surface at
 * the next ba_sync()/ba_get_*(). */
int ba_sweep(ba_engine *e, int32_t nsweeps);
/* wait for outstanding work and report the first chain error, if any.  (The chains'
 * status words come back in one batched copy; a ba_sync() that follows a clean one with
 * nothing in between but accessors -- ba_get_state, ba_ss_get_state, ba_logpri ... , each
 * of which begins with one -- is only the wait.)  While ba_ss_draw_next is serving draws
 * from a look-ahead batch, ba_sync waits for THAT batch only: the batch running ahead of it
 * stays in flight (a chain that stops there is reported when its draws are served), and it is
 * no barrier for work the caller queued on ba_stream() -- synchronise that stream itself. */
int ba_sync(ba_engine *e);
/* The reference's calling pattern is ONE draw() per MCMC iteration with the
 * caller reading the parameters in between (spike_slab_wrapper.cc:233-242,
 * spikeslab.py:191-207; Model::sample_posterior, Models/ModelTypes.hpp:93).
 * ba_draw_next() keeps that pattern at the long-launch rate: every `lookahead`
 * calls it launches `lookahead` sweeps of EVERY chain with the draws recorded
 * on the device, the calls in between only move a cursor, and
 * ba_get_state / ba_get_states / ba_logpri return the draw under the cursor --
 * bitwise what `ba_sweep(e, 1)` per iteration leaves there.  Any other call
 * that touches the engine (data, priors, options, state, seed, ba_sweep) first
 * puts the chains back where the caller has seen them (the batch's start state
 * replayed up to the cursor), so the sequence of draws never depends on the
 * look-ahead length.  Running summaries count launched sweeps, i.e. they run
 * ahead of the cursor by up to lookahead - 1 draws.
 * ba_set_lookahead(e, n): n >= 1 (1 = one launch per call; replaces any
 * ba_enable_traces / ba_enable_draws setting). */
int ba_set_lookahead(ba_engine *e, int32_t lookahead);
int ba_draw_next(ba_engine *e);
/* log_model_prob(gamma) for ngamma inclusion vectors (BregVsSampler.cpp:216-239)
 * on the regression model's sufficient statistics, models of any size (up to 1024
 * included variables); BA_E_STATE once state-space data are set (there they are per
 * chain and move every sweep) */
int ba_log_model_prob(ba_engine *e, int32_t ngamma, const uint8_t *gammas,
                      double *out);

/* ---- SpikeSlabSampler: the sigma^2-conditional sweep ---------------------------- */
/* Models/Glm/PosteriorSamplers/SpikeSlabSampler.{hpp,cpp}: the helper that the
 * logit / probit / Poisson / Student / quantile samplers drive with their own
 * (weighted) sufficient statistics and the current residual variance.
 *   slab      SpikeSlabSampler(model, slab_prior, spike_prior) (.hpp:47): mean mu
 *             and precision; precision_scales_with_sigsq = 1 for
 *             MvnGivenScalarSigma (siginv() = Omega^{-1} / sigma^2,
 *             MvnGivenScalarSigma.cpp:74-77), 0 for a fixed-precision MvnBase
 *             (then every chain must hold the same sigma^2);
 *   max_flips limit_model_selection(max_flips) (.hpp:132): limits only if > 0;
 *   spike     ba_set_spike; data: ba_upload_regression_suf with the weighted
 *             X'WX, X'Wy (WeightedRegSuf; yty, n, ybar, xbar are not used);
 *   sigma^2   per chain, ba_set_sigsq / ba_set_state.
 * ba_sss_sweep runs nsweeps x { draw_model_indicators(rng, suf, sigsq);
 * draw_beta(rng, suf, sigsq) } (SpikeSlabSampler.cpp:40-138) on every chain. */
int ba_set_sigsq(ba_engine *e, int64_t chain, double sigsq);
int ba_sss_set_slab(ba_engine *e, const double *mu, const double *precision,
                    int32_t precision_scales_with_sigsq, int32_t max_flips);
int ba_sss_sweep(ba_engine *e, int32_t nsweeps);

/* ---- AdaptiveSpikeSlabRegressionSampler: what lm.spike runs for p > 100 -------- */
/* Models/Glm/PosteriorSamplers/AdaptiveSpikeSlabRegressionSampler.{hpp,cpp}
 * (Interfaces/R/BoomSpikeSlab/src/spike_slab_wrapper.cc:99-140): same model,
 * priors (ba_set_slab / ba_set_spike / ba_set_sigma_prior) and chain state as
 * BregVsSampler; a sweep is min(max_flips, p) birth / death moves with adaptive
 * proposal rates, then sigma^2 and beta.
 *   ba_adaptive_set_options  limit_model_selection(max_flips) (default 100; 0 =
 *                            allow_model_selection(false)), set_step_size
 *                            (.001), set_target_acceptance_rate (.345); a
 *                            negative value keeps the current setting
 *   ba_adaptive_sweep        nsweeps x draw() (.cpp:62-85) on every chain
 *   ba_adaptive_get_rates    birth_rates_, death_rates_, iteration_count_ of a
 *                            chain (any pointer may be NULL)
 * A chain whose model grows beyond 64 variables moves to the large-model kernel, as
 * BregVsSampler's chains do (its moves are then read off that kernel's table of
 * log model probabilities, rebuilt after every accepted move); the limit is the
 * large-model kernel's (1024 variables), beyond it BA_E_MODEL_TOO_LARGE. */
int ba_adaptive_set_options(ba_engine *e, int32_t max_flips, double step_size,
                            double target_acceptance_rate);
int ba_adaptive_sweep(ba_engine *e, int32_t nsweeps);
int ba_adaptive_get_rates(ba_engine *e, int64_t chain, double *birth_rates,
                          double *death_rates, uint64_t *iteration_count);

/* ---- BinomialProbitSpikeSlabSampler (the probit member) -----
 * Data augmentation (BinomialProbitDataImputer.cpp:30-73: a truncated normal per
 * trial, or the central-limit draw beyond clt_threshold trials of a kind) followed
 * by SpikeSlabSampler on the complete-data sufficient statistics X'NX (fixed) and
 * X'z (BinomialProbitSpikeSlabSampler.cpp:40-85).  X is n x p column-major, y
 * successes, ntrials trials.  Priors: ba_sss_set_slab(mu, precision,
 * scales_with_sigsq = 0, max_flips) and ba_set_spike.  State through
 * ba_set_state / ba_get_state(s) (sigma^2 is 1).  RNG: stream 3 for the
 * inclusion / coefficient draws; the imputation of observation i in sweep s reads
 * stream 8 from position (s n + i) * 4096 -- the reference reads ONE stream in
 * sequence, a counter-based one lets the observations go in parallel. */
int ba_probit_set_data(ba_engine *e, int64_t n, int32_t p, const double *X,
                       const double *y, const double *ntrials, int32_t clt_threshold);
int ba_probit_sweep(ba_engine *e, int32_t nsweeps);

/* ---- BinomialLogitSpikeSlabSampler (the logit member; the
 * sampler behind BASELINE config 5, with the reference's own auxiliary-mixture
 * imputer -- it has no Polya-Gamma one) -------------------------------------------
 * Per sweep: every trial's truncated logistic draw and mixture component
 * (BinomialLogitAuxmixSampler.cpp:77-97, BinomialLogitDataImputer.cpp:128-144),
 * X'Wz for all chains by one MFMA GEMM, of every chain's own slab precision + X'WX
 * the vectors the sweep reads (those of included variables, built by one gathered
 * MFMA GEMM; a variable that enters mid-sweep has its vector built on request and
 * the chain replays that sweep), then the sampler's inclusion / coefficient draws
 * (BinomialLogitSpikeSlabSampler.cpp:50-117, :178-226; its shuffle of the visiting
 * order differs from SpikeSlabSampler's).  Same prior setters and state accessors as
 * the probit sampler.  Observations with more than clt_threshold (1 .. 64) trials take
 * the reference's large-sample imputation (BinomialLogitCltDataImputer::
 * impute_large_sample, BinomialLogitDataImputer.cpp:155-211: multinomial counts per
 * mixture component, one normal draw); models of any size.  RNG: stream 3 for the
 * sampler, stream 9 from position (s n + i) * 256 for the imputation of observation i
 * in sweep s (two uniforms per trial, or the large-sample branch's few dozen). */
int ba_logit_set_data(ba_engine *e, int64_t n, int32_t p, const double *X,
                      const double *y, const double *ntrials, int32_t clt_threshold);
int ba_logit_sweep(ba_engine *e, int32_t nsweeps);
/* The imputation step of the logit sampler: 0 (default) the reference's auxiliary
 * mixture; 1 Polya-Gamma augmentation -- omega_i ~ PG(n_i, x_i'beta) by Devroye's exact
 * sampler (Polson, Scott and Windle 2013), the normal with PG's moments beyond
 * clt_threshold trials; (y_i - n_i / 2, omega_i) takes the place of the mixture's
 * (information-weighted sum, information), everything else is the same sweep.  BOOM has
 * NO Polya-Gamma sampler (BASELINE config 5 names one): there is nothing to be
 * bit-compared with; the chain it defines has the same stationary distribution as the
 * logit likelihood's exact posterior, which the auxiliary-mixture sampler approximates,
 * and is checked against that sampler distributionally.  RNG: stream 10, observation i
 * of sweep s from position (s n + i) * 4096. */
int ba_logit_set_imputer(ba_engine *e, int32_t kind);

/* ---- PoissonRegressionSpikeSlabSampler (the Poisson member) -----------
 * Models/Glm/PosteriorSamplers/PoissonRegressionSpikeSlabSampler.cpp:55-59: per sweep the
 * auxiliary-mixture imputation of Fruehwirth-Schnatter et al. (PoissonDataImputer.cpp:36-96:
 * the last event time inside the exposure interval ~ exposure x Beta(y, 1), the first
 * event after it, each negative log time unmixed against a normal mixture of
 * NegLogGamma(count)), then SpikeSlabSampler's inclusion / coefficient draws on the
 * complete-data sufficient statistics -- on the device the logit path's machinery: X'Wz by
 * one MFMA GEMM, every chain's own slab precision + X'WX a vector at a time.
 *   ba_poisson_set_data      X n x p column-major, y counts, exposure (> 0)
 *   ba_poisson_set_mixtures  the mixtures, BY THE CALLER: the reference keeps them in a
 *                            table that interpolates and refits on demand
 *                            (create_poisson_mixture_approximation_table /
 *                            NormalMixtureApproximationTable::approximate); the BOOM-side
 *                            binding reads its table, the tests a fixture generated from
 *                            the compiled reference.  counts ascending (must cover 1 and
 *                            every positive count in the data below largest_index, from
 *                            where on the Gaussian limit is used); mixture i has ncomp[i]
 *                            (<= 32) components, packed in mu / sigma / weight
 *   priors, state            ba_sss_set_slab(mu, precision, 0, max_flips), ba_set_spike,
 *                            ba_set_state / ba_get_state(s) as for the logit sampler
 * RNG: stream 3 for the sampler, stream 11 from position (s n + i) * 256 for the
 * imputation of observation i in sweep s. */
int ba_poisson_set_data(ba_engine *e, int64_t n, int32_t p, const double *X, const double *y,
                        const double *exposure);
int ba_poisson_set_mixtures(ba_engine *e, int32_t ncounts, const int64_t *counts,
                            const int32_t *ncomp, const double *mu, const double *sigma,
                            const double *weight, int64_t largest_index);
int ba_poisson_sweep(ba_engine *e, int32_t nsweeps);

/* ---- TRegressionSpikeSlabSampler (lm.spike's error.distribution = "student") ---------------
 * Models/Glm/PosteriorSamplers/TRegressionSpikeSlabSampler.cpp:41-47: per sweep the weights
 * w_i ~ Gamma((nu + 1) / 2, rate (nu + (r_i / sigma)^2) / 2) (TDataImputer.cpp:26-30), then
 * SpikeSlabSampler's inclusion / coefficient draws given sigma^2 on the weighted suf (the
 * logit path's machinery: X'Wy by one GEMM, every chain's own Omega^{-1} + X'WX a vector at a
 * time), sigma^2 | beta, w (GenericGaussianVarianceSampler, n observations), and nu by the
 * slice sampler on the observed-data likelihood (ScalarSliceSampler, lower limit 0).
 *   ba_student_set_data      X n x p column-major, y n; Student mode
 *   priors                   ba_sss_set_slab(mu, precision, 1, max_flips), ba_set_spike,
 *                            ba_set_sigma_prior(df, sigma_guess, sigma_upper_limit)
 *   ba_student_set_nu_prior  kind 0: Uniform(a, b); kind 1: Gamma(a, b) (shape, rate);
 *                            default Uniform(0.1, 100) (R's lm.spike)
 *   ba_student_set_nu / _get_nu   chain -1: every chain; the default nu is 30
 *   ba_student_sweep         nsweeps x draw() on every chain; ba_set_state / ba_get_state(s)
 *                            carry gamma, beta and sigma^2; with ba_enable_draws the draws
 *                            of the call are recorded (ba_get_draws, ba_predict) and
 *                            ba_student_get_nu_draws returns the recorded nu path
 *   ba_student_get_weights   the last imputation's n weights of one chain (diagnostics)
 *   ba_student_get_margin    per chain (chain -1: all), the smallest relative gap between the
 *                            two sides of a slice-sampler comparison since the data were set
 *   ba_student_allow_model_selection  SpikeSlabSampler::allow_model_selection: 0 skips the
 *                            inclusion draws (no numbers read for them), 1 (default) draws them
 * ba_student_set_data starts a new model: nu = 30, the slice width 1, no margin yet.
 * ba_get_summaries' sigma^2 moments are those of the sigma^2 draws.
 * RNG: stream 3 for the inclusion / coefficient draws; stream 31 from position
 * (s n + i) * 256 for the weight of observation i in sweep s; stream 15 from position
 * s * 4096 for sigma^2 and then nu in sweep s. */
int ba_student_set_data(ba_engine *e, int64_t n, int32_t p, const double *X, const double *y);
int ba_student_set_nu_prior(ba_engine *e, int32_t kind, double a, double b);
int ba_student_set_nu(ba_engine *e, int64_t chain, double nu);
int ba_student_get_nu(ba_engine *e, int64_t chain, double *nu);
int ba_student_sweep(ba_engine *e, int32_t nsweeps);
int ba_student_get_weights(ba_engine *e, int64_t chain, double *w);
int ba_student_get_nu_draws(ba_engine *e, int64_t chain, int32_t nsweeps, double *out);
int ba_student_get_margin(ba_engine *e, int64_t chain, double *margin);
int ba_student_allow_model_selection(ba_engine *e, int32_t allow);
/* (ba_student_set_nu_prior, _set_nu, _get_nu, _get_nu_draws, _get_margin and
 * _allow_model_selection serve the state space Student-t family, ba_ss_student_*, too) */

/* ---- QuantileRegressionSpikeSlabSampler (qreg.spike) ----------------------------------------
 * Models/Glm/PosteriorSamplers/QuantileRegressionPosteriorSampler.cpp:30-39, :77-91: per sweep,
 * for every observation with residual r_i = |y_i - x_i'beta| > 0 the weight
 * w_i = lambda_inv ~ InverseGaussian(mean 1 / r_i, shape 1) (rig_mt), the weighted regression
 * of y*_i = y_i - (2 (1 - quantile) - 1) / w_i on x_i with weights w_i, then SpikeSlabSampler's
 * inclusion / coefficient draws at sigma^2 = 1 -- the Poisson path's machinery with another
 * imputation.  An observation with a zero residual is left out of that sweep's regression
 * (weight 0, no random numbers read).  There is no sigma^2 and no nu.  The chains target
 * the density proportional to prior(beta) exp(-2 sum_i rho_q(y_i - x_i'beta)), rho_q the check loss.
 *   ba_quantile_set_data     X n x p column-major, y n, 0 < quantile < 1
 *   priors, state            ba_sss_set_slab(mu, precision, 0, max_flips), ba_set_spike,
 *                            ba_set_state / ba_get_state(s) as for the Poisson sampler (sigma^2 is 1)
 *   ba_quantile_sweep        nsweeps x draw() on every chain
 *   ba_quantile_get_weights  the last imputation's n weights lambda_inv of one chain, 0 where
 *                            the residual was 0
 * The smaller root of rig_mt's quadratic is evaluated as mu / (1 + t + sqrt(t (2 + t))),
 * t = mu y / (2 lambda): the reference's form cancels at small residuals.
 * RNG: stream 3 for the inclusion / coefficient draws; stream 32 from position
 * (s n + i) * 256 for the weight of observation i in sweep s (one normal, then one uniform). */
int ba_quantile_set_data(ba_engine *e, int64_t n, int32_t p, const double *X, const double *y,
                         double quantile);
int ba_quantile_sweep(ba_engine *e, int32_t nsweeps);
int ba_quantile_get_weights(ba_engine *e, int64_t chain, double *w);

/* ---- MLVS: multinomial logit spike and slab (mlm.spike's data-augmentation move) -------------
 * Models/Glm/PosteriorSamplers/MLVS.cpp:71-75 (draw), :101-118 (draw_beta), :120-153
 * (keep_flip, draw_inclusion_vector), :163-190 (log_model_prob); the imputation is
 * MLVS_data_imputer.cpp:51-82.  n observations choose among M = nchoices alternatives; the
 * model's D = (M - 1) psub + pch coefficients are laid out as ChoiceData::write_x(false) does
 * (Models/Glm/ChoiceData.cpp:93-115): expanded row i M + m holds xsubject_i in columns
 * [(m - 1) psub, m psub) for m >= 1 -- choice 0 is the baseline -- and xchoice_{i, m} in the
 * last pch columns.  Per sweep and observation: eta_m = row (i, m) times beta, the
 * Fruhwirth-Schnatter / Fruhwirth utilities u_m (u_y = -rlexp(lse(eta)); the others
 * -lse2(logzmin, rlexp(eta_m))), for every m the component k of the ten-component normal
 * mixture given u_m - eta_m, u_m -= mu_k and w_m = 1 / sigma_k^2; then X'WX, X'Wu and
 * weighted_sum_of_squares = sum w u^2 (MultinomialLogitCompleteDataSuf.cpp:41-50), the
 * inclusion sweep and beta ~ N(V_g^{-1}(X'Wu_g + Omega^{-1}_g mu_g), V_g^{-1}).  The sweep is
 * not SpikeSlabSampler's: it visits the first min(D, max_flips) entries of one fixed order,
 * keeps a flip iff u < logit_inv(logp_new - logp_old), the empty model's value is
 * log prior + weighted_sum_of_squares / 2 (the reference's sign, MLVS.cpp:166-168), and a start
 * whose value is not finite is an error (BA_E_ILLEGAL_START, "MLVS did not start with a legal
 * configuration.") -- there is no make_valid.  Every flip consumes its uniform (the reference
 * skips it when logp_new is not finite).
 *   ba_mlogit_set_data        y n int32 in 0 .. M - 1; Xsubject n x psub column-major (NULL iff
 *                             psub == 0); Xchoice (n M) x pch column-major, row i M + m (NULL
 *                             iff pch == 0); 2 <= M <= 16.  The expanded design and its square
 *                             are built on the device: 16 n M D bytes, refused above 8 GiB
 *   ba_mlogit_set_flip_order  the sweep's visiting order, D int32, a permutation (default: the
 *                             identity).  The reference's is std::shuffle(seq, std::default_random_engine())
 *                             with a fresh engine on every draw, i.e. always the same one: a
 *                             caller computes it with that very call (boom_amd.hpp does)
 *   priors, state             ba_sss_set_slab(mu, precision, 0, max_flips), ba_set_spike,
 *                             ba_set_state / ba_get_state(s) as for the Poisson sampler (sigma^2 is 1)
 *   ba_mlogit_allow_model_selection  0: suppress_model_selection (beta only); 1: the default
 *   ba_mlogit_sweep           nsweeps x draw() on every chain
 *   ba_mlogit_get_latent      the last imputation's N = n M utilities (less their component's
 *                             mean) and weights of one chain, row i M + m
 *   ba_mlogit_get_wss         weighted_sum_of_squares of the last imputation of one chain
 * Models of more than 64 included variables are not served (BA_E_MODEL_TOO_LARGE).  Not
 * covered: log_sampling_probs (downsampling), restricted choice sets, the composite
 * sampler's RWM / TIM moves (mlm.spike's proposal.weights beyond DA), the ba_group_* wrappers.
 * RNG: stream 3 for the flips (max_flips uniforms a sweep, no shuffle uniforms) and the
 * coefficient draw; stream 48 from position (s n + i) * 64 for observation i in sweep s: one
 * uniform for rlexp(loglam), then for m = 0 .. M - 1 one for rlexp(eta_m) unless m = y_i and
 * one for the component -- 2 M in all, plus one per redraw of an rlexp whose log(-log(U)) is
 * not finite. */
int ba_mlogit_set_data(ba_engine *e, int64_t n, int32_t nchoices, int32_t psub, int32_t pch,
                       const int32_t *y, const double *Xsubject, const double *Xchoice);
int ba_mlogit_set_flip_order(ba_engine *e, const int32_t *order);
int ba_mlogit_allow_model_selection(ba_engine *e, int32_t allow);
int ba_mlogit_sweep(ba_engine *e, int32_t nsweeps);
int ba_mlogit_get_latent(ba_engine *e, int64_t chain, double *u, double *w);
int ba_mlogit_get_wss(ba_engine *e, int64_t chain, double *wss);

/* ---- posterior summaries --------------------------------------------------- */
/* Running sums over every sweep since the last ba_reset_summaries(), reduced
 * over this engine's chains on the device:
 *   inclusion_count[p] (as double), beta_sum[p], beta_sumsq[p],
 *   scalars[16] = {sweeps*chains, sum sigsq, sum sigsq^2, sum |gamma|,
 *                  accepted flips, proposed flips, min accept margin, accepted
 *                  flips served from a chain's other slot,
 *                  [8..15] per-phase cycle counters of the diagnostic build
 *                  (zero in the production library; after ba_adaptive_sweep
 *                  scalar 8 is the smallest relative distance of a weighted-
 *                  draw uniform from a boundary of the cumulative rates)}
 * The layout is one contiguous block of (3p + 16) doubles so that a single
 * collective moves it (see ba_summaries_device). */
int ba_reset_summaries(ba_engine *e);
int ba_get_summaries(ba_engine *e, double *inclusion_count, double *beta_sum,
                     double *beta_sumsq, double *scalars);
/* reduce into a device buffer of (3p + 16) doubles owned by the caller (e.g. a
 * torch tensor that then goes through RCCL); stream-ordered on the engine's
 * stream followed by a sync */
int ba_summaries_device(ba_engine *e, void *out_device);
/* per-sweep traces of the last ba_sweep call for ESS: each chains x nsweeps,
 * row-major; any pointer may be NULL.  Tracing must be enabled first. */
int ba_enable_traces(ba_engine *e, int32_t max_sweeps);
int ba_get_traces(ba_engine *e, int32_t nsweeps, double *sigsq, double *logp,
                  double *model_size);
/* Recording of every sweep's draw (the step the callers do on the host today:
 * RListIoManager::write, Interfaces/R/list_io.cpp; spikeslab.py:191-207): with
 * recording enabled a ba_sweep(n) call keeps the n draws of every chain on the
 * device (traces included), so a `for (i < niter) sample_posterior(); record()`
 * loop becomes one launch and niter reads.  ba_get_draws expands one chain's
 * (local index, as everywhere) draws: gamma nsweeps x p, beta nsweeps x p
 * (zeros outside gamma), sigsq nsweeps; any pointer may be NULL. */
int ba_enable_draws(ba_engine *e, int32_t max_sweeps);
int ba_get_draws(ba_engine *e, int64_t chain, int32_t nsweeps, uint8_t *gamma,
                 double *beta, double *sigsq);

/* Posterior predictive means from the record (lm_spike.predict, spikeslab.py:530-546:
 * coefficient_draws[burn:, :] @ predictors.T), all chains at once: draws
 * [first_draw, first_draw + ndraws) of the last recorded ba_sweep call (first_draw =
 * the caller's burn-in), newX column-major nnew x p, out chains x ndraws x nnew. */
int ba_predict(ba_engine *e, int32_t first_draw, int32_t ndraws, int32_t nnew,
               const double *newX, double *out);

/* the recorded coefficient paths of chosen variables (ESS of the largest
 * coefficients): out is chains x nvars x nsweeps, 0 where a variable was
 * excluded */
int ba_get_coefficient_traces(ba_engine *e, int32_t nsweeps, int32_t nvars,
                              const int32_t *vars, double *out);

/* the engine's HIP stream (hipStream_t) for callers that order their own work: what is put
 * on it after this call runs after every launch the engine has issued (consecutive
 * ba_sweep calls overlap on a second stream of the engine; this call joins them) */
void *ba_stream(ba_engine *e);

/* ---- measurement -------------------------------------------------------------
 * Device time per kernel class (new; no reference counterpart -- the reference has
 * no profiler hook).  With timing enabled every kernel launch of the
 * engine is bracketed by a pair of HIP events on the engine's stream;
 * ba_get_kernel_times waits for the stream and returns, per class, the summed
 * milliseconds and the number of launches since the last reset (arrays of
 * ba_kernel_classes() entries; either may be NULL).  A sweep round that is several
 * kernels (bsts: SSVS + Kalman + X'e GEMM) is timed kernel by kernel this way;
 * bench.py's roofline objects come from here.  Disabled (the default) it costs
 * nothing; it never changes a draw.  enabled = 1 also keeps consecutive ba_sweep launches
 * apart (one launch at a time: clean per-kernel figures); enabled = 2 lets them overlap as
 * they do untimed (each launch's pair sits on the stream the launch went to). */
int32_t ba_kernel_classes(void);
const char *ba_kernel_class_name(int32_t cls);
int ba_set_kernel_timing(ba_engine *e, int32_t enabled);
int ba_get_kernel_times(ba_engine *e, double *ms, int64_t *launches, int32_t reset);

/* ---- bsts: StateSpaceRegressionModel + LocalLevelStateModel ----------------- */
/* StateSpaceRegressionModel(y, X, observed) (StateSpaceRegressionModel.cpp:100-125):
 * X is T x p column-major; observed may be NULL.  Replaces the engine's data:
 * XtX is fixed, per-chain Xty / yty / n are rebuilt by every impute_state. */
int ba_ss_set_data(ba_engine *e, int32_t T, int32_t p, const double *y,
                   const double *X, const uint8_t *observed);
/* LocalLevelStateModel + ZeroMeanGaussianConjSampler(df, sigma_guess) with
 * set_sigma_upper_limit, set_initial_state_mean / _variance
 * (LocalLevelStateModel.cpp:32-91; ZeroMeanGaussianConjSampler.cpp:37-60) */
int ba_ss_set_local_level(ba_engine *e, double level_df,
                          double level_sigma_guess,
                          double level_sigma_upper_limit,
                          double initial_state_mean,
                          double initial_state_variance,
                          double initial_level_sigma);
/* Richer state, instead of ba_ss_set_local_level: BOOM's
 * block-diagonal state -- any list of state models, in the order add_state receives
 * them (Models/StateSpace/StateSpaceModelBase.hpp:637-638; the transition / variance
 * matrices are block diagonal, Filters/SparseMatrix.hpp:2196).
 *
 * ba_ss_add_state_model appends ONE state model (the first call after
 * ba_ss_set_local_level / ba_ss_clear_state_models starts a new list):
 *   kind 1  LocalLevelStateModel + ZeroMeanGaussianConjSampler
 *           (StateModels/LocalLevelStateModel.cpp)                      1 component
 *   kind 2  LocalLinearTrendStateModel with one ZeroMeanMvnIndependenceSampler per
 *           variance, as bsts builds it (StateModels/LocalLinearTrend.cpp,
 *           PosteriorSamplers/ZeroMeanMvnIndependenceSampler.cpp:63-70)  2 components
 *   kind 3  SeasonalStateModel(nseasons = iparams[0], season_duration = iparams[1])
 *           with set_time_of_first_observation(iparams[2]) and a
 *           ZeroMeanGaussianConjSampler (StateModels/SeasonalStateModel.cpp: the
 *           transition / state-error variance are the seasonal matrices on the steps
 *           INTO a new season, :89-104, :248-258, and identity / zero inside one)
 *                                                                        nseasons - 1
 *   kind 4  ArStateModel(lags = iparams[0] <= 16) + ArPosteriorSampler(ChisqModel(df,
 *           sigma_guess)) (StateModels/ArStateModel.cpp; Models/TimeSeries/
 *           PosteriorSamplers/ArPosteriorSampler.cpp:52-143: up to three multivariate
 *           proposals for phi, accepted when stationary, else one coefficient at a time
 *           from a truncated normal -- the reference's Tn2Sampler on the device,
 *           distributions/Tn2Sampler.cpp:25-131 --; then sigma)          lags
 *   kind 5  StaticInterceptStateModel (StateModels/StaticInterceptStateModel.hpp:35-131,
 *           .cpp:29-54): T = 1, no state error, no parameter and no sampler -- the var_*
 *           arrays are not read (may be NULL); its value is its initial draw
 *           N(initial_state_mean, initial_state_variance >= 0), moved by the smoother  1
 *   kind 6  TrigStateModel(period, frequencies) (StateModels/TrigStateModel.cpp:130-223):
 *           iparams[0] = the number of frequencies (<= 32); initial_phi = the 2 x 2 rotations
 *           of the transition matrix, (cos, sin) of 2 pi f / period per frequency, as
 *           state_transition_matrix(0) holds them (the caller computes them -- or reads them
 *           off the reference's model object -- so that no second cosine routine is involved);
 *           Z = 1 at every pair's first component; ONE variance for all components with its
 *           ZeroMeanGaussianConjSampler(ChisqModel(df, sigma_guess)), as bsts builds it
 *           (Interfaces/R/bsts/src/create_state_model.cpp:559-586)          2 x frequencies
 *   kind 7  SemilocalLinearTrendStateModel(level, slope) (StateModels/SemilocalLinearTrend.cpp:
 *           37-323): state (level, slope, the slope's long-run mean mu); level' = level + slope +
 *           e1, slope' = mu + phi (slope - mu) + e2.  The level's variance has a
 *           ZeroMeanGaussianConjSampler, the slope's NonzeroMeanAr1Model (mu, phi, sigma) a
 *           NonzeroMeanAr1Sampler (Models/TimeSeries/PosteriorSamplers/NonzeroMeanAr1Sampler.cpp:
 *           58-137: mu | phi, sigma normal; phi | mu, sigma normal, truncated to (-1, 1) -- or
 *           (0, 1) -- by rejection when forced stationary (positive); sigma from the residual sum
 *           of squares), as bsts builds it (create_state_model.cpp:600-672).  iparams =
 *           {force_stationary, force_positive} (positive without stationary -- a one-sided
 *           truncation -- is refused); the var_* arrays have two entries (level, slope);
 *           initial_phi = {mu's prior mean, sd, phi's prior mean, sd, initial mu, initial phi};
 *           initial_state_mean / _variance have three entries, the third is not read (the
 *           component IS mu: mean mu, variance 0).  Takes one of the 4 autoregression slots.  3
 *   kind 8  StudentLocalLinearTrendStateModel (StateModels/StudentLocalLinearTrend.cpp, bsts
 *           AddStudentLocalLinearTrend): state (level, slope) as kind 2, but the level and slope
 *           errors of the step t -> t + 1 have the variances sigma_c^2 / w_c[t] with latent weights
 *           w_c[t] ~ Gamma(nu_c / 2, nu_c / 2): Student-t errors with nu_c degrees of freedom.  Its
 *           StudentLocalLinearTrendPosteriorSampler draws sigma_level^2, nu_level, sigma_slope^2,
 *           nu_slope (sigma^2 from the weighted sum of squares, nu by a new unimodal
 *           ScalarSliceSampler per draw); observe_state redraws the weights after every state
 *           draw.  The var_* arrays have two entries (level, slope); initial_phi = {nu_level prior
 *           kind, a, b, nu_slope prior kind, a, b, initial nu_level, initial nu_slope}, the prior
 *           kinds as ba_student_set_nu_prior's (0: uniform(a, b) -- bsts's default is (1, 500);
 *           1: gamma(a, b)).  Refused: an initial nu that is not positive or has zero prior
 *           density, a second such model in the list, the Student-t / Poisson / logit observation
 *           families.  With it ba_ss_forecast ("forecasts with a Student local linear trend are not
 *           implemented") and a look-ahead above 1 (ba_ss_set_lookahead, ba_ss_draw_next: the
 *           snapshots do not carry the weights) are refused.  A drawn weight that is not finite
 *           and positive stops the chain with status 13 (BA_E_INVALID).                     2
 *   kind 9  ArStateModel with an ArSpikeSlabSampler (bsts AddAutoAr; Models/TimeSeries/
 *           PosteriorSamplers/ArSpikeSlabSampler.cpp): an autoregression (kind 4's state and
 *           transition) whose coefficients have a spike-and-slab prior -- excluded lags are exactly 0.
 *           iparams = {lags <= 16, truncate (accept stationary draws only), max_flips (<= 0: no
 *           limit), allow_model_selection}.  initial_phi holds 3 lags + lags^2 numbers: the initial
 *           coefficients (stationary when truncate is on), the slab's mean, the prior inclusion
 *           probabilities in [0, 1], the slab's precision (lags x lags, column-major, symmetric
 *           positive definite).  The model starts with every lag included.  Takes one of the 4
 *           autoregression slots and is a member of the autoregression family: its sampler
 *           (indicators: the shuffle's random_int, one uniform per flip; up to 100 coefficient
 *           proposals of n normals each, then draw_phi_univariate; the sigma draw) reads the
 *           family's sampler id in sequence.  ba_ss_get_state_model / ba_ss_get_ar / ba_ss_forecast /
 *           ba_ss_prediction_errors serve it as they serve kind 4; ba_ss_get_ar_inclusion gives the
 *           indicators.  Refused: the Student-t / Poisson / logit observation families.  Chain
 *           status 3: no legal configuration; 1: the coefficient draw's precision did not
 *           factor; 14 (BA_E_INVALID): a draw that is not finite.                            1
 *   kind 10 RandomWalkHolidayStateModel (StateModels/RandomWalkHolidayStateModel.cpp, bsts
 *           AddRandomWalkHoliday) + ZeroMeanGaussianConjSampler(ChisqModel(df, sigma_guess)), as
 *           bsts builds it (create_state_model.cpp:891-940).  iparams = {width}, the holiday's
 *           maximum window width, 1 <= width <= 63.  T = I; where the block's calendar says time t
 *           is active at position k(t), the step into t adds N(0, sigma^2) to component k(t) and
 *           Z_t selects component k(t); elsewhere the step adds nothing and Z_t = 0.  observe_state
 *           takes now[k(t)] - then[k(t)] at the active t >= 1.  The initial state is rmvn(mean,
 *           diagonal variance): the variances must be positive.  The calendar comes through
 *           ba_ss_set_holiday_calendar (below); a sweep, ba_ss_impute_state, ba_ss_draw_next and
 *           ba_ss_prediction_errors refuse a list whose holiday has no calendar or one shorter than
 *           the series, ba_ss_forecast one shorter than the series and the horizon.  Refused: the
 *           Student-t / Poisson / logit observation families, a list that also holds kind 8.   width
 * Several kind 10 models may be added, one per holiday, and may be active on the same day.
 *   kind 11 the calendar seasonal: SeasonalStateModelBase whose new_season(t) is read from a
 *           calendar -- MonthlyAnnualCycle (StateModels/SeasonalStateModel.hpp, bsts
 *           AddMonthlyAnnualCycle) is the one of 12 seasons whose seasons start on the first day
 *           of a month -- + ZeroMeanGaussianConjSampler, as bsts builds it.  iparams =
 *           {nseasons}, nseasons >= 2; nseasons - 1 components, Z = e_0.  Kind 3 in everything
 *           (initial state, prior, sigma upper limit, a fixed sigma) but this: the step t -> t + 1
 *           has the seasonal transition and RQR = sigma^2 e_0 e_0' where the block's calendar says
 *           time t + 1 starts a new season, and is the identity without error elsewhere;
 *           observe_state takes now[0] + sum(then) at the t >= 1 that start a season.  The
 *           calendar comes through ba_ss_set_season_calendar (below); a missing or short one is
 *           refused as kind 10's is.  RNG: kind 3's conventions exactly -- one stream-2 normal
 *           per step into a new season, none when sigma = 0; sampler id 7 + 16 per earlier
 *           seasonal model of kind 3 or 11 -- so a regular calendar (t % duration == phase) draws
 *           what kind 3 draws, bit for bit.  Refused: the Student-t / Poisson / logit
 *           observation families, a list that also holds kind 8.                            nseasons
 * With kinds 1 to 11 every Gaussian Add* component of bsts can be added but the regression-holiday
 * and dynamic-regression families (state models with data of their own).
 * iparams is ignored for kinds 1, 2 and 5 (may be NULL).  The var_* arrays hold one entry
 * per variance parameter of the model (two for kinds 2 and 7: level, slope; one otherwise):
 * ChisqModel(df, sigma_guess) prior, sigma upper limit (infinity: none), initial sigma.
 * initial_phi: lags entries, NULL = zeros; must be stationary, as ArModel's constructor
 * demands (ArModel::check_stationary, ArModel.cpp:142-170, decided by the quick bound
 * sum |phi| < 1 and then, where the reference finds polynomial roots, by the equivalent
 * step-down recursion).  initial_state_mean / _variance: the model's components (the
 * variance's diagonal; positive, a local level's may be 0).  Limits: state dimension
 * <= 64, 8 state models, 16 variance parameters, 4 autoregression models.
 * RNG streams: variance parameter v of a model reads the chain's sampler id 1 (level),
 * 6 (slope), 7 (seasonal, kinds 3 and 11: one family), 8 (a random-walk holiday), 13 (trig), 14 (a semilocal slope: NonzeroMeanAr1Sampler) or 12 (ArPosteriorSampler: the proposals' normals, then the
 * sigma draw -- the reference takes the proposals from GlobalRng::rng and the rest from
 * the sampler's generator) + 16 for every earlier model of the same family (local level
 * and local linear trend are one family); the state draw reads stream 2.  A Student local linear
 * trend (kind 8) is in no family: its sampler's four draws read sampler id 160 in sequence, and
 * weight c (0 level, 1 slope) of the step t -> t + 1 in the chain's s-th state draw reads id 161 at
 * slot (s T + t) 2 + c of 256 uniforms (then the slot's spill stream; ba_set_slot_limit applies). */
int ba_ss_clear_state_models(ba_engine *e);
int ba_ss_add_state_model(ba_engine *e, int32_t kind, const int32_t *iparams,
                          const double *var_df, const double *var_sigma_guess,
                          const double *var_sigma_upper_limit,
                          const double *var_initial_sigma, const double *initial_phi,
                          const double *initial_state_mean,
                          const double *initial_state_variance);
/* which kernel draws the state (changes no draw): 0 = the general kernel, one chain per
 * workgroup; (2, four chains per wavefront, was removed in round 5: bit-identical and never
 * faster -- BA_E_INVALID now); 3 = the kernel compiled for the shape [level | trend] [+ seasonal of duration 1]
 * [+ one autoregression] with m <= 16 where the list has that shape; 1 = the default choice.
 * Independently of those: 4 = the local-level model's rounds as separate launches per round
 * (regression sweep, state draw, X'e), 5 = as one persistent launch per call in which every
 * chain loops over the rounds by itself (the default where it applies: a series of at most
 * 2048 steps, models of at most 48 variables).  And: 6 / 7 = the persistent launch's notes of a
 * debugging session (printed to stderr when one of this engine's chains stops) on / off (off
 * by default; the buffer is the engine's own, on its device) */
int ba_ss_set_tuning(ba_engine *e, int32_t kernel);
/* the state dimension and the number of state models of the specification */
int ba_ss_state_dimension(ba_engine *e, int32_t *state_dimension, int32_t *nblocks);
/* state model `block` of one chain: its variance parameters (nvar), the model's
 * sufficient statistics of the last sweep (n, sum of squares per variance) and, for an
 * autoregression model, its coefficients (lags) and the ArModel's sufficient
 * statistics (xtx lags x lags column-major, xty, yty, n).  A semilocal linear trend (kind 7):
 * variances = (level, slope), phi[0..1] = (phi, mu) of the slope's NonzeroMeanAr1Model, ar_xtx
 * [0..5] = its Ar1Suf (sum of squares, sum, cross product of successive values, n, first value,
 * last value; Models/TimeSeries/NonzeroMeanAr1Model.cpp:33-91), ar_n = n; ar_xty / ar_yty are
 * refused.  A Student local linear trend (kind 8): variances = (level, slope), suf_n = T - 1 and
 * suf_ss = sum_t r_t^2 w_old[t] (the WeightedGaussianSuf of the last state draw's residuals with the
 * weights that draw was made with), phi[0..1] = (nu_level, nu_slope).  Any pointer may be NULL */
int ba_ss_get_state_model(ba_engine *e, int64_t chain, int32_t block, double *variances,
                          double *suf_n, double *suf_ss, double *phi, double *ar_xtx,
                          double *ar_xty, double *ar_yty, double *ar_n);
/* one chain's state draw (T x m, step t at [t * m, (t + 1) * m), the models' components
 * in the order the models were added) */
int ba_ss_get_state_draw(ba_engine *e, int64_t chain, double *state);
/* (ba_ss_add_state_model, ba_ss_get_state_model, ba_ss_get_state_draw and ba_ss_get_ar serve the
 * Student-t family, ba_ss_student_*, too) */
/* The template of rounds 2-3, kept: a trend state model -- trend = 1: local level; 2:
 * local linear trend -- plus an optional SeasonalStateModel(nseasons, season_duration =
 * 1); nseasons = 0: none.  Equivalent to ba_ss_add_state_model(trend) [+ (seasonal)].
 * The three-element arrays are indexed level, slope, seasonal (prior df, sigma guess,
 * sigma upper limit, initial sigma of each variance parameter; unused entries are
 * ignored); initial_state_mean / _variance have m = trend + max(nseasons - 1, 0)
 * entries.  RNG streams: 1 level, 6 slope, 7 seasonal, 2 state. */
int ba_ss_set_structural(ba_engine *e, int32_t trend, int32_t nseasons,
                         const double *var_df, const double *var_sigma_guess,
                         const double *var_sigma_upper_limit,
                         const double *var_initial_sigma,
                         const double *initial_state_mean,
                         const double *initial_state_variance);
/* After ba_ss_set_structural: appends ONE ArStateModel(lags) (kind 4 above) to the
 * template; ba_ss_get_ar reads it.  RNG stream 12. */
int ba_ss_add_ar(ba_engine *e, int32_t lags, double prior_df, double sigma_guess,
                 double sigma_upper_limit, double initial_sigma,
                 const double *initial_phi, const double *initial_state_mean,
                 const double *initial_state_variance);
/* one chain's autoregression coefficients (lags), error variance and the ArModel's
 * sufficient statistics of the last sweep (xtx lags x lags column-major, xty, yty,
 * n); any pointer may be NULL */
int ba_ss_get_ar(ba_engine *e, int64_t chain, double *phi, double *sigsq,
                 double *suf_xtx, double *suf_xty, double *suf_yty, double *suf_n);
/* (the template's accessor) one chain's state draw (T x m, step t at [t * m, (t + 1) * m)),
 * the three variance parameters level / slope / seasonal and the state models'
 * sufficient statistics (n, sum of squares) of the last sweep; any pointer may be NULL */
int ba_ss_get_structural(ba_engine *e, int64_t chain, double *state,
                         double *variances, double *suf_n, double *suf_ss);
/* The callers' loop on the bsts path -- for (i in niter) { model->sample_posterior();
 * record the draw } (Interfaces/R/bsts/src/bsts.cc:82-119) -- at the device's rate.
 * ba_ss_set_lookahead(e, L), L > 1: ba_ss_draw_next enqueues the sweep rounds L at a
 * time (the batch after the one being served goes out as soon as serving starts), every
 * round's draw is recorded on the device and handed out one per call: ba_get_state,
 * ba_get_states, ba_logpri, ba_ss_get_state, ba_ss_get_structural, ba_ss_get_state_model,
 * ba_ss_get_state_draw, ba_ss_get_ar and ba_ss_prediction_errors see the draw being served -- gamma, beta, sigma^2
 * and the state models' variances / coefficients of EVERY chain, the state path of the
 * chains named with ba_ss_lookahead_chains (default: chain 0).  Anything else -- a
 * mutator, ba_ss_sweep, a sufficient statistic, the state path of another chain, a
 * forecast -- first puts the chains back where the caller has seen them (the snapshot
 * taken at the batch's start, replayed up to the draw being served: same stream
 * positions, same draws), so the look-ahead is unobservable.  L = 1 (default): one
 * round per call.  ba_sync while a batch is being served waits for THAT batch.
 * What such a rewind costs is bounded: L is the LARGEST batch -- every rewind halves the
 * batches that follow (down to one round per call: no look-ahead), every batch served to its
 * end doubles them again; a chain whose state path was asked for joins the recorded chains
 * (up to 32).  L is cut down to what a 2 GiB record holds. */
int ba_ss_set_lookahead(ba_engine *e, int32_t lookahead);
int ba_ss_lookahead_chains(ba_engine *e, int32_t nchains, const int64_t *chains);
int ba_ss_draw_next(ba_engine *e);
/* nsweeps x StateSpacePosteriorSampler::draw()
 * (StateSpacePosteriorSampler.cpp:42-64) on every chain.  Local level model, a series of
 * at most 2048 steps, models of at most 48 variables: the rounds of the call run as ONE
 * persistent launch per 64 rounds (every chain loops over its rounds by itself; chains
 * meet in tiles of 16 for X'(y - state)); otherwise three launches per round (regression
 * sweep, state draw, X'(y - state)).  The same draws either way: ba_ss_set_tuning(e, 4 | 5).
 * The state draw's standard normals (RNG stream 2) are Box-Muller pairs on per-draw
 * substreams -- draws 2 j and 2 j + 1 of a chain are R cos(2 pi u2), R sin(2 pi u2) of the two
 * uniforms at stream position 512 j, R = sqrt(-2 log(1 - u1)) --, not the reference's
 * sequential Kinderman-Ramage normals.  A same-seed comparison with BOOM can therefore show
 * the same posterior (within Monte Carlo error) and cannot show the same draws, state paths or
 * stream positions, for any seed.  The link is carried by tests/test_philox_ref.py (reference
 * of the pairs == the oracle), tests/test_stream_normals_gpu.py and
 * tests/test_stream_views_gpu.py (the device's generator and stream readers against that
 * reference directly) and tests/test_substream_bridge.py (substreams vs sequential vs MT). */
int ba_ss_sweep(ba_engine *e, int32_t nsweeps);
/* one Base::impute_state (StateSpaceModelBase.cpp:278-291) with the current
 * parameters, on every chain */
int ba_ss_impute_state(ba_engine *e);
/* The Student local linear trend (kind 8 above) of the list of state models.
 * ba_ss_trend_get_weights: one chain's weights, T each; entry t scales the state errors of the step
 * t -> t + 1, entry T - 1 is never drawn and stays 1.  ba_ss_trend_set_weights: of one chain or
 * (chain = -1) of all; every entry finite and > 0, else "Weights must be finite and positive.".
 * ba_ss_trend_get_weight_suf: out[0..5] = the GammaSuf (n, sum, sum of logs) of the level weights
 * the last state draw's observe_state drew, then the slope's.  ba_ss_trend_draw_parameters: the
 * model's sample_posterior() alone (sigma_level^2, nu_level, sigma_slope^2, nu_slope on every
 * chain), as ba_ss_impute_state is impute_state alone. */
int ba_ss_trend_get_weights(ba_engine *e, int64_t chain, double *level_w, double *slope_w);
int ba_ss_trend_set_weights(ba_engine *e, int64_t chain, const double *level_w, const double *slope_w);
int ba_ss_trend_get_weight_suf(ba_engine *e, int64_t chain, double *out);
int ba_ss_trend_draw_parameters(ba_engine *e);
/* The spike-and-slab autoregressions (kind 9 above) of the list of state models.
 * ba_ss_autoar_draw_parameters: the ArSpikeSlabSampler::draw() of all such blocks alone, on every
 * chain (as ba_ss_trend_draw_parameters is for kind 8).  ba_ss_get_ar_inclusion: the live inclusion
 * indicators of state model `block` in one chain, `lags` bytes; under a look-ahead the chains are
 * first put back at the draw being served. */
int ba_ss_autoar_draw_parameters(ba_engine *e);
int ba_ss_get_ar_inclusion(ba_engine *e, int64_t chain, int32_t block, uint8_t *gamma);

/* The calendar of a random-walk holiday (state model `block`, kind 10): entry t of `position` is -1
 * (time t is outside the holiday's window) or the position of time t in the window, in [0, width)
 * -- what the reference reads off Holiday::active and days_into_influence_window of time_zero + t.
 * Any other entry is refused with a text.  `count` must cover the series (count >= T); the entries
 * past T serve ba_ss_forecast, which needs count >= T + horizon.  One calendar per block, shared by
 * all chains; a position may recur in a later window (the random walk then continues from its last
 * incidence).  In the state draw the block takes one state-error normal of stream 2 per step,
 * whether the step into it is active or not (an inactive step's is not used).  Under a look-ahead the
 * setter is a mutator like the others.  ba_ss_get_holiday_calendar: *count = the entries set (0: none
 * yet); position may be NULL to ask for the count alone, else it has room for that many. */
int ba_ss_set_holiday_calendar(ba_engine *e, int32_t block, const int32_t *position, int64_t count);
int ba_ss_get_holiday_calendar(ba_engine *e, int32_t block, int32_t *position, int64_t *count);

/* The calendar of a calendar seasonal (state model `block`, kind 11): entry t of `new_season` is 1
 * where time t starts a new season, else 0; any other value is refused with a text.  Entry 0 is
 * accepted and never read (no step leads into time 0).  `count` must cover the series (count >= T)
 * for a sweep, ba_ss_impute_state, ba_ss_draw_next and ba_ss_prediction_errors; ba_ss_forecast needs
 * count >= T + horizon: forecast step i uses the transition of time T - 2 + i, that is entry
 * T - 1 + i.  One calendar per block, shared by all chains.  Under a look-ahead the setter is a
 * mutator like the others.  The getter is shaped like ba_ss_get_holiday_calendar.  Neither pair
 * accepts a block of the other kind.
 * ba_monthly_cycle_calendar fills MonthlyAnnualCycle's calendar: out[t] = 1 where the day t days
 * after the date (year, month, day) of the first observation is the first day of a month, in the
 * proleptic Gregorian calendar; a date that does not exist is refused.  Host only: it needs no
 * engine and no device. */
int ba_ss_set_season_calendar(ba_engine *e, int32_t block, const uint8_t *new_season, int64_t count);
int ba_ss_get_season_calendar(ba_engine *e, int32_t block, uint8_t *new_season, int64_t *count);
int ba_monthly_cycle_calendar(int32_t year, int32_t month, int32_t day, int64_t count, uint8_t *out);

/* DynamicRegressionStateModel(X) + DynamicRegressionIndependentPosteriorSampler (one ChisqModel(df,
 * sigma_guess) and sigma upper limit per coefficient), bsts AddDynamicRegression with
 * DynamicRegressionRandomWalkOptions (StateModels/DynamicRegressionStateModel.cpp,
 * create_state_model.cpp:1245-1287).  predictors: rows x xdim, row-major, row t = x_t; finite.
 * A block of xdim coefficients: T = I, RQR = diag(sigma_1^2 .. sigma_xdim^2), Z_t = x_t;
 * observe_state adds (now[i] - then[i])^2 per coefficient, n = T - 1 each.  The block cannot exist
 * without its data, so it has a call of its own instead of a kind of ba_ss_add_state_model (kind 12
 * there is refused as any unknown kind); the call appends to the list exactly as
 * ba_ss_add_state_model does, and the first one after ba_ss_clear_state_models starts a new list.
 * The var_* arrays, initial_state_mean and initial_state_variance hold xdim entries each; an initial
 * sigma may be 0, the initial state is rmvn(mean, diagonal variance): the variances must be positive.
 * Limits: 1 <= xdim, state dimension <= 64, 16 variance parameters in the list (the block takes xdim).
 * rows >= T is needed by a sweep, ba_ss_impute_state, ba_ss_draw_next and ba_ss_prediction_errors,
 * rows >= T + horizon by ba_ss_forecast (the reference's add_forecast_data): each refuses with a text
 * when the rows are too few.  ba_ss_set_dynamic_predictors replaces the block's predictors (or extends
 * them with the forecast's rows); under a look-ahead it is a mutator like the others.
 * ba_ss_get_dynamic_predictors: *rows = the rows set; predictors may be NULL to ask for the count
 * alone, else it has room for rows x xdim doubles.  ba_ss_get_state_model reports the block's xdim
 * variances and sufficient statistics (arrays of xdim); ba_ss_get_state_draw and
 * ba_ss_state_dimension serve it unchanged.
 * RNG streams (a convention of this library; BOOM draws the d variances from one generator):
 * variance slot i of the block reads the chain's sampler id 10 + 16 x (the dynamic coefficients
 * earlier in the list, those of this block included); at most 16 slots, so at most 250.  In the
 * state draw the block takes xdim stream-2 normals for the initial state and xdim per step, whatever
 * the sigmas.  Refused with a text, in either order of the calls: the Student-t / Poisson / logit
 * observation families; a list that also holds a Student local linear trend (kind 8), a random-walk
 * holiday (kind 10) or a calendar seasonal (kind 11).  The AR form is ba_ss_add_dynamic_regression_ar
 * below.  Not built: the hierarchical form (bsts does not reach it either). */
int ba_ss_add_dynamic_regression(ba_engine *e, int32_t xdim, const double *predictors, int64_t rows,
                                 const double *var_df, const double *var_sigma_guess,
                                 const double *var_sigma_upper_limit, const double *var_initial_sigma,
                                 const double *initial_state_mean, const double *initial_state_variance);
/* DynamicRegressionArStateModel(X, lags) + DynamicRegressionArPosteriorSampler, bsts AddDynamicRegression
 * with DynamicRegressionArOptions(lags) (StateModels/DynamicRegressionArStateModel.cpp,
 * PosteriorSamplers/DynamicRegressionArPosteriorSampler.cpp): every coefficient follows an autoregression
 * of `lags` lags, beta_{t+1,i} = phi_i' (beta_{t,i}, .., beta_{t-lags+1,i}) + N(0, sigma_i^2), and
 * Z_t = x_{t,i} at coefficient i's current value, 0 at its lags.  The call appends xdim consecutive state
 * models, one per coefficient, each of dimension `lags` and each in everything but its observation row
 * an autoregression (kind 4): ArModel statistics add_mixture_data(now[0], then, 1), ArPosteriorSampler's
 * draw (draw_phi with 3 multivariate proposals and the univariate fallback, then draw_sigma), the
 * initial state StateModelBase::simulate_initial_state's.  *first_block_out (may be NULL) = the index
 * of the model's first block; block first + i is coefficient i.  All xdim blocks are appended, or none.
 * predictors: rows x xdim row-major, finite.  var_df, var_sigma_guess, var_sigma_upper_limit,
 * var_initial_sigma: xdim entries (an initial sigma must be positive, as kind 4's).  initial_phi: xdim x lags row-major, every row stationary (NULL: zeros).
 * initial_state_mean, initial_state_variance: xdim x lags (bsts: 0 and 1); variances positive.
 * Limits: 1 <= lags <= 16, 1 <= xdim, and those of the list: 4 autoregression slots (each coefficient
 * takes one, so xdim <= 4 less the list's other autoregressions and semilocal trends), 8 state models,
 * state dimension 64, 16 variance parameters.
 * ba_ss_set_dynamic_predictors / ba_ss_get_dynamic_predictors on the model's FIRST block set and return
 * all xdim columns (rows x xdim); on another block of the model they refuse with a text.
 * ba_ss_get_state_model, ba_ss_get_state_draw and ba_ss_state_dimension serve each block as they serve
 * kind 4 (phi, the ArModel statistics, one variance).  Rows needed: as for ba_ss_add_dynamic_regression.
 * RNG: block by block the AR family's sampler id (12 + 16 per earlier autoregression of the list), read
 * in sequence as kind 4 reads it; in the state draw each block takes `lags` stream-2 normals for the
 * initial state and one per step.  Refusals as for ba_ss_add_dynamic_regression, in either order of the
 * calls; a plain dynamic regression in the same list is allowed (they share the predictor table by
 * column).  The look-ahead, ba_ss_forecast and ba_ss_prediction_errors serve the model. */
int ba_ss_add_dynamic_regression_ar(ba_engine *e, int32_t xdim, int32_t lags, const double *predictors, int64_t rows,
                                    const double *var_df, const double *var_sigma_guess,
                                    const double *var_sigma_upper_limit, const double *var_initial_sigma,
                                    const double *initial_phi, const double *initial_state_mean,
                                    const double *initial_state_variance, int32_t *first_block_out);
int ba_ss_set_dynamic_predictors(ba_engine *e, int32_t block, const double *predictors, int64_t rows);
int ba_ss_get_dynamic_predictors(ba_engine *e, int32_t block, double *predictors, int64_t *rows);

/* RegressionHolidayStateModel with its own sample_posterior (the scalar model's), bsts
 * AddRegressionHoliday (StateModels/RegressionHolidayStateModel.cpp, create_state_model.cpp:952-986).
 * A model holds nholidays holidays; holiday h has a window of widths[h] >= 1 days and one coefficient
 * per day of it, shared across the years, all under the one prior N(prior_mean, prior_sd^2) (prior_sd
 * positive and finite).  initial_coefficients: sum of the widths, holiday by holiday (NULL: zeros).
 * *model_out (may be NULL) = the model's index among the list's regression holiday models.
 * The model's state is the constant 1 with variance 0 and its Z_t is the coefficient active at t: on
 * the device it is an offset on the observation series, not a block.  ba_ss_state_dimension,
 * ba_ss_get_state_draw and ba_ss_get_state_model do not count it (the reference's state vector
 * carries a trailing constant 1 per model; bsts's "state contribution" of the model at time t is
 * coefficient[index(t)], which the caller forms from ba_ss_get_regression_holiday and the calendar).
 * The models belong to the list of state models -- at least one state model has to be there first --
 * and are dropped with it (ba_ss_clear_state_models, ba_ss_set_structural).  Limits: 4 models and 256
 * coefficients per list.  Allowed beside every Gaussian state model.
 * ba_ss_set_regression_holiday_calendar: entry t is -1 (no holiday of the model is active at time t)
 * or the flat index offset_h + day in [0, sum of the widths) of the coefficient that is -- the caller
 * flattens (holiday, day), as it turns dates into positions for kind 10; one entry per time, so one
 * holiday of a model is active at a time by construction (two models may coincide).  count >= T is
 * needed by a sweep, ba_ss_impute_state, ba_ss_draw_next and ba_ss_prediction_errors, count >= T +
 * horizon by ba_ss_forecast, which adds the coefficient active at T + i: (obs + pred) + effect, model
 * by model.  Each refuses with a text when the entries are too few.  The setter is a mutator like the
 * others; the getter is shaped like ba_ss_get_holiday_calendar.
 * A round (ba_ss_sweep) draws the observation model, then every coefficient in (model, coefficient)
 * order -- precision = count / sigma^2 + 1 / prior_sd^2, mean = (total / sigma^2 + prior_mean /
 * prior_sd^2) / precision, rnorm(mean, sqrt(1 / precision)) with the sigma^2 just drawn --, then the
 * state, whose observe_state leaves total = the sum over the coefficient's observed steps of (y_t -
 * x_t'beta) - Z_t'alpha_t + coefficient and count = those steps (the same for every chain; 0: the
 * prior's draw).  Before the first state draw the totals are empty.
 * ba_ss_get_regression_holiday: one chain's coefficients, totals and the counts of a model (sum of the
 * widths each; any may be NULL).  ba_ss_set_regression_holiday: the coefficients of one chain, or of
 * every chain (chain = -1); a mutator.
 * RNG stream (a convention of this library; BOOM draws from the model's own generator): the chain's
 * sampler id 162, one position per chain for all its models.
 * Refused with a text, in either order of the calls: the Student-t / Poisson / logit observation
 * families; a look-ahead above 1 (the record does not carry the coefficients).  Not built: the
 * dynamic-intercept variant, ba_group_* forwarding (the hierarchical model: below). */
int ba_ss_add_regression_holiday(ba_engine *e, int32_t nholidays, const int32_t *widths, double prior_mean,
                                 double prior_sd, const double *initial_coefficients, int32_t *model_out);
int ba_ss_set_regression_holiday_calendar(ba_engine *e, int32_t model, const int32_t *index, int64_t count);
int ba_ss_get_regression_holiday_calendar(ba_engine *e, int32_t model, int32_t *index, int64_t *count);
int ba_ss_get_regression_holiday(ba_engine *e, int64_t chain, int32_t model, double *coefficients, double *totals,
                                 double *counts);
int ba_ss_set_regression_holiday(ba_engine *e, int64_t chain, int32_t model, const double *coefficients);

/* HierarchicalRegressionHolidayStateModel (bsts AddHierarchicalRegressionHoliday) with its sampler,
 * HierGaussianRegressionAsisSampler: a regression holiday model whose nholidays holidays share one window
 * width d <= 16 and whose coefficient vectors share the prior beta_h ~ N(mu, Omega^-1), with
 * mu ~ N(mean_prior_mean, mean_prior_variance) (d and d x d, row-major) and Omega ~ Wishart(
 * variance_guess_weight, variance_guess_weight x variance_guess).  bsts passes no residual-variance prior:
 * sigma^2 is the observation model's.  The model takes one of the list's four regression holiday slots and
 * its nholidays x d coefficients count towards the 256; its calendar, coefficients, totals and counts go
 * through the calls above (flat index h d + day).  Every chain starts at mu = 0 and Omega = I, the
 * reference's MvnModel(d).  *model_out: its index among the list's regression holiday models.
 * Refused with a text beyond the plain model's refusals: d > 16; a weight not above d - 1; a
 * mean_prior_variance or variance_guess that is not symmetric positive definite; entries not finite.
 * ba_ss_get_ / ba_ss_set_hierarchical_regression_holiday: one chain's mu (d) and Omega (d x d, row-major;
 * either may be NULL in the getter); the setter takes chain = -1 for every chain, is a mutator and refuses
 * an Omega that is not symmetric positive definite.
 * RNG stream (a convention of this library; BOOM draws from the sampler's generator and, for the first
 * draw of mu, the global one): the chain's sampler id 163, one position per chain for all its hierarchical
 * models, in (model, step) order.  A draw with a factor that is not positive definite or a result that is
 * not finite stops the chain (status 16) and leaves its coefficients, mu, Omega and position as they were.
 * Departures from BOOM, all in DESIGN 3.26: totals and counts are the plain model's (missing days are
 * skipped, time 0 is observed); the centred draw's xtx is formed from the current counts every time. */
int ba_ss_add_hierarchical_regression_holiday(ba_engine *e, int32_t nholidays, int32_t width,
                                              const double *mean_prior_mean, const double *mean_prior_variance,
                                              const double *variance_guess, double variance_guess_weight,
                                              const double *initial_coefficients, int32_t *model_out);
int ba_ss_get_hierarchical_regression_holiday(ba_engine *e, int64_t chain, int32_t model, double *mean, double *precision);
int ba_ss_set_hierarchical_regression_holiday(ba_engine *e, int64_t chain, int32_t model, const double *mean,
                                              const double *precision);

/* ---- bsts(family = "student"): StateSpaceStudentRegressionModel with
 * StateSpaceStudentPosteriorSampler (Models/StateSpace/StateSpaceStudentRegressionModel.cpp,
 * PosteriorSamplers/StateSpaceStudentPosteriorSampler.cpp:56-126) ----------------------------
 * One observation per time step.  The observation model is TRegressionSpikeSlabSampler with its
 * latent data fixed (the kernels of ba_student_sweep on the response y_t - Z_t'alpha_t over the
 * observed steps); the state draw is the general structural kernel with the per-step observation
 * variance H_t = sigma^2 / w_t (sigma^2 nu / (nu - 2), or 1e8 sigma^2 for nu <= 2, where a step
 * is missing or its weight is 0).
 *   ba_ss_student_set_data   as ba_ss_set_data; starts a new model (nu = 30, all weights 1, no
 *                            state draw yet)
 *   state models             ba_ss_add_state_model (a plain local level is the one-block list;
 *                            after ba_ss_set_local_level alone the family is refused); the general
 *                            kernel always, whatever ba_ss_set_tuning says
 *   priors                   ba_sss_set_slab(mu, precision, 1, max_flips), ba_set_spike,
 *                            ba_set_sigma_prior, ba_student_set_nu_prior, ba_student_set_nu
 *   ba_ss_student_sweep      nsweeps x StateSpacePosteriorSampler::draw (StateSpacePosteriorSampler.cpp:
 *                            41-63): indicators and beta given sigma^2, sigma^2, nu, the state models'
 *                            parameters, the weights, the state.  A sampler that has drawn no state yet
 *                            first draws it with the weights in hand (1 unless set) and imputes the
 *                            weights once, as the reference's first draw() does.
 *   ba_ss_student_impute_state   one impute_state with the current parameters and weights
 *   ba_ss_student_get_weights / _set_weights   one chain's T weights (set: chain -1 = every chain;
 *                            AugmentedStudentRegressionData::set_weight: "Weights must be finite and
 *                            non-negative."; a missing step's weight is not read).  After _set_weights
 *                            the next sweep starts with an impute_state on the new weights.
 *   ba_ss_student_forecast   simulate_forecast (StateSpaceStudentRegressionModel.cpp:205-251): newX and
 *                            out as in ba_ss_forecast; step i is rstudent_mt(Z'state + x_i'beta, sigma,
 *                            nu) after the state errors of the step, the reference's draws on the
 *                            chain's forecast stream (id 5), which goes on from call to call
 * Also served for this kind: ba_set_state / ba_get_state(s), ba_enable_draws with ba_get_draws and
 * ba_student_get_nu_draws, ba_student_get_nu / _get_margin / _allow_model_selection,
 * ba_ss_get_state_draw, ba_ss_get_state_model, ba_ss_get_ar, ba_ss_state_dimension.  Not served:
 * ba_ss_forecast (use ba_ss_student_forecast), ba_ss_draw_next, ba_ss_sweep, ba_ss_impute_state
 * (refused).
 * RNG: stream 3 indicators / beta; stream 15 from position r * 4096 for sigma^2, then nu, of round
 * r; stream 31 from position (s T + t) * 256 for the weight of step t in the sampler's s-th
 * weight imputation (the first draw() makes two); stream 2 the state; the state models' streams
 * as on the Gaussian path. */
int ba_ss_student_set_data(ba_engine *e, int32_t T, int32_t p, const double *y,
                           const double *X, const uint8_t *observed);
int ba_ss_student_sweep(ba_engine *e, int32_t nsweeps);
int ba_ss_student_get_weights(ba_engine *e, int64_t chain, double *w);
int ba_ss_student_set_weights(ba_engine *e, int64_t chain, const double *w);
int ba_ss_student_impute_state(ba_engine *e);
int ba_ss_student_forecast(ba_engine *e, int32_t horizon, const double *newX, double *out);

/* ---- bsts(family = "poisson"): StateSpacePoissonModel with StateSpacePoissonPosteriorSampler
 * (Models/StateSpace/StateSpacePoissonModel.cpp, PosteriorSamplers/
 * StateSpacePoissonPosteriorSampler.cpp:79-147) ---------------------------------------------------
 * One observation per time step, regression present.  An observed step carries a latent value v_t
 * and a precision q_t (0 and 1 in a new model); the filter sees v_t - x_t'beta with the observation
 * variance H_t = 1 / q_t, pi^2 / 6 where the step is missing.  The observation model is
 * PoissonRegressionSpikeSlabSampler with its latent data fixed (the sweep of ba_poisson_sweep at
 * sigma^2 = 1 on the response v_t - Z_t'alpha_t with weight q_t over the observed steps); the
 * imputation is PoissonDataImputer::impute at eta_t = Z_t'alpha_t + x_t'beta, its two points
 * combined the external one first; the state draw is the general structural kernel on every
 * chain's own series.
 *   ba_ss_poisson_set_data   counts, exposures, X (T x p column-major), observed (NULL: all); counts
 *                            must be non-negative integers and exposures positive at the observed
 *                            steps (a missing step's are never read).  Starts a new model (v = 0,
 *                            q = 1, no state draw yet).  The mixtures: ba_poisson_set_mixtures, after
 *                            this call (a sweep without them is refused)
 *   state models             ba_ss_add_state_model (a plain local level is the one-block list;
 *                            after ba_ss_set_local_level alone the family is refused); the general
 *                            kernel always, whatever ba_ss_set_tuning says
 *   priors                   ba_sss_set_slab(mu, precision, 0, max_flips) -- a fixed-precision slab --,
 *                            ba_set_spike.  There is no sigma^2 (it is 1) and no nu
 *   ba_ss_poisson_sweep      nsweeps x StateSpacePosteriorSampler::draw (StateSpacePosteriorSampler.cpp:
 *                            42-64): indicators and beta, the state models' parameters, the latent
 *                            data, the state.  A sampler that has drawn no state yet first draws it
 *                            with the latent data in hand and uses up one imputation's random numbers,
 *                            as the reference's first draw() does (its values are all overwritten
 *                            before they are read)
 *   ba_ss_poisson_impute_state   one impute_state with the current parameters and latent data
 *   ba_ss_poisson_get_latent / _set_latent   one chain's T values and precisions (set: chain -1 =
 *                            every chain; a missing step's entries are not read; a negative precision:
 *                            "precision must be non-negative."; a zero or non-finite precision at an
 *                            observed step is refused too -- the reference's variance is -infinity
 *                            there).  After _set_latent the next sweep starts with an impute_state on
 *                            the new data.
 *   ba_ss_poisson_forecast   simulate_forecast (StateSpacePoissonModel.cpp:215-242): newX and out as in
 *                            ba_ss_forecast, exposure `horizon` non-negative finite numbers (NULL:
 *                            ones); step i is a Poisson(exposure_i exp(Z'state + x_i'beta)) count after
 *                            the state errors of the step, on the chain's forecast stream (id 5), which
 *                            goes on from call to call.  The state errors are the reference's draws; the
 *                            count is an exact Poisson draw (inversion below a mean of 10, Hoermann's
 *                            PTRS above: device_rng_counts.h), not the number Bmath's rpois makes of the
 *                            stream.  A cell whose mean overflows is NaN
 * Also served for this kind: ba_set_state / ba_get_state(s), ba_enable_draws with ba_get_draws, the
 * summaries, ba_ss_get_state_draw, ba_ss_get_state_model, ba_ss_get_ar, ba_ss_state_dimension,
 * ba_set_slot_limit.  Not served: ba_ss_forecast (use ba_ss_poisson_forecast), ba_ss_draw_next,
 * ba_ss_sweep, ba_ss_impute_state, ba_poisson_sweep, ba_ss_student_* (refused).
 * RNG: stream 3 indicators / beta; stream 11 from position (s T + t) * 256 for step t in the
 * sampler's s-th imputation (the first draw() makes two: round r of a fresh sampler imputes with
 * s = r + 1); stream 2 the state; the state models' streams as on the Gaussian path. */
int ba_ss_poisson_set_data(ba_engine *e, int32_t T, int32_t p, const double *counts,
                           const double *exposure, const double *X, const uint8_t *observed);
int ba_ss_poisson_sweep(ba_engine *e, int32_t nsweeps);
int ba_ss_poisson_impute_state(ba_engine *e);
int ba_ss_poisson_get_latent(ba_engine *e, int64_t chain, double *value, double *precision);
int ba_ss_poisson_set_latent(ba_engine *e, int64_t chain, const double *value, const double *precision);
int ba_ss_poisson_forecast(ba_engine *e, int32_t horizon, const double *newX, const double *exposure,
                           double *out);

/* ---- bsts(family = "logit"): StateSpaceLogitModel with StateSpaceLogitPosteriorSampler
 * (Models/StateSpace/StateSpaceLogitModel.cpp, PosteriorSamplers/
 * StateSpaceLogitPosteriorSampler.cpp:49-123) ------------------------------------------------------
 * One observation per time step, regression present.  An observed step carries successes y_t, trials
 * n_t, a latent value v_t and a precision q_t (0 and 4 / n_t in a new model); the filter sees
 * v_t - x_t'beta with the observation variance H_t = 1 / q_t, pi^2 / 3 (the variance of the standard
 * logistic distribution) where the step is missing.  The observation model is
 * BinomialLogitSpikeSlabSampler with its latent data fixed (the sweep of ba_logit_sweep at
 * sigma^2 = 1 on the response v_t - Z_t'alpha_t with weight q_t over the observed steps); the
 * imputation is BinomialLogitCltDataImputer::impute(n_t, y_t, eta_t) at eta_t = Z_t'alpha_t +
 * x_t'beta (two uniforms per trial up to clt_threshold trials, the large-sample branch above), then
 * v_t = sum / information, q_t = information; the state draw is the general structural kernel on
 * every chain's own series.  There is no Polya-Gamma imputer in this sampler.
 *   ba_ss_logit_set_data     successes, trials, X (T x p column-major), observed (NULL: all),
 *                            clt_threshold (1 .. 64, as in ba_logit_set_data).  At the observed steps
 *                            trials must be integers of at least 1 and successes integers in
 *                            0 .. n_t (a missing step's are never read).  The reference accepts
 *                            n_t = 0 at an observed step and then filters with a latent value that is
 *                            not a number; here it is refused.  Starts a new model (v = 0,
 *                            q = 4 / n_t, no state draw yet)
 *   state models             ba_ss_add_state_model (a plain local level is the one-block list;
 *                            after ba_ss_set_local_level alone the family is refused); the general
 *                            kernel always, whatever ba_ss_set_tuning says
 *   priors                   ba_sss_set_slab(mu, precision, 0, max_flips) -- a fixed-precision slab --,
 *                            ba_set_spike.  There is no sigma^2 (it is 1)
 *   ba_ss_logit_sweep        nsweeps x StateSpacePosteriorSampler::draw (StateSpacePosteriorSampler.cpp:
 *                            42-64): indicators and beta, the state models' parameters, the latent
 *                            data, the state.  A sampler that has drawn no state yet first draws it
 *                            with the latent data in hand and uses up one imputation's random numbers,
 *                            as the reference's first draw() does (its values are all overwritten
 *                            before they are read)
 *   ba_ss_logit_impute_state   one impute_state with the current parameters and latent data
 *   ba_ss_logit_get_latent / _set_latent   one chain's T values and precisions (set: chain -1 =
 *                            every chain; a missing step's entries are not read; a negative precision:
 *                            "precision must be non-negative."; a zero or non-finite precision at an
 *                            observed step is refused too).  After _set_latent the next sweep starts
 *                            with an impute_state on the new data.
 *   ba_ss_logit_forecast     simulate_forecast (StateSpaceLogitModel.cpp:221-248): newX and out as in
 *                            ba_ss_forecast, trials `horizon` non-negative finite numbers, rounded to
 *                            the nearest integer as the reference's lround does (NULL: ones); step i is
 *                            a Binomial(trials_i, plogis(Z'state + x_i'beta)) count after the state
 *                            errors of the step, on the chain's forecast stream (id 5), which goes on
 *                            from call to call.  The state errors are the reference's draws; the count
 *                            is an exact binomial draw (inversion below n min(p, 1 - p) = 10, Hoermann's
 *                            BTRS above: device_rng_counts.h), not the number Bmath's rbinom makes of
 *                            the stream
 * Also served for this kind: ba_set_state / ba_get_state(s), ba_enable_draws with ba_get_draws, the
 * summaries, ba_ss_get_state_draw, ba_ss_get_state_model, ba_ss_get_ar, ba_ss_state_dimension,
 * ba_set_slot_limit.  Not served: ba_ss_forecast (use ba_ss_logit_forecast), ba_ss_draw_next,
 * ba_ss_sweep, ba_ss_impute_state, ba_logit_sweep, ba_logit_set_imputer, ba_ss_student_*,
 * ba_ss_poisson_* (refused).
 * RNG: stream 3 indicators / beta; stream 9 from position (s T + t) * 256 for step t in the
 * sampler's s-th imputation (the first draw() makes two: round r of a fresh sampler imputes with
 * s = r + 1); stream 2 the state; the state models' streams as on the Gaussian path. */
int ba_ss_logit_set_data(ba_engine *e, int32_t T, int32_t p, const double *successes, const double *trials,
                         const double *X, const uint8_t *observed, int32_t clt_threshold);
int ba_ss_logit_sweep(ba_engine *e, int32_t nsweeps);
int ba_ss_logit_impute_state(ba_engine *e);
int ba_ss_logit_get_latent(ba_engine *e, int64_t chain, double *value, double *precision);
int ba_ss_logit_set_latent(ba_engine *e, int64_t chain, const double *value, const double *precision);
int ba_ss_logit_forecast(ba_engine *e, int32_t horizon, const double *newX, const double *trials,
                         double *out);
/* StateSpaceRegressionModel::simulate_forecast(rng, newX, final_state)
 * (StateSpaceRegressionModel.cpp:214-219, :256-278; what bsts' predict does for
 * every saved draw): one draw from the predictive distribution of the next
 * `horizon` observations for EVERY chain's current parameters and final state.
 * newX is horizon x p column-major (host); out is chains x horizon (host),
 * row-major.  Each call continues the chains' forecast streams.  Works for the
 * local level model and for every list of state models, with Gaussian observation
 * noise.  The Student-t, Poisson and logit families are refused here: their forecasts
 * are ba_ss_student_forecast, ba_ss_poisson_forecast and ba_ss_logit_forecast. */
int ba_ss_forecast(ba_engine *e, int32_t horizon, const double *newX, double *out);
/* bsts's one.step.prediction.errors and log.likelihood: ScalarStateSpaceModelBase::
 * one_step_prediction_errors (StateSpaceModelBase.cpp:682-691) and the filter's log likelihood
 * for chains [chain_first, chain_first + chain_count) -- a plain Kalman filter
 * (ScalarMarginalDistribution::update, ScalarKalmanFilter.cpp:41-83) over the series at exactly
 * the parameters the accessors report at that moment (ba_get_state, ba_ss_get_state_model,
 * ba_ss_get_state / ba_ss_get_structural, ba_ss_trend_get_weights: a Student local linear trend
 * is filtered with its per-step variances sigma_c^2 / w_c[t]).  errors: v_t = y_t - x_t'beta -
 * Z'a_t, 0 at a missing step (standardize != 0: v_t / sqrt(F_t)); variances: F_t; both
 * chain_count x T, a chain's T values together; log_likelihood: chain_count, the sum over the
 * observed steps of log N(v_t; 0, F_t).  Any of the three may be NULL, not all.  Valid before
 * any sweep (the initial values).  An observer: no stream position, state path, sufficient
 * statistic or snapshot changes, and a look-ahead is neither settled nor shortened.  A chain
 * whose forecast variance is not positive and finite at some step gets NaN from that step on
 * and the call returns BA_E_FORECAST_VARIANCE ("Found a zero (or negative) forecast
 * variance!", the chain's index); the chain itself and its status are unchanged.  Gaussian
 * observation model only: the Student-t, Poisson and logit families return BA_E_STATE ("one-step
 * prediction errors are built for the Gaussian observation model only").  A stopped chain is
 * reported as by ba_ss_forecast. */
int ba_ss_prediction_errors(ba_engine *e, int64_t chain_first, int64_t chain_count, int32_t standardize,
                            double *errors, double *variances, double *log_likelihood);
/* bsts.prediction.errors(model, cutpoints = ...): StateSpaceRegressionModel::
 * one_step_holdout_prediction_errors(newX, newY, final_state, standardize)
 * (StateSpaceRegressionModel.cpp:280-305; StateSpaceModel's twin is the call with p = 0) for chains
 * [chain_first, chain_first + chain_count): the one-step prediction errors of `horizon` holdout rows that
 * follow the engine's series, at the parameters ba_ss_prediction_errors would read live at that moment
 * and from the chain's drawn final state alpha (time T - 1, what ba_ss_forecast starts from).  The filter
 * starts at a = T_{T-1} alpha, P = RQR_{T-1} and runs on the time indices T .. T + horizon - 1 with no
 * missing step: v_i = newY_i - newX_i'beta - Z_{T+i}'a, F_i = Z_{T+i}'P Z_{T+i} + sigma^2, then the update
 * and the transition as ba_ss_prediction_errors does them.  A seasonal's phase is counted on from T; a
 * holiday's or calendar seasonal's calendar and a dynamic regression's predictors are read at T ..
 * T + horizon - 1, the rows ba_ss_forecast(horizon) needs (the same refusals when they are too few).
 * newX: horizon x p column-major, as ba_ss_forecast's (NULL where p = 0); newY: horizon finite numbers;
 * errors (v_i; standardize != 0: v_i / sqrt(F_i)) and variances (F_i; may be NULL): chain_count x horizon,
 * a chain's values together; all on the host.  bsts calls it after every draw on the series cut at the
 * cutpoint and appends the result to ba_ss_prediction_errors' in-sample errors.  It needs a state draw
 * (BA_E_STATE "no state draw yet ..." as ba_ss_forecast), settles a look-ahead to the draw being served as
 * ba_ss_forecast does, and is an observer otherwise: no stream position, state path, sufficient statistic,
 * status or snapshot changes.  A forecast variance that is not positive and finite: as
 * ba_ss_prediction_errors (NaN from that step on, BA_E_FORECAST_VARIANCE with the chain's index).
 * Refused with BA_E_STATE: the Student-t, Poisson and logit families ("holdout prediction errors are built
 * for the Gaussian observation model only"); a list with a Student local linear trend (the reference's
 * method reads the trend's weights past the end of the series: nothing defined to reproduce); a list with
 * regression holiday models, plain or hierarchical (not built).  BA_E_INVALID: horizon <= 0, a null newY or
 * errors, a null newX with p > 0, a newY entry that is not finite, a chain range out of bounds. */
int ba_ss_holdout_prediction_errors(ba_engine *e, int64_t chain_first, int64_t chain_count, int32_t standardize,
                                    int32_t horizon, const double *newX, const double *newY, double *errors,
                                    double *variances);
/* state(): T doubles of one chain; level sigsq; level suf (n, sumsq) */
int ba_ss_get_state(ba_engine *e, int64_t chain, double *state,
                    double *level_sigsq, double *level_n, double *level_sumsq);
int ba_ss_set_level_sigsq(ba_engine *e, int64_t chain, double sigsq);
/* per-chain regression sufficient statistics left by impute_state */
int ba_ss_get_chain_suf(ba_engine *e, int64_t chain, double *xty, double *yty,
                        double *n);

/* ---- several devices behind one handle (north-star: "C++ host code ...
 * chains shard across the GPUs of one node with a single RCCL gather") --------------
 * A group is one engine per entry of `devices` in ONE process: engine i lives on HIP
 * device devices[i] with its own stream and owns the global chains
 * [i * chains_per_device, (i + 1) * chains_per_device), so a chain's draws do not
 * depend on the device that runs it.  Nothing on the sampling path crosses devices;
 * the two collectives go through librccl directly (loaded on demand; xGMI between the
 * devices of a node): ba_group_build_suf_from_xy = rows of X sharded over the devices,
 * local f64-MFMA syrk, ONE ncclAllReduce of (X'X | X'y | y'y, sum y | sum x), every
 * engine installs the bitwise identical total; ba_group_get_summaries = ONE
 * ncclAllGather of the per-device summary blocks, summed on the host.  A device list
 * that repeats ONE device is allowed (no collective: blocks are summed on the device);
 * a mixed list is not.  Everything that is per engine (priors beyond the common ones
 * below, options, state accessors, look-ahead, the other samplers) is reached through
 * ba_group_engine(g, i) with the single-engine entry points; ba_group_locate maps a
 * global chain id to (engine, local chain).  Errors: the BA_E_* codes, message from
 * ba_group_last_error().  New: the reference has no multi-chain or multi-device
 * driver. */
typedef struct ba_group ba_group;
const char *ba_group_last_error(void);
/* 1 when librccl can be loaded and exports what a multi-device group calls */
int32_t ba_group_rccl_available(void);
int ba_group_create(const int32_t *devices, int32_t ndevices, int32_t chains_per_device,
                    uint64_t seed, ba_group **out);
void ba_group_destroy(ba_group *g);
int32_t ba_group_size(const ba_group *g);
ba_engine *ba_group_engine(ba_group *g, int32_t i);
int ba_group_locate(const ba_group *g, int64_t global_chain, int32_t *engine_index,
                    int64_t *local_chain);
/* NeRegSuf(X, y) for a host matrix (n x p column-major): see above */
int ba_group_build_suf_from_xy(ba_group *g, int64_t n, int32_t p, const double *X,
                               const double *y);
/* ba_set_slab + ba_set_spike + ba_set_sigma_prior on every engine */
int ba_group_set_priors(ba_group *g, const double *prior_mean,
                        const double *unscaled_prior_precision,
                        const double *prior_inclusion_probabilities, int64_t max_model_size,
                        double prior_df, double sigma_guess, double sigma_upper_limit);
/* ba_set_state(e, -1, ...) on every engine */
int ba_group_set_state(ba_group *g, const uint8_t *gamma, const double *beta, double sigsq);
/* ba_sweep on every engine (asynchronous: the devices run side by side); ba_sync */
int ba_group_sweep(ba_group *g, int32_t nsweeps);
/* fn(engine, arg) on every engine of the group, in order; stops at the first error.  What
 * is the same on every device -- the bsts / logit / Poisson data (replicated), priors, the
 * state models, options, the look-ahead -- is set this way with the single-engine entry
 * points; the sweeps of those samplers go out on every device before any is waited for. */
int ba_group_call(ba_group *g, int (*fn)(ba_engine *, void *), void *arg);
int ba_group_ss_sweep(ba_group *g, int32_t nsweeps);
int ba_group_ss_draw_next(ba_group *g);
int ba_group_logit_sweep(ba_group *g, int32_t nsweeps);
int ba_group_poisson_sweep(ba_group *g, int32_t nsweeps);
int ba_group_sync(ba_group *g);
int ba_group_reset_summaries(ba_group *g);
/* whole-job summaries, laid out as ba_get_summaries; blocks (may be NULL) receives the
 * gathered per-device blocks, ba_group_size(g) x (3p + 16) doubles */
int ba_group_get_summaries(ba_group *g, double *inclusion_count, double *beta_sum,
                           double *beta_sumsq, double *scalars, double *blocks);

#ifdef __cplusplus
}
#endif
#endif /* BOOM_AMD_H */
