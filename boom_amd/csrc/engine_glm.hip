// Host side of the latent-data families: BinomialProbit-, BinomialLogit-, PoissonRegression-,
// TRegression- and QuantileRegressionSpikeSlabSampler, and MLVS (multinomial logit).  Each
// imputes its latent data (probit_kernel.hip, student_kernel.hip, quantile_kernel.hip,
// mlogit_kernel.hip) and lets the SpikeSlabSampler sweep -- MLVS: its own variant of it, the
// sweep's mode 3 -- draw indicators and coefficients on the imputed regression; the logit,
// Poisson, Student-t, quantile and multinomial logit samplers keep every chain's own
// V = slab precision + X'WX, built a vector at a time (the column service, xtwx_cols_kernel.hip).
#include "engine_internal.h"
#include "planes_sizing.h"

namespace boom_amd {

// the vectors of V named by cols.req[0, R), in batches the planes can hold
int build_columns(ba_engine *e, int64_t R) {
  const int64_t n = e->lat.n;
  for (int64_t r0 = 0; r0 < R; r0 += e->cols.batch) {
    const int64_t nr = std::min<int64_t>(e->cols.batch, R - r0);
    HIP_TRY(launch_xtwx_cols(e->stream, e->lat.X.ptr, n, e->p, e->lat.w.ptr,
                             e->cols.req.ptr + 2 * r0, (int)nr, e->dA.ptr, e->cols.V.ptr,
                             e->cols.valid.ptr, e->cols.words, e->cols.planes.ptr));
  }
  return BA_OK;
}

// Chains of the logit sampler parked at "add variable j" for want of vector j of
// their V (CHAIN_NEED_COLUMN): the vectors are computed -- one GEMM for all of
// them -- and the chains replay the sweep they were in, from its start and with the
// same draws, now finding the vector.  *served: something was replayed (st is fresh).
int serve_columns(ba_engine *e, std::vector<int32_t> &st, bool *served) {
  *served = false;
  if (!column_service(e->data_kind) || !e->cols.wanted.count) return BA_OK;
  const size_t C = (size_t)e->cfg.chains;
  bool any = false;
  for (size_t c = 0; c < C; ++c) any = any || st[c] == CHAIN_NEED_COLUMN || st[c] == CHAIN_NEED_COLUMN_BIG;
  if (!any) return BA_OK;
  std::vector<int32_t> want(C), req;
  HIP_TRY(hipMemcpy(want.data(), e->cols.wanted.ptr, C * 4, hipMemcpyDeviceToHost));
  for (size_t c = 0; c < C; ++c) {
    if (st[c] != CHAIN_NEED_COLUMN && st[c] != CHAIN_NEED_COLUMN_BIG) continue;
    if (want[c] < 0 || want[c] >= e->p) return fail(BA_E_STATE, "a parked chain names no variable");
    req.push_back((int32_t)c);
    req.push_back(want[c]);
    // (the large-model kernel takes its chains back in the parked state)
    st[c] = (st[c] == CHAIN_NEED_COLUMN) ? CHAIN_OK : CHAIN_MODEL_TOO_LARGE;
  }
  const int64_t R = (int64_t)req.size() / 2;
  HIP_TRY(hipMemcpyAsync(e->cols.req.ptr, req.data(), req.size() * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->dstatus.ptr, st.data(), C * 4, hipMemcpyHostToDevice, e->stream));
  int rc = build_columns(e, R);
  if (rc) return rc;
  SsvsParams P;
  fill_params(e, P);
  HIP_TRY(launch_sweeps(e, P, 0));   // the sweep still owed
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(st.data(), e->dstatus.ptr, C * 4, hipMemcpyDeviceToHost));
  *served = true;
  return BA_OK;
}

// A family's data on the device: X, the responses, the family's third vector (trial counts /
// exposures; none for Student-t), X squared for the families of the column service (the
// diagonal of X'WX).  The imputation starts over: no latent data, sweep 0.
int upload_latent_data(ba_engine *e, int64_t n, int32_t p, const double *X, const double *y,
                              const double *third, bool squared, int clt_threshold) {
  HIP_TRY(e->lat.X.resize((size_t)n * p));
  HIP_TRY(e->lat.y.resize((size_t)n));
  if (third) HIP_TRY(e->lat.aux.resize((size_t)n));
  HIP_TRY(hipMemcpy(e->lat.X.ptr, X, (size_t)n * p * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->lat.y.ptr, y, (size_t)n * 8, hipMemcpyHostToDevice));
  if (third) HIP_TRY(hipMemcpy(e->lat.aux.ptr, third, (size_t)n * 8, hipMemcpyHostToDevice));
  if (squared) {
    HIP_TRY(e->lat.Xsq.resize((size_t)n * p));
    HIP_TRY(launch_square(e->stream, e->lat.X.ptr, (size_t)n * p, e->lat.Xsq.ptr));
  }
  e->lat.z.release();
  e->lat.n = n;
  e->lat.clt = clt_threshold;
  e->lat.draws = 0;
  return BA_OK;
}

// the latent data of the binomial and Poisson samplers have unit variance: sigma^2 = 1 in
// every chain, whatever a caller left there before the data were set
int set_unit_sigsq(ba_engine *e) { return write_per_chain(e, e->dsigsq.ptr, -1, 1.0); }

// the imputation kernels' view of the data: what every family's kernel reads ...
static void fill_latent_params(ba_engine *e, LatentParams &L) {
  L.n = (int32_t)e->lat.n;
  L.p = (int32_t)e->p;
  L.chains = (int32_t)e->cfg.chains;
  L.slot_limit = e->slot_limit;
  L.chain_offset = e->cfg.chain_offset;
  L.X = e->lat.X.ptr;
  L.gamma = e->dgamma.ptr;
  L.beta = e->dbeta.ptr;
  L.z = e->lat.z.ptr;
  L.w = e->lat.w.ptr;
  L.seed_lo = (uint32_t)e->seed;
  L.seed_hi = (uint32_t)(e->seed >> 32);
  L.status = e->dstatus.ptr;
}

// ... and each family's own (the probit kernel reads neither w nor the mixtures)
void fill_probit_params(ba_engine *e, ProbitParams &Q) {
  std::memset(&Q, 0, sizeof(Q));
  fill_latent_params(e, Q);
  Q.clt_threshold = e->lat.clt;
  Q.y = e->lat.y.ptr;
  Q.ntrials = e->lat.aux.ptr;
  Q.xtz = e->dxty_c.ptr;
  Q.mix_off = e->dpois_off.ptr;
  Q.mix_mu = e->dpois_mu.ptr;
  Q.mix_sigma = e->dpois_sigma.ptr;
  Q.mix_logw = e->dpois_logw.ptr;
  Q.obs_mix = e->dpois_obs.ptr;
  Q.mix_one = e->poisson_mix_one;
}

void fill_student_params(ba_engine *e, StudentParams &T) {
  std::memset(&T, 0, sizeof(T));
  fill_latent_params(e, T);
  T.y = e->lat.y.ptr;
  T.sigsq = e->dsigsq.ptr;
  T.nu = e->dstu_nu.ptr;
  T.dx = e->dstu_dx.ptr;
  T.margin = e->dstu_margin.ptr;
  T.u = e->dstu_u.ptr;
  T.prior_df = e->prior_df;
  T.prior_ss = e->prior_ss;
  T.sigma_max = e->sigma_max;
  T.nu_kind = e->student_nu_kind;
  T.nu_a = e->student_nu_a;
  T.nu_b = e->student_nu_b;
  T.trace_idx = e->dtrace_idx.ptr;
  T.trace_sigsq = e->dtr_sig.ptr;
  T.trace_nu = e->dstu_nu_rec.ptr;
  T.trace_stride = e->dstu_nu_rec.count ? e->trace_stride : 0;
  T.acc = e->dacc.ptr;
}

static void fill_quantile_params(ba_engine *e, QuantileParams &U) {
  std::memset(&U, 0, sizeof(U));
  fill_latent_params(e, U);
  U.y = e->lat.y.ptr;
  U.shift = 1.0 - 2.0 * e->quantile_q;
}

static void fill_mlogit_params(ba_engine *e, MlogitParams &G) {
  std::memset(&G, 0, sizeof(G));
  fill_latent_params(e, G);
  G.n = (int32_t)e->mlogit_n;   // (the subjects: the rows are lat.n = n * nchoices)
  G.nchoices = e->mlogit_choices;
  G.y = e->dml_y.ptr;
  G.u = e->dml_u.ptr;
  G.wss_part = e->dml_wss_part.ptr;
  G.wss = e->dml_wss.ptr;
  // The normal mixture for the extreme value distribution, the three literal vectors of
  // MLVS_data_imputer.cpp:39-43 (means, variances, weights), and what the constructor there
  // derives from them: sigsq_inv_ = pow(variances, -1), sd_ = pow(sigsq_inv_, -0.5),
  // log_mixing_weights_ = log(weights).
  static const double kMu[MLOGIT_NCOMP] = {5.09, 3.29, 1.82, 1.24, 0.76, 0.39, 0.04, -0.31, -0.67, -1.06};
  static const double kVar[MLOGIT_NCOMP] = {4.5, 2.02, 1.1, 0.42, 0.2, 0.11, 0.08, 0.08, 0.09, 0.15};
  static const double kWeight[MLOGIT_NCOMP] = {0.004, 0.04, 0.168, 0.147, 0.125, 0.101, 0.104, 0.116, 0.107, 0.088};
  for (int c = 0; c < MLOGIT_NCOMP; ++c) {
    G.mix_mu[c] = kMu[c];
    G.mix_prec[c] = std::pow(kVar[c], -1.0);
    G.mix_sd[c] = std::pow(G.mix_prec[c], -0.5);
    G.mix_logsd[c] = std::log(G.mix_sd[c]);
    G.mix_logw[c] = std::log(kWeight[c]);
  }
}

// the Student sampler's per-chain state: nu = 30 (TRegression.cpp:35-45), suggested_dx = 1
// (TRegressionSampler.cpp:88-107), no slice comparison seen yet
int student_prepare(ba_engine *e) {
  int rc = alloc_chain_state(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains;
  if (e->dstu_nu.count == C) return BA_OK;
  HIP_TRY(e->dstu_nu.resize(C));
  HIP_TRY(e->dstu_dx.resize(C));
  HIP_TRY(e->dstu_margin.resize(C));
  std::vector<double> nu(C, 30.0), dx(C, 1.0), m(C, std::numeric_limits<double>::infinity());
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(e->dstu_nu.ptr, nu.data(), C * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->dstu_dx.ptr, dx.data(), C * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->dstu_margin.ptr, m.data(), C * 8, hipMemcpyHostToDevice));
  return BA_OK;
}

// the buffers of the families whose V is every chain's own (chains x n latent responses and
// weights, V, its diagonal, the column service's lists and planes)
int column_buffers(ba_engine *e) {
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, n = (size_t)e->lat.n;
  if (e->lat.z.count != C * n || e->cols.V.count != C * p * p) {
    HIP_TRY(e->lat.z.resize(C * n));
    HIP_TRY(e->lat.w.resize(C * n));
    HIP_TRY(e->cols.V.resize(C * p * p));
    HIP_TRY(e->dxty_c.resize(C * p));
    e->cols.words = (int)((p + 31) / 32);
    HIP_TRY(e->cols.vdiag.resize(C * p));
    HIP_TRY(e->cols.valid.resize(C * (size_t)e->cols.words));
    HIP_TRY(e->cols.req.resize(2 * C * p));
    HIP_TRY(e->cols.count.resize(1));
    HIP_TRY(e->cols.wanted.resize(C));
    // the planes of one column GEMM launch: at most 1 GiB, at least one request tile; the
    // workspace also holds the planes of the rows products, one set per chain (planes_sizing.h)
    e->cols.batch = column_request_batch(C, (int64_t)n, p);
    HIP_TRY(e->cols.planes.resize(column_planes_doubles(C, (int64_t)n, p)));
  }
  return BA_OK;
}

// the sweep loop shared by the logit, the Poisson, the Student-t and the quantile samplers:
// imputation (per family), X'Wz and the diagonal, the vectors of V the sweep starts from, the
// inclusion / coefficient draws with park-and-replay for vectors requested mid-sweep
static int logit_family_sweep(ba_engine *e, int32_t nsweeps) {
  const DataKind kind = e->data_kind;
  const bool student = kind == DATA_STUDENT;
  if (!e->have_slab) return fail(BA_E_STATE, "call ba_sss_set_slab first");
  if (student && !e->sss_slab_scales)
    return fail(BA_E_INVALID, "the Student-t sampler takes a slab whose precision scales with sigma^2 (scales_with_sigsq = 1)");
  if (kind == DATA_QUANTILE && e->sss_slab_scales)
    return fail(BA_E_INVALID, "the quantile regression sampler takes a fixed-precision slab (scales_with_sigsq = 0)");
  if (kind == DATA_MLOGIT && e->sss_slab_scales)
    return fail(BA_E_INVALID, "the multinomial logit sampler takes a fixed-precision slab (scales_with_sigsq = 0)");
  if (!student && e->sss_slab_scales) return fail(BA_E_INVALID, "the logit sampler takes a fixed-precision slab (scales_with_sigsq = 0)");
  int rc = alloc_chain_state(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, n = (size_t)e->lat.n;
  if (student) {
    rc = student_prepare(e);
    if (rc) return rc;
    if (e->trace_stride > 0 && nsweeps > e->trace_stride)
      return fail(BA_E_INVALID, "nsweeps exceeds the enabled trace length");
    if (e->dstu_u.count != C * n) HIP_TRY(e->dstu_u.resize(C * n));
  }
  if (kind == DATA_MLOGIT) {
    const size_t nb = (size_t)((e->mlogit_n + 255) / 256);
    if (e->dml_u.count != C * n) HIP_TRY(e->dml_u.resize(C * n));
    if (e->dml_wss_part.count != C * nb) HIP_TRY(e->dml_wss_part.resize(C * nb));
    if (e->dml_wss.count != C) {
      HIP_TRY(e->dml_wss.resize(C));
      HIP_TRY(hipMemset(e->dml_wss.ptr, 0, C * 8));
    }
    if (e->dml_order.count != p) {   // (default: the identity)
      std::vector<uint16_t> id(p);
      for (size_t j = 0; j < p; ++j) id[j] = (uint16_t)j;
      HIP_TRY(e->dml_order.resize(p));
      HIP_TRY(hipMemcpy(e->dml_order.ptr, id.data(), p * 2, hipMemcpyHostToDevice));
    }
  }
  rc = column_buffers(e);
  if (rc) return rc;
  if (!student) {
    rc = set_unit_sigsq(e);
    if (rc) return rc;
  }
  rc = switch_mode(e, 1, 1.0);
  if (rc) return rc;
  rc = upload_shared(e);
  if (rc) return rc;
  HIP_TRY(e->dmodel.resize(2 * C * ssvs_scalar_layout(64).total));
  SsvsParams P;
  fill_params(e, P);
  // the imputation kernel's parameters: the struct of the family in hand
  ProbitParams Q;
  StudentParams T;
  QuantileParams U;
  MlogitParams G;
  LatentParams *L;
  switch (kind) {
    case DATA_STUDENT: fill_student_params(e, T); L = &T; break;
    case DATA_QUANTILE: fill_quantile_params(e, U); L = &U; break;
    case DATA_MLOGIT: fill_mlogit_params(e, G); L = &G; break;
    default: fill_probit_params(e, Q); L = &Q; break;   // (logit, Poisson)
  }
  double *const Xsq = e->lat.Xsq.ptr, *const xtz = e->dxty_c.ptr, *const vdiag = e->cols.vdiag.ptr,
               *const planes = e->cols.planes.ptr;
  // (the draws recorded are those of the last ba_student_sweep call)
  if (student && e->trace_stride > 0) HIP_TRY(hipMemsetAsync(e->dtrace_idx.ptr, 0, C * 4, e->stream));
  // BinomialLogitSpikeSlabSampler::draw (BinomialLogitSpikeSlabSampler.cpp:50-54) /
  // PoissonRegressionSpikeSlabSampler::draw (PoissonRegressionSpikeSlabSampler.cpp:55-59) /
  // QuantileRegressionSpikeSlabSampler::draw (QuantileRegressionPosteriorSampler.cpp:77-91) /
  // MLVS::draw (MLVS.cpp:71-75)
  for (int i = 0; i < nsweeps; ++i) {
    L->sweep = e->lat.draws++;
    // impute_latent_data: z, w, X'Wz and the diagonal of V = slab precision + X'WX ...
    switch (kind) {
      case DATA_STUDENT: HIP_TRY(launch_student_impute(e->stream, T, Xsq, e->dA.ptr, xtz, vdiag, planes)); break;
      case DATA_QUANTILE: HIP_TRY(launch_quantile_impute(e->stream, U, Xsq, e->dA.ptr, xtz, vdiag, planes)); break;
      case DATA_MLOGIT: HIP_TRY(launch_mlogit_impute(e->stream, G, Xsq, e->dA.ptr, xtz, vdiag, planes)); break;
      case DATA_POISSON: HIP_TRY(launch_logit_impute(e->stream, Q, Xsq, e->dA.ptr, vdiag, planes, 2)); break;
      default: HIP_TRY(launch_logit_impute(e->stream, Q, Xsq, e->dA.ptr, vdiag, planes, e->logit_imputer)); break;
    }
    // ... and the vectors of V the sweep starts from: those of the included variables
    HIP_TRY(launch_xtwx_cols_start(e->stream, e->dgamma.ptr, (int)C, (int)p, e->cols.req.ptr,
                                   e->cols.count.ptr, e->cols.valid.ptr, e->cols.words));
    int32_t R = 0;
    HIP_TRY(hipMemcpyAsync(&R, e->cols.count.ptr, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = build_columns(e, R);
    if (rc) return rc;
    HIP_TRY(launch_sweeps(e, P, 1));                                         // draw_model_indicators, draw_beta
    // (a chain that stopped for a missing vector of V, or outgrew the launch's
    // capacity, replays THIS sweep's draws on this sweep's latent data before the
    // next imputation: check_chain_status serves both)
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = check_chain_status(e);
    if (rc) return rc;
    if (student) {
      // draw_sigsq_full_conditional, draw_nu_given_observed_data
      HIP_TRY(launch_student_sigma_nu(e->stream, T));
      rc = check_chain_status(e);
      if (rc) return rc;
    }
    fill_params(e, P);
  }
  e->table_ok = false;
  e->model_ok = false;
  return BA_OK;
}

// the sweep entry points that are nothing but the loop above on their own kind of data
static int latent_sweep_entry(ba_engine *e, DataKind kind, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = sweep_refusal(e, kind);
  if (rc) return rc;
  return logit_family_sweep(e, nsweeps);
}

// the getters' refusal while `buf` does not hold `count` doubles of an imputation
static int imputed(const ba_engine *e, const DevBuf<double> &buf, size_t count, const char *sweep_first) {
  if (buf.count != count || e->lat.draws == 0) return fail(BA_E_STATE, sweep_first);
  return BA_OK;
}

}  // namespace boom_amd

extern "C" {

// ------------------------ BinomialProbitSpikeSlabSampler (data augmentation + SpikeSlabSampler)
int ba_probit_set_data(ba_engine *e, int64_t n, int32_t p, const double *X, const double *y,
                       const double *ntrials, int32_t clt_threshold) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!X || !y || !ntrials) return fail(BA_E_INVALID, "null argument");
  if (n <= 0 || p <= 0) return fail(BA_E_INVALID, "n and p must be positive");
  // up to 2 * clt_threshold truncated-normal draws per observation read the
  // observation's substream of PROBIT_STRIDE uniforms (a draw takes 2 - 20 of them)
  if (clt_threshold < 0 || clt_threshold > 64)
    return fail(BA_E_INVALID, "clt_threshold must be between 0 and 64");
  for (int64_t i = 0; i < n; ++i) {
    if (y[i] < 0 || ntrials[i] < 0)
      return fail(BA_E_INVALID, "Negative values not allowed in BinomialProbitDataImputer::impute().");
    if (y[i] > ntrials[i])
      return fail(BA_E_INVALID, "Success count exceeds trial count in BinomialProbitDataImputer::impute.");
  }
  // refresh_xtx (BinomialProbitSpikeSlabSampler.cpp:71-77): X'NX, built on the
  // matrix cores from the rows scaled by sqrt(n_i).  Exact for Bernoulli data; for
  // trial counts that are not perfect squares sqrt(n_i)^2 differs from n_i by one
  // rounding, i.e. an element differs from the reference's sum_i n_i x x' by no more
  // than the two summation orders already differ (~1e-16 relative per term).  The
  // binomial cases of tests/test_probit_gpu.py (1 - 8 and 1 - 12 trials) hold the
  // inclusion indicators bit-exact against the oracle on this matrix.
  std::vector<double> Xs((size_t)n * p), zero((size_t)n, 0.0);
  for (int32_t j = 0; j < p; ++j)
    for (int64_t i = 0; i < n; ++i) Xs[(size_t)j * n + i] = X[(size_t)j * n + i] * std::sqrt(ntrials[i]);
  int rc = ba_build_suf_from_xy(e, n, p, Xs.data(), zero.data());
  if (rc) return rc;
  rc = upload_latent_data(e, n, p, X, y, ntrials, /*squared=*/false, clt_threshold);
  if (rc) return rc;
  e->data_kind = DATA_PROBIT;
  return BA_OK;
}

int ba_probit_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = sweep_refusal(e, DATA_PROBIT);
  if (rc) return rc;
  if (!e->have_slab) return fail(BA_E_STATE, "call ba_sss_set_slab first");
  if (e->sss_slab_scales) return fail(BA_E_INVALID, "the probit sampler takes a fixed-precision slab (scales_with_sigsq = 0)");
  rc = alloc_chain_state(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, n = (size_t)e->lat.n;
  if (e->lat.z.count != C * n) {
    HIP_TRY(e->lat.z.resize(C * n));
    HIP_TRY(e->dxty_c.resize(C * p));
    HIP_TRY(e->cols.planes.resize((size_t)xtwx_cols_planes((int64_t)n) * C * p));   // (split-K planes of X'z)
  }
  rc = set_unit_sigsq(e);
  if (rc) return rc;
  rc = switch_mode(e, 1, 1.0);
  if (rc) return rc;
  rc = upload_shared(e);
  if (rc) return rc;
  HIP_TRY(e->dmodel.resize(2 * C * ssvs_scalar_layout(64).total));
  SsvsParams P;
  fill_params(e, P);
  ProbitParams Q;
  fill_probit_params(e, Q);
  // BinomialProbitSpikeSlabSampler::draw (BinomialProbitSpikeSlabSampler.cpp:40-46)
  for (int i = 0; i < nsweeps; ++i) {
    Q.sweep = e->lat.draws++;
    HIP_TRY(launch_probit_impute(e->stream, Q, e->cols.planes.ptr));   // impute_latent_data, X'z
    HIP_TRY(launch_sweeps(e, P, 1));               // draw_model_indicators, draw_beta
    // (a chain that outgrew the launch's capacity replays THIS sweep's draws on
    // this sweep's latent data before the next imputation)
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = check_chain_status(e);
    if (rc) return rc;
    fill_params(e, P);
    P.model_keep = 1;
    e->model_ok = true;
  }
  return BA_OK;
}

// ------------------------ BinomialLogitSpikeSlabSampler (auxiliary-mixture augmentation)
int ba_logit_set_data(ba_engine *e, int64_t n, int32_t p, const double *X, const double *y,
                      const double *ntrials, int32_t clt_threshold) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!X || !y || !ntrials) return fail(BA_E_INVALID, "null argument");
  if (n <= 0 || p <= 0) return fail(BA_E_INVALID, "n and p must be positive");
  // (per-trial imputation reads two uniforms per trial of the observation's substream
  // of LOGIT_STRIDE; the large-sample branch beyond the threshold a few dozen)
  if (clt_threshold < 1 || 4 * clt_threshold > LOGIT_STRIDE)
    return fail(BA_E_INVALID, "clt_threshold must be between 1 and 64");
  for (int64_t i = 0; i < n; ++i) {
    if (y[i] < 0 || ntrials[i] < 0)
      return fail(BA_E_INVALID, "The number of successes and the number of trials must both be non-negative in BinomialLogitPartialAugmentationDataImputer::impute().");
    if (y[i] > ntrials[i])
      return fail(BA_E_INVALID, "The number of successes must not exceed the number of trials in BinomialLogitPartialAugmentationDataImputer::impute().");
  }
  // (dimensions, the shared buffers and a placeholder X'X; the sweeps use every
  // chain's own X'WX)
  std::vector<double> zero((size_t)n, 0.0);
  int rc = ba_build_suf_from_xy(e, n, p, X, zero.data());
  if (rc) return rc;
  rc = upload_latent_data(e, n, p, X, y, ntrials, /*squared=*/true, clt_threshold);
  if (rc) return rc;
  e->data_kind = DATA_LOGIT;
  return BA_OK;
}

int ba_logit_set_imputer(ba_engine *e, int32_t kind) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (kind != 0 && kind != 1) return fail(BA_E_INVALID, "imputer must be 0 (auxiliary mixture) or 1 (Polya-Gamma)");
  // (StateSpaceLogitPosteriorSampler has the auxiliary-mixture imputer only)
  if (e->data_kind == DATA_SS_LOGIT)
    return fail(BA_E_STATE, "logit state-space data are set: the imputer is the auxiliary mixture's");
  MUTATE(e);
  e->logit_imputer = kind;
  return BA_OK;
}

int ba_logit_sweep(ba_engine *e, int32_t nsweeps) { return latent_sweep_entry(e, DATA_LOGIT, nsweeps); }

// ------------------------ PoissonRegressionSpikeSlabSampler
int ba_poisson_set_data(ba_engine *e, int64_t n, int32_t p, const double *X, const double *y,
                        const double *exposure) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!X || !y || !exposure) return fail(BA_E_INVALID, "null argument");
  if (n <= 0 || p <= 0) return fail(BA_E_INVALID, "n and p must be positive");
  for (int64_t i = 0; i < n; ++i) {
    if (y[i] < 0 || y[i] != std::floor(y[i])) return fail(BA_E_INVALID, "counts must be non-negative integers");
    if (!(exposure[i] > 0)) return fail(BA_E_INVALID, "exposures must be positive");
  }
  std::vector<double> zero((size_t)n, 0.0);
  int rc = ba_build_suf_from_xy(e, n, p, X, zero.data());   // (dimensions and the shared buffers)
  if (rc) return rc;
  rc = upload_latent_data(e, n, p, X, y, exposure, /*squared=*/true, 0);
  if (rc) return rc;
  e->poisson_y.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) e->poisson_y[(size_t)i] = (int64_t)std::llround(y[i]);
  e->poisson_mix_set = false;
  e->data_kind = DATA_POISSON;
  return BA_OK;
}

int ba_poisson_set_mixtures(ba_engine *e, int32_t ncounts, const int64_t *counts, const int32_t *ncomp,
                            const double *mu, const double *sigma, const double *weight,
                            int64_t largest_index) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  // (the state space Poisson family too: ba_ss_poisson_set_data fills poisson_y from the observed steps)
  if (e->data_kind != DATA_POISSON && e->data_kind != DATA_SS_POISSON) return fail(BA_E_STATE, set_data_first(DATA_POISSON));
  if (ncounts <= 0 || !counts || !ncomp || !mu || !sigma || !weight) return fail(BA_E_INVALID, "null argument");
  std::vector<int32_t> off((size_t)ncounts + 1, 0);
  for (int i = 0; i < ncounts; ++i) {
    if (i > 0 && counts[i] <= counts[i - 1]) return fail(BA_E_INVALID, "counts must be ascending and distinct");
    if (ncomp[i] <= 0 || ncomp[i] > POISSON_MAX_COMP) return fail(BA_E_INVALID, "a mixture has 1 .. 32 components");
    off[(size_t)i + 1] = off[(size_t)i] + ncomp[i];
  }
  const size_t tot = (size_t)off[(size_t)ncounts];
  std::vector<double> logw(tot);
  for (size_t c = 0; c < tot; ++c) {
    if (!(weight[c] > 0) || !(sigma[c] > 0)) return fail(BA_E_INVALID, "mixture weights and standard deviations must be positive");
    logw[c] = std::log(weight[c]);
  }
  auto find = [&](int64_t v) -> int {
    const int64_t *it = std::lower_bound(counts, counts + ncounts, v);
    return (it != counts + ncounts && *it == v) ? (int)(it - counts) : -2;
  };
  const size_t n = e->poisson_y.size();
  std::vector<int32_t> obs(n, -1);
  for (size_t i = 0; i < n; ++i) {
    const int64_t v = e->poisson_y[i];
    if (v <= 0) continue;
    if (v >= largest_index) { obs[i] = -1; continue; }   // the Gaussian limit (poisson_mixture_approximation_table.cpp:49-55)
    const int m = find(v);
    if (m < 0) return fail(BA_E_INVALID, "no mixture was given for a count that occurs in the data");
    obs[i] = m;
  }
  const int one = find(1);
  if (one < 0) return fail(BA_E_INVALID, "the mixture of count 1 (the event past the interval) is needed");
  HIP_TRY(e->dpois_off.resize(off.size()));
  HIP_TRY(e->dpois_mu.resize(tot));
  HIP_TRY(e->dpois_sigma.resize(tot));
  HIP_TRY(e->dpois_logw.resize(tot));
  HIP_TRY(e->dpois_obs.resize(n));
  HIP_TRY(hipMemcpy(e->dpois_off.ptr, off.data(), off.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->dpois_mu.ptr, mu, tot * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->dpois_sigma.ptr, sigma, tot * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->dpois_logw.ptr, logw.data(), tot * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->dpois_obs.ptr, obs.data(), n * 4, hipMemcpyHostToDevice));
  e->poisson_mix_one = one;
  e->poisson_mix_set = true;
  return BA_OK;
}

int ba_poisson_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = sweep_refusal(e, DATA_POISSON);
  if (rc) return rc;
  if (!e->poisson_mix_set) return fail(BA_E_STATE, "call ba_poisson_set_mixtures first");
  return logit_family_sweep(e, nsweeps);
}

// ------------------------ TRegressionSpikeSlabSampler
int ba_student_set_data(ba_engine *e, int64_t n, int32_t p, const double *X, const double *y) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!X || !y) return fail(BA_E_INVALID, "null argument");
  if (n <= 0 || p <= 0) return fail(BA_E_INVALID, "n and p must be positive");
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(y[i])) return fail(BA_E_INVALID, "responses must be finite");
  std::vector<double> zero((size_t)n, 0.0);
  int rc = ba_build_suf_from_xy(e, n, p, X, zero.data());   // (dimensions and the shared buffers)
  if (rc) return rc;
  rc = upload_latent_data(e, n, p, X, y, nullptr, /*squared=*/true, 0);
  if (rc) return rc;
  e->dstu_u.release();
  // a new TRegressionModel: nu = 30, suggested_dx = 1, no slice margin yet (student_prepare)
  e->dstu_nu.release();
  e->dstu_dx.release();
  e->dstu_margin.release();
  e->data_kind = DATA_STUDENT;
  return BA_OK;
}

int ba_student_allow_model_selection(ba_engine *e, int32_t allow) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  e->student_allow_selection = allow != 0;
  return BA_OK;
}

int ba_student_set_nu_prior(ba_engine *e, int32_t kind, double a, double b) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (kind == STUDENT_NU_UNIFORM) {
    if (!(std::isfinite(a) && std::isfinite(b) && a >= 0 && b > a))
      return fail(BA_E_INVALID, "a Uniform(a, b) prior on nu needs 0 <= a < b, both finite");
  } else if (kind == STUDENT_NU_GAMMA) {
    if (!(std::isfinite(a) && std::isfinite(b) && a > 0 && b > 0))
      return fail(BA_E_INVALID, "a Gamma(a, b) prior on nu needs a positive shape and rate");
  } else {
    return fail(BA_E_INVALID, "kind must be 0 (Uniform) or 1 (Gamma)");
  }
  MUTATE(e);
  e->student_nu_kind = kind;
  e->student_nu_a = a;
  e->student_nu_b = b;
  return BA_OK;
}

int ba_student_set_nu(ba_engine *e, int64_t chain, double nu) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!(nu > 0) || !std::isfinite(nu)) return fail(BA_E_INVALID, "nu must be positive and finite");
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = student_prepare(e);
  if (rc) return rc;
  return write_per_chain(e, e->dstu_nu.ptr, chain, nu);
}

int ba_student_get_nu(ba_engine *e, int64_t chain, double *nu) {
  ENGINE_PROLOGUE(e);
  if (!nu) return fail(BA_E_INVALID, "null argument");
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = student_prepare(e);
  if (rc) return rc;
  return read_per_chain(e, e->dstu_nu.ptr, chain, nu);
}

int ba_student_get_margin(ba_engine *e, int64_t chain, double *margin) {
  ENGINE_PROLOGUE(e);
  if (!margin) return fail(BA_E_INVALID, "null argument");
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = student_prepare(e);
  if (rc) return rc;
  return read_per_chain(e, e->dstu_margin.ptr, chain, margin);
}

int ba_student_get_weights(ba_engine *e, int64_t chain, double *w) {
  ENGINE_PROLOGUE(e);
  if (!w) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != DATA_STUDENT) return fail(BA_E_STATE, set_data_first(DATA_STUDENT));
  const size_t n = (size_t)e->lat.n;
  return read_chain_row(e, chain, e->lat.w, n, w, [&] {
    return imputed(e, e->lat.w, (size_t)e->cfg.chains * n, "no imputation has run yet: call ba_student_sweep first");
  });
}

int ba_student_get_nu_draws(ba_engine *e, int64_t chain, int32_t nsweeps, double *out) {
  ENGINE_PROLOGUE(e);
  if (!out) return fail(BA_E_INVALID, "null argument");
  if (e->trace_stride <= 0 || e->dstu_nu_rec.count == 0)
    return fail(BA_E_STATE, "draws are not recorded: call ba_enable_draws before ba_student_sweep");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  if (nsweeps <= 0 || nsweeps > e->trace_stride) return fail(BA_E_INVALID, "nsweeps out of range");
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, e->dstu_nu_rec.ptr + (size_t)chain * e->trace_stride, (size_t)nsweeps * 8,
                    hipMemcpyDeviceToHost));
  return BA_OK;
}

int ba_student_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = sweep_refusal(e, DATA_STUDENT);
  if (rc) return rc;
  if (e->trace_stride > 0 && e->dstu_nu_rec.count != (size_t)e->cfg.chains * e->trace_stride) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(e->dstu_nu_rec.resize((size_t)e->cfg.chains * e->trace_stride));
  }
  return logit_family_sweep(e, nsweeps);
}

// ------------------------ QuantileRegressionSpikeSlabSampler
int ba_quantile_set_data(ba_engine *e, int64_t n, int32_t p, const double *X, const double *y, double quantile) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!X || !y) return fail(BA_E_INVALID, "null argument");
  if (n <= 0 || p <= 0) return fail(BA_E_INVALID, "n and p must be positive");
  if (!(quantile > 0 && quantile < 1)) return fail(BA_E_INVALID, "quantile must be strictly between 0 and 1");
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(y[i])) return fail(BA_E_INVALID, "responses must be finite");
  std::vector<double> zero((size_t)n, 0.0);
  int rc = ba_build_suf_from_xy(e, n, p, X, zero.data());   // (dimensions and the shared buffers)
  if (rc) return rc;
  rc = upload_latent_data(e, n, p, X, y, nullptr, /*squared=*/true, 0);
  if (rc) return rc;
  e->quantile_q = quantile;
  e->data_kind = DATA_QUANTILE;
  return BA_OK;
}

int ba_quantile_sweep(ba_engine *e, int32_t nsweeps) { return latent_sweep_entry(e, DATA_QUANTILE, nsweeps); }

int ba_quantile_get_weights(ba_engine *e, int64_t chain, double *w) {
  ENGINE_PROLOGUE(e);
  if (!w) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != DATA_QUANTILE) return fail(BA_E_STATE, set_data_first(DATA_QUANTILE));
  const size_t n = (size_t)e->lat.n;
  return read_chain_row(e, chain, e->lat.w, n, w, [&] {
    return imputed(e, e->lat.w, (size_t)e->cfg.chains * n, "no imputation has run yet: call ba_quantile_sweep first");
  });
}

// ------------------------ MLVS (multinomial logit spike and slab)
int ba_mlogit_set_data(ba_engine *e, int64_t n, int32_t nchoices, int32_t psub, int32_t pch, const int32_t *y,
                       const double *Xsubject, const double *Xchoice) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!y) return fail(BA_E_INVALID, "null argument");
  if (n <= 0) return fail(BA_E_INVALID, "n must be positive");
  if (nchoices < 2 || nchoices > MLOGIT_MAX_CHOICES)
    return fail(BA_E_INVALID, "the number of choices must be between 2 and 16");
  if (psub < 0 || pch < 0 || (psub == 0 && pch == 0))
    return fail(BA_E_INVALID, "subject and choice dimensions must be non-negative and not both zero");
  if ((psub > 0) != (Xsubject != nullptr)) return fail(BA_E_INVALID, "Xsubject must be given iff psub > 0");
  if ((pch > 0) != (Xchoice != nullptr)) return fail(BA_E_INVALID, "Xchoice must be given iff pch > 0");
  for (int64_t i = 0; i < n; ++i)
    if (y[i] < 0 || y[i] >= nchoices) return fail(BA_E_INVALID, "responses must be choices 0 .. nchoices - 1");
  const int64_t N = n * nchoices, D = (int64_t)(nchoices - 1) * psub + pch;
  if (D > 65535) return fail(BA_E_INVALID, "number of predictors must be in [1, 65535]");
  if (N > (int64_t)0x7fffffff) return fail(BA_E_INVALID, "n times the number of choices must fit 31 bits");
  // the expanded design and its element-wise square stay on the device: 16 N D bytes
  if ((double)N * (double)D * 16.0 > 8.0 * 1073741824.0)
    return fail(BA_E_INVALID, "the expanded design (n nchoices rows by (nchoices - 1) psub + pch columns, 16 bytes "
                              "an element with its square) exceeds 8 GiB");
  DevBuf<double> dxs, dxc, zero;
  if (psub > 0) {
    HIP_TRY(dxs.resize((size_t)n * psub));
    HIP_TRY(hipMemcpy(dxs.ptr, Xsubject, (size_t)n * psub * 8, hipMemcpyHostToDevice));
  }
  if (pch > 0) {
    HIP_TRY(dxc.resize((size_t)N * pch));
    HIP_TRY(hipMemcpy(dxc.ptr, Xchoice, (size_t)N * pch * 8, hipMemcpyHostToDevice));
  }
  HIP_TRY(e->lat.X.resize((size_t)N * D));
  HIP_TRY(e->lat.Xsq.resize((size_t)N * D));
  HIP_TRY(launch_mlogit_expand(e->stream, n, nchoices, psub, pch, dxs.ptr, dxc.ptr, e->lat.X.ptr, e->lat.Xsq.ptr));
  HIP_TRY(zero.resize((size_t)N));
  HIP_TRY(hipMemsetAsync(zero.ptr, 0, (size_t)N * 8, e->stream));
  int rc = ba_build_suf_from_xy_device(e, N, (int32_t)D, e->lat.X.ptr, zero.ptr);   // (dimensions and the shared buffers)
  if (rc) return rc;
  HIP_TRY(e->dml_y.resize((size_t)n));
  HIP_TRY(hipMemcpy(e->dml_y.ptr, y, (size_t)n * 4, hipMemcpyHostToDevice));
  e->lat.z.release();
  e->dml_u.release();
  e->dml_order.release();   // (the identity until ba_mlogit_set_flip_order)
  e->lat.n = N;
  e->lat.clt = 0;
  e->lat.draws = 0;
  e->mlogit_n = n;
  e->mlogit_choices = nchoices;
  e->mlogit_psub = psub;
  e->mlogit_pch = pch;
  e->data_kind = DATA_MLOGIT;
  return BA_OK;
}

int ba_mlogit_set_flip_order(ba_engine *e, const int32_t *order) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!order) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != DATA_MLOGIT) return fail(BA_E_STATE, set_data_first(DATA_MLOGIT));
  const size_t p = (size_t)e->p;
  std::vector<uint16_t> o(p);
  std::vector<uint8_t> seen(p, 0);
  for (size_t j = 0; j < p; ++j) {
    if (order[j] < 0 || (size_t)order[j] >= p || seen[(size_t)order[j]])
      return fail(BA_E_INVALID, "the flip order must be a permutation of 0 .. D - 1");
    seen[(size_t)order[j]] = 1;
    o[j] = (uint16_t)order[j];
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(e->dml_order.resize(p));
  HIP_TRY(hipMemcpy(e->dml_order.ptr, o.data(), p * 2, hipMemcpyHostToDevice));
  return BA_OK;
}

int ba_mlogit_allow_model_selection(ba_engine *e, int32_t allow) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  e->mlogit_select = allow != 0;
  return BA_OK;
}

int ba_mlogit_sweep(ba_engine *e, int32_t nsweeps) { return latent_sweep_entry(e, DATA_MLOGIT, nsweeps); }

int ba_mlogit_get_latent(ba_engine *e, int64_t chain, double *u, double *w) {
  ENGINE_PROLOGUE(e);
  if (!u || !w) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != DATA_MLOGIT) return fail(BA_E_STATE, set_data_first(DATA_MLOGIT));
  const size_t N = (size_t)e->lat.n;
  auto ready = [&] {
    return imputed(e, e->dml_u, (size_t)e->cfg.chains * N, "no imputation has run yet: call ba_mlogit_sweep first");
  };
  int rc = read_chain_row(e, chain, e->dml_u, N, u, ready);
  if (rc) return rc;
  return read_chain_row(e, chain, e->lat.w, N, w, ready);
}

int ba_mlogit_get_wss(ba_engine *e, int64_t chain, double *wss) {
  ENGINE_PROLOGUE(e);
  if (!wss) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != DATA_MLOGIT) return fail(BA_E_STATE, set_data_first(DATA_MLOGIT));
  return read_chain_row(e, chain, e->dml_wss, 1, wss, [&] {
    return imputed(e, e->dml_wss, (size_t)e->cfg.chains, "no imputation has run yet: call ba_mlogit_sweep first");
  });
}

}  // extern "C"
