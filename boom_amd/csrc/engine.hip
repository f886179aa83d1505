// Host side of the C-ABI (include/boom_amd.h): owns the device buffers of one
// engine, assembles priors the way BregVsSampler's constructors do, launches
// the kernels and turns per-chain status words back into the reference's
// error messages.
#include "engine_internal.h"

namespace boom_amd {

static thread_local std::string g_error = "";

int fail(int code, const std::string &msg) {
  g_error = msg;
  return code;
}

}  // namespace boom_amd

namespace {


const char *status_message(int st) {
  switch (st) {
    case CHAIN_NOT_PD:
      return "The posterior information matrix is not positive definite.  "
             "Check your data or consider adjusting your prior.";
    case CHAIN_NEGATIVE_SS:
      return "Illegal data caused negative sum of squares in "
             "Breg::set_reg_post_params.";
    case CHAIN_ILLEGAL_START:
      return "BregVsSampler did not start with a legal configuration.";
    case CHAIN_RNG_BRANCH:
      return "Variance draw failed: lower bound must be to the right of the mode "
             "of logf in BoundedAdaptiveRejectionSampler, or a rejection sampler "
             "exceeded its number of attempts.";
    case CHAIN_FORECAST_VARIANCE:
      return "Found a zero (or negative) forecast variance!";
    case CHAIN_MODEL_TOO_LARGE:
      return "A chain's model size exceeded the engine's working capacity "
             "(a pinned max_model_size_hint, or more than 1024 variables in "
             "the model).";
    case STUDENT_SLICE_ERROR:
      return "The slice sampler of nu failed in ScalarSliceSampler (an infinite "
             "log density at the current value, an infinite upper limit, more than "
             "100 doublings or more than 100 contractions).";
    case QUANTILE_WEIGHT_ERROR:
      return "An inverse-Gaussian weight of the quantile regression imputation came out "
             "non-finite or not positive.";
    case MLOGIT_IMPUTE_ERROR:
      return "A linear predictor or a utility of the multinomial logit imputation came out "
             "non-finite, or the mixture component scan of rmulti fell off its end.";
    case MLVS_ILLEGAL_START:
      return "MLVS did not start with a legal configuration.";
    case STUDENT_BAD_WEIGHT:
      return "Weights must be finite and non-negative.";
    case AR_SPIKE_BAD_DRAW:
      return "A coefficient or variance draw of the spike-and-slab autoregression sampler came out non-finite.";
    case RHH_BAD_DRAW:
      return "A draw of the hierarchical regression holiday sampler met a matrix that is not positive definite or came out non-finite.";
    default:
      return "unknown chain status";
  }
}

int status_code(int st) {
  switch (st) {
    case CHAIN_NOT_PD: return BA_E_NOT_PD;
    case CHAIN_NEGATIVE_SS: return BA_E_NEGATIVE_SS;
    case CHAIN_ILLEGAL_START: return BA_E_ILLEGAL_START;
    case CHAIN_RNG_BRANCH: return BA_E_RNG_BRANCH;
    case CHAIN_FORECAST_VARIANCE: return BA_E_FORECAST_VARIANCE;
    case CHAIN_MODEL_TOO_LARGE: return BA_E_MODEL_TOO_LARGE;
    case STUDENT_SLICE_ERROR: return BA_E_RNG_BRANCH;
    case QUANTILE_WEIGHT_ERROR: return BA_E_RNG_BRANCH;
    case MLOGIT_IMPUTE_ERROR: return BA_E_RNG_BRANCH;
    case MLVS_ILLEGAL_START: return BA_E_ILLEGAL_START;
    case STUDENT_BAD_WEIGHT: return BA_E_INVALID;
    case AR_SPIKE_BAD_DRAW: return BA_E_INVALID;
    case RHH_BAD_DRAW: return BA_E_NOT_PD;
    default: return BA_E_INVALID;
  }
}

}  // namespace

namespace boom_amd {
thread_local KTimer *g_kt = nullptr;   // the timer of the engine whose entry point this thread is in
bool kt_active() { return g_kt != nullptr; }
void kt_mark(hipStream_t stream, int cls, bool begin) {
  KTimer *k = g_kt;
  if (!k || cls < 0 || cls >= KT_CLASSES) return;
  if (k->open.size() < (size_t)KT_CLASSES) k->open.resize(KT_CLASSES, nullptr);
  hipEvent_t ev = k->get();
  (void)hipEventRecord(ev, stream);
  if (begin) {
    if (k->open[cls]) k->pool.push_back(k->open[cls]);
    k->open[cls] = ev;
  } else if (k->open[cls]) {
    k->spans.push_back(KtSpan{cls, k->open[cls], ev});
    k->open[cls] = nullptr;
  } else {
    k->pool.push_back(ev);
  }
}
}  // namespace boom_amd

namespace boom_amd {

// CorrelationMap::fill, Models/Glm/PosteriorSamplers/CorrelationMap.cpp:41-59
static void build_correlation_map(const ba_engine &e, std::vector<int32_t> &start,
                                  std::vector<int32_t> &idx,
                                  std::vector<double> &cor) {
  const int p = e.p;
  const double n = e.n;
  std::vector<double> xbar(p), sd(p);
  for (int i = 0; i < p; ++i) xbar[i] = e.xsum[i] / n;
  auto cov = [&](int i, int j) {
    return (e.xtx[(size_t)j * p + i] + (-n) * xbar[i] * xbar[j]) / (n - 1);
  };
  for (int i = 0; i < p; ++i) {
    sd[i] = std::sqrt(cov(i, i));
    if (!(sd[i] > 0.0)) sd[i] = 1.0;
  }
  start.assign(p + 1, 0);
  idx.clear();
  cor.clear();
  for (int i = 0; i < p; ++i) {
    start[i] = (int32_t)idx.size();
    for (int j = 0; j < p; ++j) {
      if (j == i) continue;
      const double c = std::fabs(cov(i, j) / (sd[i] * sd[j]));
      if (c >= e.swap_threshold) {
        idx.push_back(j);
        cor.push_back(c);
      }
    }
  }
  start[p] = (int32_t)idx.size();
}

// Working capacity of a chain's LDS set: 16, 32, 48 or 64 variables (the sweep
// kernel is instantiated per capacity; smaller is faster).  The capacity is
// ADAPTIVE: launches run with the current capacity, a chain that outgrows it
// stops at a sweep boundary and is resumed by ba_sync() with the next size
// (escalate()), and the capacity follows the largest model seen.  A
// max_model_size prior caps it; ba_config.max_model_size_hint pins it.
static int lds_cap(const ba_engine &e) {   // largest capacity whose LDS set fits a CU
  int k = 64;
  while (k > 16 && ssvs_lds_layout(e.p, k).total > e.lds_per_cu) k -= 16;
  return k;
}
int cap_limit(const ba_engine &e) {
  int64_t need = std::min(64, e.p);
  if (e.max_model_size >= 0) need = std::min<int64_t>(need, std::max<int64_t>(1, e.max_model_size));
  const int k = (int)std::min<int64_t>(64, ((need + 15) / 16) * 16);
  return std::min(k, lds_cap(e));
}
static int choose_kcap(const ba_engine &e) {
  const int limit = cap_limit(e);
  if (e.cfg.max_model_size_hint > 0) {
    const int k = (int)std::min<int64_t>(64, (((int64_t)e.cfg.max_model_size_hint + 15) / 16) * 16);
    return std::min(k, lds_cap(e));
  }
  int start = 32;  // (ba_set_tuning: tests force early escalations)
  if (e.tune_kcap_start > 0) start = std::max(16, (e.tune_kcap_start / 16) * 16);
  return std::min(start, limit);
}

// Wavefronts per chain.  The proposal batches scale with the number of waves
// (64 proposals each, evaluated speculatively), and several resident waves per
// SIMD hide the gather / scalar-load latencies; the register budget of the
// 4-wave kernels only exists for capacities <= 32.  ba_set_tuning overrides.
int choose_waves(const ba_engine &e, int kcap) {
  {
    const int w = e.tune_waves;
    if (w == 1 || w == 2 || (w == 4 && kcap <= 32)) return w;
  }
  // Two wavefronts per chain at every engine size: the helper wave is worth more than
  // the second resident chain it displaces (measured on the C2 workload, sweeps/s with
  // 1 / 2 wavefronts: 1024 chains 28 / 41 M, 2048 30 / 36 M, 4096 31 / 43 M, 8192
  // 32 / 46 M), so chains beyond 4 per CU simply run in further rounds.
  (void)kcap;
  // The state-space path alternates ONE sweep with the state draw: no table survives a round
  // and there is no quiet sweep to fork, the helper wave has little to do; one wavefront per
  // chain measured better at every size (T=2000, p=100, us per round with 1 / 2 wavefronts:
  // 512 chains 144 / 144, 1024 167 / 172, 2048 279 / 304, 4096 545 / 590).
  // (the local-level round only: with the structural kernel behind it the same choice makes
  // THAT kernel slower -- 5.72 vs 5.06 ms per round at m = 13 -- for reasons not understood)
  if (e.data_kind == DATA_STATE_SPACE && !e.ssm_set) return 1;
  return 2;
}

int upload_shared(ba_engine *e) {
  if (!e->device_dirty) return BA_OK;
  const int p = e->p;
  if (!e->have_suf) return fail(BA_E_STATE, "no regression data set");
  if (!e->have_slab || !e->have_spike || !e->have_sigma)
    return fail(BA_E_STATE, "priors (slab, spike, sigma) must be set before sampling");
  const size_t pp = (size_t)p * p;
  std::vector<double> V(pp), l1(p), l0(p), scal(2);
  for (size_t i = 0; i < pp; ++i) V[i] = e->ominv[i] + e->xtx[i] * e->v_scale_want;
  e->v_scale = e->v_scale_want;
  // VariableSelectionPrior::ensure_log_probabilities,
  // VariableSelectionPrior.cpp:310-317
  for (int j = 0; j < p; ++j) {
    l1[j] = std::log(e->pi[j]);
    l0[j] = std::log(1 - e->pi[j]);
  }
  scal[0] = e->yty;
  scal[1] = e->n;
  HIP_TRY(e->dV.resize(pp));
  HIP_TRY(e->dA.resize(pp));
  HIP_TRY(e->db.resize(p));
  HIP_TRY(e->dl1.resize(p));
  HIP_TRY(e->dl0.resize(p));
  HIP_TRY(e->dpi.resize(p));
  HIP_TRY(e->dxty.resize(p));
  HIP_TRY(e->dscal.resize(2));
  hipStream_t s = e->stream;
  HIP_TRY(hipMemcpyAsync(e->dV.ptr, V.data(), pp * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->dA.ptr, e->ominv.data(), pp * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->db.ptr, e->b.data(), p * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->dl1.ptr, l1.data(), p * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->dl0.ptr, l0.data(), p * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->dpi.ptr, e->pi.data(), p * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->dxty.ptr, e->xty.data(), p * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->dscal.ptr, scal.data(), 16, hipMemcpyHostToDevice, s));
  e->cm_enabled = e->swap_threshold < 1.0;
  if (e->cm_enabled) {
    std::vector<int32_t> start, idx;
    std::vector<double> cor;
    build_correlation_map(*e, start, idx, cor);
    HIP_TRY(e->dcm_start.resize(start.size()));
    HIP_TRY(e->dcm_idx.resize(std::max<size_t>(1, idx.size())));
    HIP_TRY(e->dcm_cor.resize(std::max<size_t>(1, cor.size())));
    HIP_TRY(hipMemcpyAsync(e->dcm_start.ptr, start.data(), start.size() * 4, hipMemcpyHostToDevice, s));
    if (!idx.empty()) {
      HIP_TRY(hipMemcpyAsync(e->dcm_idx.ptr, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(e->dcm_cor.ptr, cor.data(), cor.size() * 8, hipMemcpyHostToDevice, s));
    }
  }
  HIP_TRY(hipStreamSynchronize(s));
  e->kcap = choose_kcap(*e);
  e->waves = choose_waves(*e, e->kcap);
  e->device_dirty = false;
  e->table_ok = false;
  e->model_ok = false;
  return BA_OK;
}

int alloc_chain_state(ba_engine *e) {
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p;
  if (e->state_ready && e->dgamma.count == C * p) return BA_OK;
  HIP_TRY(e->dgamma.resize(C * p));
  HIP_TRY(e->dbeta.resize(C * p));
  HIP_TRY(e->dsigsq.resize(C));
  HIP_TRY(e->dperm.resize(C * p));
  HIP_TRY(e->dpos.resize(C));
  HIP_TRY(e->dpos_sss.resize(C));
  HIP_TRY(e->dstatus.resize(C));
  HIP_TRY(e->dfail.resize(C));
  HIP_TRY(e->dtodo.resize(C));
  HIP_TRY(e->dtab_lp.resize(2 * C * p));    // two slots per chain (ssvs_params.h)
  HIP_TRY(e->dtab_kind.resize(2 * C * p));
  HIP_TRY(e->dtab_tag.resize(C));
  HIP_TRY(e->dmodel_tag.resize(C));
  e->model_ok = false;
  HIP_TRY(e->dran.resize(C));
  e->table_ok = false;
  e->model_ok = false;
  HIP_TRY(e->dmaxk.resize(1));
  HIP_TRY(e->dtrace_idx.resize(C));
  HIP_TRY(e->dinc.resize(C * p));
  HIP_TRY(e->dbsum.resize(C * p));
  HIP_TRY(e->dbsumsq.resize(C * p));
  HIP_TRY(e->dacc.resize(C * ACC_COUNT));
  HIP_TRY(e->dsummary.resize(3 * p + SUMMARY_SCALARS));
  // defaults: gamma = 0, beta = 0, sigsq = 1 (RegressionModel(xdim)), perm =
  // identity (seq<uint>(0, p-1), BregVsSampler.cpp:186), stream position 0
  std::vector<uint16_t> perm(C * p);
  for (size_t c = 0; c < C; ++c)
    for (size_t j = 0; j < p; ++j) perm[c * p + j] = (uint16_t)j;
  std::vector<double> ones(C, 1.0);
  hipStream_t s = e->stream;
  HIP_TRY(hipMemsetAsync(e->dgamma.ptr, 0, C * p, s));
  HIP_TRY(hipMemsetAsync(e->dbeta.ptr, 0, C * p * 8, s));
  HIP_TRY(hipMemcpyAsync(e->dsigsq.ptr, ones.data(), C * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->dperm.ptr, perm.data(), C * p * 2, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(e->dpos.ptr, 0, C * 8, s));
  HIP_TRY(hipMemsetAsync(e->dpos_sss.ptr, 0, C * 8, s));
  HIP_TRY(hipMemsetAsync(e->dstatus.ptr, 0, C * 4, s));
  HIP_TRY(hipMemsetAsync(e->dfail.ptr, 0, C * 4, s));
  HIP_TRY(hipMemsetAsync(e->dtodo.ptr, 0, C * 4, s));
  HIP_TRY(hipMemsetAsync(e->dmaxk.ptr, 0, 4, s));
  HIP_TRY(hipMemsetAsync(e->dtrace_idx.ptr, 0, C * 4, s));
  HIP_TRY(hipStreamSynchronize(s));
  e->state_ready = true;
  return ba_reset_summaries(e);
}

void fill_params(ba_engine *e, SsvsParams &P) {
  std::memset(&P, 0, sizeof(P));
  P.p = e->p;
  P.chains = e->cfg.chains;
  P.chain_first = 0;
  P.chain_count = e->cfg.chains;
  P.chain_offset = e->cfg.chain_offset;
  P.kcap = e->kcap;
  P.waves = e->waves;
  P.V = e->dV.ptr;
  P.A = e->dA.ptr;
  P.b = e->db.ptr;
  P.l1 = e->dl1.ptr;
  P.l0 = e->dl0.ptr;
  P.pi = e->dpi.ptr;
  if (e->data_kind == DATA_STATE_SPACE) {
    P.xty = e->dxty_c.ptr;
    P.xty_stride = e->p;
    P.yty = e->dyty_c.ptr;
    P.nobs = e->dnobs_c.ptr;
    P.suf_stride = 1;
  } else if (latent_data(e->data_kind) && e->dxty_c.count) {
    P.xty = e->dxty_c.ptr;      // X'z of every chain's own imputation
    P.xty_stride = e->p;
    P.yty = e->dscal.ptr;
    P.nobs = e->dscal.ptr + 1;
    P.suf_stride = 0;
  } else {
    P.xty = e->dxty.ptr;
    P.xty_stride = 0;
    P.yty = e->dscal.ptr;
    P.nobs = e->dscal.ptr + 1;
    P.suf_stride = 0;
  }
  P.prior_df = e->prior_df;
  P.prior_ss = e->prior_ss;
  P.sigma_max = e->sigma_max;
  P.swap_threshold = e->swap_threshold;
  P.max_model_size = e->max_model_size;
  const int mf = e->max_flips < 0 ? e->p : e->max_flips;
  P.max_flips = std::min(mf, e->p);
  P.draw_beta = e->draw_beta;
  P.draw_sigma = e->draw_sigma;
  P.cm_start = e->cm_enabled ? e->dcm_start.ptr : nullptr;
  P.cm_idx = e->dcm_idx.ptr;
  P.cm_cor = e->dcm_cor.ptr;
  P.gamma = e->dgamma.ptr;
  P.beta = e->dbeta.ptr;
  P.sigsq = e->dsigsq.ptr;
  P.perm = e->dperm.ptr;
  P.rng_pos = e->dpos.ptr;
  P.status = e->dstatus.ptr;
  P.failures = e->dfail.ptr;
  P.todo = e->dtodo.ptr;
  P.maxk = e->dmaxk.ptr;
  P.trace_idx = e->dtrace_idx.ptr;
  P.model_scratch = e->dmodel.ptr;
  P.table_lp = e->dtab_lp.ptr;
  P.table_kind = e->dtab_kind.ptr;
  P.table_tag = e->dtab_tag.ptr;
  P.table_keep = e->table_ok ? 1 : 0;
  P.model_tag = e->dmodel_tag.ptr;
  P.model_keep = e->model_ok ? 1 : 0;
  P.suf_changed = (e->data_kind == DATA_STATE_SPACE || latent_data(e->data_kind)) ? 1 : 0;
  P.run_limit = 0;
  P.ran = nullptr;
  P.model_scratch_stride = (int64_t)ssvs_scalar_layout(64).total;
  P.big_kcap = e->big_kcap;
  P.big_model = e->dbig_model.ptr;
  P.big_model_stride = e->big_kcap > 0 ? (int64_t)ssvs_scalar_layout(e->big_kcap).total : 0;
  P.big_xs = e->dbig_xs.ptr;
  P.seed_lo = (uint32_t)e->seed;
  P.seed_hi = (uint32_t)(e->seed >> 32);
  P.stream = 0;
  P.mode = e->cur_mode;
  P.walk_policy = e->tune_walk_policy >= 0 ? e->tune_walk_policy : 1;  // (see ssvs_params.h)
  P.rebuild_policy = e->tune_rebuild_policy;
  if (e->cur_mode == 1) {
    // SpikeSlabSampler: given sigma^2, no sigma draw, no swap move, own stream
    P.slab_scales = e->sss_slab_scales;
    P.stream = 3;
    P.rng_pos = e->dpos_sss.ptr;
    P.draw_sigma = 0;
    P.draw_beta = 1;
    P.cm_start = nullptr;
    P.max_flips = (e->sss_max_flips > 0) ? std::min(e->sss_max_flips, e->p) : e->p;
  }
  if (e->cur_mode == 1 && student_kind(e->data_kind) && !e->student_allow_selection)
    P.max_flips = 0;   // SpikeSlabSampler::allow_model_selection(false): no indicator draws
  if (e->cur_mode == 1 && column_service(e->data_kind) && e->cols.V.count) {
    // BinomialLogitSpikeSlabSampler: the sampler's own shuffle, every chain's own V
    // (which moves with the latent data: factors and tables are rebuilt)
    // (the Poisson, Student and quantile samplers drive the plain SpikeSlabSampler; the state space
    // logit family's observation model is BinomialLogitSpikeSlabSampler itself)
    P.mode = (e->data_kind == DATA_LOGIT || e->data_kind == DATA_SS_LOGIT) ? 2 : 1;
    if (e->data_kind == DATA_MLOGIT) {
      // MLVS::draw_inclusion_vector: its own fixed order, acceptance and empty model (mode 3)
      P.mode = 3;
      P.flip_order = e->dml_order.ptr;
      P.wss = e->dml_wss.ptr;
      if (!e->mlogit_select) P.max_flips = 0;   // MLVS::suppress_model_selection
    }
    P.V = e->cols.V.ptr;
    P.v_chain_stride = (int64_t)e->p * e->p;
    P.model_keep = 0;
    P.table_keep = 0;
    P.col_valid = e->cols.valid.ptr;
    P.col_words = e->cols.words;
    P.col_request = e->cols.wanted.ptr;
    P.v_diag = e->cols.vdiag.ptr;
  }
  if (e->cur_mode == 2) {
    // AdaptiveSpikeSlabRegressionSampler: own stream, no swap move
    P.mode = 0;
    P.stream = 4;
    P.rng_pos = e->dpos_ada.ptr;
    P.cm_start = nullptr;
  }
  P.ada_birth = e->dada_birth.ptr;
  P.ada_death = e->dada_death.ptr;
  P.ada_iter = e->dada_iter.ptr;
  P.ada_step = e->ada_step;
  P.ada_target = e->ada_target;
  P.ada_max_flips = e->ada_max_flips;
  P.q_in = P.q_out = nullptr;
  P.q_error = nullptr;
  P.trace_row0 = -1;
  P.snap_gamma = nullptr;
  P.adaptive = (e->cur_mode == 2) ? 1 : 0;
  P.ada_ws = e->dada_ws.ptr;
  P.inc_count = e->dinc.ptr;
  P.beta_sum = e->dbsum.ptr;
  P.beta_sumsq = e->dbsumsq.ptr;
  P.acc = e->dacc.ptr;
  P.trace_sigsq = e->dtr_sig.ptr;
  P.trace_logp = e->dtr_logp.ptr;
  P.trace_k = e->dtr_k.ptr;
  P.trace_stride = e->trace_stride;
  P.rec_idx = e->drec_idx.ptr;
  P.rec_beta = e->drec_beta.ptr;
  P.rec_cap = e->rec_cap;
}

// ---- models of more than 64 variables: the HBM-resident kernel -------------------
enum { BIG_KCAP_MAX = 1024 };
// largest capacity that can ever be needed (0: the LDS kernel covers everything)
static int big_limit(const ba_engine &e) {
  int64_t need = e.p;
  if (e.max_model_size >= 0) need = std::min<int64_t>(need, e.max_model_size);
  if (need <= 64) return 0;
  return (int)std::min<int64_t>(BIG_KCAP_MAX, ((need + 63) / 64) * 64);
}
static int ensure_big_buffers(ba_engine *e) {
  const size_t C = (size_t)e->cfg.chains, kc = (size_t)e->big_kcap;
  const size_t want_model = 2 * C * ssvs_scalar_layout(e->big_kcap).total;
  const size_t want_xs = C * 2 * kc * 64;
  if (e->dbig_model.count != want_model) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(e->dbig_model.resize(want_model));
    HIP_TRY(e->dbig_xs.resize(want_xs));
  }
  const SsvsBigLds lay = ssvs_big_lds_layout(e->p, e->big_kcap);
  if (lay.total > e->lds_per_cu)
    return fail(BA_E_MODEL_TOO_LARGE, "the model does not fit the large-model kernel's LDS working set");
  // the draw record holds rec_cap variables per draw: widen it (keeping what is recorded)
  if (e->drec_idx.count > 0 && e->rec_cap < e->big_kcap) {
    const size_t rows = C * (size_t)e->trace_stride, oc = (size_t)e->rec_cap;
    DevBuf<uint16_t> ni;
    DevBuf<double> nb;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(ni.resize(rows * kc));
    HIP_TRY(nb.resize(rows * kc));
    HIP_TRY(hipMemcpy2DAsync(ni.ptr, kc * 2, e->drec_idx.ptr, oc * 2, oc * 2, rows, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpy2DAsync(nb.ptr, kc * 8, e->drec_beta.ptr, oc * 8, oc * 8, rows, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    std::swap(ni.ptr, e->drec_idx.ptr);
    std::swap(ni.count, e->drec_idx.count);
    std::swap(nb.ptr, e->drec_beta.ptr);
    std::swap(nb.count, e->drec_beta.count);
    e->rec_cap = e->big_kcap;
  }
  return BA_OK;
}
// one launch of the sweep: the LDS kernel for every chain it can hold, and --
// once any chain has outgrown it -- the HBM-resident kernel right behind it for
// the chains the first one parked (status CHAIN_MODEL_TOO_LARGE)
hipError_t launch_sweeps(ba_engine *e, const SsvsParams &P, int nsweeps) {
  hipError_t err = (e->cur_mode == 2) ? launch_ssvs_adaptive(e->stream, P, nsweeps)
                                      : launch_ssvs_sweep(e->stream, P, nsweeps);
  if (err == hipSuccess && e->big_active) err = launch_ssvs_big(e->stream, P, 0);
  return err;
}
// the chains parked by the last launches need (more) large-model capacity;
// returns 1 when nothing more can be done (the status stays an error)
int grow_big(ba_engine *e, int *stuck) {
  *stuck = 0;
  const int bl = big_limit(*e);
  if (bl == 0) { *stuck = 1; return BA_OK; }
  if (!e->big_active) {
    e->big_active = true;
    if (e->big_kcap == 0) e->big_kcap = std::min(bl, 128);
  } else {
    if (e->big_kcap >= bl) { *stuck = 1; return BA_OK; }
    e->big_kcap = std::min(bl, e->big_kcap * 2);
  }
  return ensure_big_buffers(e);
}

// Resume chains that outgrew the capacity of the launch they were in, with the
// next larger capacity; then follow the largest model size seen.
static int escalate(ba_engine *e, std::vector<int32_t> &st) {
  const size_t C = (size_t)e->cfg.chains;
  for (;;) {
    {
      bool served = false;
      int rc = serve_columns(e, st, &served);
      if (rc) return rc;
      if (served) continue;
    }
    bool any = false;
    for (size_t c = 0; c < C; ++c) any = any || (st[c] == CHAIN_MODEL_TOO_LARGE);
    if (!any) return BA_OK;
    if (e->cfg.max_model_size_hint > 0) return BA_OK;  // stays an error
    if (e->kcap >= cap_limit(*e)) {
      // (MLVS has no large-model sweep: more than 64 included variables stay an error)
      if (e->data_kind == DATA_MLOGIT) return BA_OK;
      // beyond the LDS kernel: the parked chains go to the HBM-resident one
      int stuck = 0;
      int rc = grow_big(e, &stuck);
      if (rc) return rc;
      if (stuck) return BA_OK;
      SsvsParams P;
      fill_params(e, P);
      HIP_TRY(launch_ssvs_big(e->stream, P, 0));
      HIP_TRY(hipStreamSynchronize(e->stream));
      HIP_TRY(hipMemcpy(st.data(), e->dstatus.ptr, C * 4, hipMemcpyDeviceToHost));
      continue;
    }
    e->kcap += 16;
    e->waves = choose_waves(*e, e->kcap);
    for (size_t c = 0; c < C; ++c)
      if (st[c] == CHAIN_MODEL_TOO_LARGE) st[c] = CHAIN_OK;
    HIP_TRY(hipMemcpyAsync(e->dstatus.ptr, st.data(), C * 4, hipMemcpyHostToDevice, e->stream));
    SsvsParams P;
    fill_params(e, P);
    HIP_TRY(launch_sweeps(e, P, 0));   // runs the sweeps still owed
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(st.data(), e->dstatus.ptr, C * 4, hipMemcpyDeviceToHost));
  }
}

// the pinned staging buffer of the accessors' batched copies (engine struct)
hipError_t pinned_reserve(ba_engine *e, size_t bytes) {
  if (bytes <= e->pinned_bytes) return hipSuccess;
  if (e->pinned) (void)hipHostFree(e->pinned);
  e->pinned = nullptr;
  e->pinned_bytes = 0;
  const size_t want = std::max<size_t>(bytes, (size_t)1 << 16);
  hipError_t err = hipHostMalloc(&e->pinned, want, hipHostMallocDefault);
  if (err == hipSuccess) e->pinned_bytes = want;
  return err;
}

// (debugging sessions, ba_ss_set_tuning(e, 6): what THIS engine's round kernel noted, printed
// when one of its chains stops; the buffer lives on the engine's device)
static void dump_round_debug(ba_engine *e) {
  if (!e->round_debug || e->dround_debug.count == 0 || set_device(e)) return;
  DevBuf<int32_t> &g_round_debug = e->dround_debug;
  int32_t h[16 * 17];
  if (hipMemcpy(h, g_round_debug.ptr, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return;
  std::fprintf(stderr, "round kernel: %d sums that are not numbers\n", h[0]);
  for (int i = 0; i < std::min(h[0], 15); ++i) {
    const int32_t *o = h + 16 + i * 16;
    std::fprintf(stderr, "  chain %d round %d of %d variable %d row %d tile %d slot %d members %d bits %08x%08x\n", o[0], o[1], o[9],
                 o[2], o[3], o[4], o[5], o[6], (unsigned)o[7], (unsigned)o[8]);
  }
  {
    double d[32];
    if (hipMemcpy(d, g_round_debug.ptr + 16 * 17, sizeof d, hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int i = 0; i < std::min(h[1], 4); ++i)
      std::fprintf(stderr, "  stopped in the state draw: chain %g round %g status %g sigsq %.17g level_sigsq %.17g prep_n %g level_sumsq %.17g level_n %g\n",
                   d[i * 8], d[i * 8 + 1], d[i * 8 + 2], d[i * 8 + 3], d[i * 8 + 4], d[i * 8 + 5], d[i * 8 + 6], d[i * 8 + 7]);
  }
  (void)hipMemset(g_round_debug.ptr, 0, (16 * 17 + 64) * 4);
}

int check_chain_status(ba_engine *e) {
  const size_t C = (size_t)e->cfg.chains;
  if (!e->state_ready) return BA_OK;
  std::vector<int32_t> st(C);
  // the status words and the launches' largest model in ONE round trip
  const bool follow = e->cfg.max_model_size_hint <= 0 && e->kcap > 0;
  HIP_TRY(pinned_reserve(e, C * 4 + 16));
  int32_t *hst = (int32_t *)e->pinned, *hmaxk = hst + C;
  HIP_TRY(hipMemcpyAsync(hst, e->dstatus.ptr, C * 4, hipMemcpyDeviceToHost, e->stream));
  if (follow) HIP_TRY(hipMemcpyAsync(hmaxk, e->dmaxk.ptr, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::memcpy(st.data(), hst, C * 4);
  bool all_ok = true;
  for (size_t c = 0; c < C; ++c) all_ok = all_ok && st[c] == CHAIN_OK;
  {
    int rc = BA_OK;
    if (!all_ok) rc = e->data_kind == DATA_STATE_SPACE ? ss_escalate(e, st) : escalate(e, st);
    if (rc) return rc;
    // capacity follows the models: room for growth, no more
    if (follow) {
      int32_t maxk = *hmaxk;
      if (all_ok) {
        HIP_TRY(hipMemsetAsync(e->dmaxk.ptr, 0, 4, e->stream));   // (in order before the next launch)
      } else {   // (a catch-up has run since the copy above)
        HIP_TRY(hipMemcpyAsync(&maxk, e->dmaxk.ptr, 4, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemsetAsync(e->dmaxk.ptr, 0, 4, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
      }
      const int want = std::min(cap_limit(*e), std::max(16, ((maxk + 8 + 15) / 16) * 16));
      if (maxk > 0 && want < e->kcap) {
        e->kcap = want;
        e->waves = choose_waves(*e, e->kcap);
      }
      if (maxk > 0 && maxk <= 56) e->big_active = false;  // every chain is back in the LDS kernel
    }
  }
  for (size_t c = 0; c < C; ++c) {
    if (st[c] != CHAIN_OK) {
      char buf[64];
      std::snprintf(buf, sizeof buf, " (chain %lld)",
                    (long long)(e->cfg.chain_offset + (int64_t)c));
      dump_round_debug(e);
      {  // (and which chains)
        int bad = 0;
        for (size_t d = 0; d < C; ++d) bad += st[d] != CHAIN_OK;
        if (e->round_debug && e->dround_debug.count) {
          std::fprintf(stderr, "  %d chains stopped:", bad);
          for (size_t d = 0; d < C; ++d) if (st[d] != CHAIN_OK) std::fprintf(stderr, " %zu(%d)", d, st[d]);
          std::fprintf(stderr, "\n");
        }
      }
      if (e->data_kind == DATA_MLOGIT && st[c] == CHAIN_MODEL_TOO_LARGE)
        return fail(BA_E_MODEL_TOO_LARGE, std::string("The multinomial logit sampler holds models of up to 64 included "
                                                      "variables; a chain needs more.") + buf);
      return fail(status_code(st[c]), std::string(status_message(st[c])) + buf);
    }
  }
  return BA_OK;
}

int set_device(const ba_engine *e) {
  HIP_TRY(hipSetDevice(e->cfg.device));
  return BA_OK;
}

// ---- a second stream that really runs beside the first --------------------------------
// HIP maps streams onto a few hardware queues; two streams on one queue run one after the
// other, whatever the program meant (measured: the bsts round 207 instead of 167 us when
// the engine's two streams happen to share a queue, which depends on how many streams the
// process created before).  So a candidate is TESTED: a kernel on the main stream waits
// (bounded: 20 ms) for a flag that a kernel on the candidate sets; the first candidate whose
// kernel gets through while the other is waiting is kept.
static __global__ void stream_probe_wait_kernel(volatile int *flag, int *saw, long long ticks) {
  const long long t0 = wall_clock64();
  int v = 0;
  while ((v = *flag) == 0 && wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
  *saw = v;
}
static __global__ void stream_probe_set_kernel(volatile int *flag) { *flag = 1; }

int concurrent_stream(ba_engine *e, hipStream_t *out) {
  DevBuf<int32_t> buf;
  HIP_TRY(buf.resize(2));
  hipStream_t tried[8];
  int ntried = 0;
  hipStream_t good = nullptr;
  for (; ntried < 8 && !good; ++ntried) {
    hipStream_t c = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&c, hipStreamNonBlocking));
    tried[ntried] = c;
    HIP_TRY(hipMemsetAsync(buf.ptr, 0, 8, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // (wall_clock64 counts at 100 MHz: 2e6 ticks = 20 ms)
    hipLaunchKernelGGL(stream_probe_wait_kernel, dim3(1), dim3(1), 0, e->stream, (volatile int *)buf.ptr,
                       (int *)buf.ptr + 1, 2000000ll);
    hipLaunchKernelGGL(stream_probe_set_kernel, dim3(1), dim3(1), 0, c, (volatile int *)buf.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipStreamSynchronize(c));
    int32_t saw = 0;
    HIP_TRY(hipMemcpy(&saw, buf.ptr + 1, 4, hipMemcpyDeviceToHost));
    if (saw) good = c;
  }
  // (none ran beside the main stream: the last one serves, in sequence)
  if (!good) good = tried[ntried - 1];
  for (int i = 0; i < ntried; ++i)
    if (tried[i] != good) (void)hipStreamDestroy(tried[i]);
  *out = good;
  return BA_OK;
}

// ---- pipelined sweeps ---------------------------------------------------------------
// The end of a pipeline: the main stream waits for the other one, so that whatever is
// enqueued next comes after every sweep launch; a workgroup that waited for its chain in
// vain (it cannot happen while the chains fit the machine; bounded all the same) is an error.
int pipe_join(ba_engine *e) {
  if (!e->pipe.on) return BA_OK;
  e->pipe.on = false;
  e->pipe.k = 0;
  e->pipe.groups = false;
  HIP_TRY(hipEventRecord(e->pipe.join_ev, e->pipe.stream));
  HIP_TRY(hipStreamWaitEvent(e->stream, e->pipe.join_ev, 0));
  return BA_OK;
}
// (force: read the word whatever the flag says -- the look-ahead's batches, whose launches
// and checks interleave)
static int pipe_check(ba_engine *e, bool force = false) {
  if (e->pipe.err.count == 0 || (!force && !e->pipe.unchecked)) return BA_OK;
  e->pipe.unchecked = false;
  int32_t err = 0;
  HIP_TRY(hipMemcpy(&err, e->pipe.err.ptr, 4, hipMemcpyDeviceToHost));
  if (err) {
    HIP_TRY(hipMemset(e->pipe.err.ptr, 0, 4));
    return fail(BA_E_HIP, "a pipelined sweep launch waited for a chain in vain");
  }
  return BA_OK;
}
// the second stream and its events, at the first launch that needs them
static int pipe_open(ba_engine *e) {
  if (e->pipe.stream) return BA_OK;
  int rc = concurrent_stream(e, &e->pipe.stream);
  if (rc) return rc;
  for (int i = 0; i < 4; ++i) HIP_TRY(hipEventCreateWithFlags(&e->pipe.ev[i], hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&e->pipe.join_ev, hipEventDisableTiming));
  return BA_OK;
}
// How many chains' workgroups the device holds at once for a sweep launch of `lds` bytes per
// workgroup (*resident; 0: not even one fits a CU), and whether that is every chain of the
// engine: what lets consecutive launches hand chains over.
static bool chains_fit(const ba_engine *e, size_t lds, int *resident = nullptr) {
  const int r = lds > e->lds_per_cu ? 0 : (int)std::min<size_t>(4, e->lds_per_cu / lds) * e->cu_count;
  if (resident) *resident = r;
  return e->cfg.chains <= r;
}

int all_chains_ok(ba_engine *e, bool *ok) {
  const size_t C = (size_t)e->cfg.chains;
  std::vector<int32_t> st(C);
  HIP_TRY(hipMemcpy(st.data(), e->dstatus.ptr, C * 4, hipMemcpyDeviceToHost));
  *ok = true;
  for (size_t c = 0; c < C; ++c) *ok = *ok && st[c] == CHAIN_OK;
  return BA_OK;
}
// (the statuses and the sweeps booked as owed belong to the dropped launches -- a chain that
// stopped in them stopped after the point the chains go back to -- and so do the proposal
// tables and the models' factors)
int drop_launched_ahead(ba_engine *e) {
  const size_t C = (size_t)e->cfg.chains;
  HIP_TRY(hipMemsetAsync(e->dstatus.ptr, 0, C * 4, e->stream));
  HIP_TRY(hipMemsetAsync(e->dtodo.ptr, 0, C * 4, e->stream));
  e->table_ok = false;
  e->model_ok = false;
  return BA_OK;
}

// ---- look-ahead serving (ba_draw_next) ------------------------------------------
static int sweep_impl(ba_engine *e, int32_t nsweeps, bool record = true, int la_half = -1);
static int read_record(ba_engine *e, int64_t c, int row0, int nrows, uint8_t *gamma,
                       double *beta, double *sigsq);
static int read_record_row_all(ba_engine *e, int row, uint8_t *gamma, double *beta, double *sigsq);

static void la_discard(ba_engine *e) {
  e->la.avail = e->la.served = 0;
  e->la.cache.clear();
  e->la.synced = false;
}

static int la_redo_batch(ba_engine *e);

// the batch being served is complete and sound; a pipelined batch in which a chain stopped
// (capacity, an error) is run again the old way -- same draws -- where those are dealt with
static int la_wait(ba_engine *e) {
  if (e->la.synced) return BA_OK;
  if (e->la.cur_piped) {
    HIP_TRY(hipEventSynchronize(e->la.done[e->la.slot]));
    int rc = pipe_check(e, true);
    bool ok = true;
    if (!rc) rc = all_chains_ok(e, &ok);
    if (!rc && !ok) rc = la_redo_batch(e);
    if (rc) return rc;
  } else {
    HIP_TRY(hipStreamSynchronize(e->stream));
    int rc = check_chain_status(e);
    if (rc) return rc;
  }
  e->la.synced = true;
  return BA_OK;
}

// the draw ba_draw_next is serving, for one chain: from the host copy of the
// chain's rows of the batch (fetched at the chain's first read in the batch)
static int la_read(ba_engine *e, int64_t c, uint8_t *gamma, double *beta, double *sigsq) {
  int rc = la_wait(e);
  if (rc) return rc;
  const size_t p = (size_t)e->p, cap = (size_t)e->rec_cap, n = (size_t)e->la.avail;
  auto it = e->la.cache.find(c);
  if (it == e->la.cache.end()) {
    ba_engine::La::Rows r;
    r.k.resize(n); r.sig.resize(n); r.beta.resize(n * cap); r.idx.resize(n * cap);
    const size_t base = (size_t)c * e->trace_stride + (size_t)e->la.slot * (size_t)e->la.len;
    HIP_TRY(hipMemcpy(r.k.data(), e->dtr_k.ptr + base, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.sig.data(), e->dtr_sig.ptr + base, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.idx.data(), e->drec_idx.ptr + base * cap, n * cap * 2, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.beta.data(), e->drec_beta.ptr + base * cap, n * cap * 8, hipMemcpyDeviceToHost));
    it = e->la.cache.emplace(c, std::move(r)).first;
  }
  const ba_engine::La::Rows &r = it->second;
  const size_t row = (size_t)e->la.served - 1;
  const int k = (int)r.k[row];
  if (k < 0 || (size_t)k > cap) return fail(BA_E_STATE, "corrupt draw record");
  if (gamma) std::memset(gamma, 0, p);
  if (beta) std::memset(beta, 0, p * 8);
  for (int m = 0; m < k; ++m) {
    const size_t j = r.idx[row * cap + m];
    if (j >= p) return fail(BA_E_STATE, "corrupt draw record");
    if (gamma) gamma[j] = 1;
    if (beta) beta[j] = r.beta[row * cap + m];
  }
  if (sigsq) *sigsq = r.sig[row];
  return BA_OK;
}

// What a chain's state is, so that a snapshot of it can be rewound to -- THE list: the live
// array, its two snapshot sets, the elements per chain and the SsvsParams member through which
// a pipelined batch's workgroups save the same array on entry (ssvs_kernel.hip).  A per-chain
// array that a sweep changes belongs here, and nowhere else on the host.
template <class F>
static int la_snap_fields(ba_engine *e, F f) {
  const size_t p = (size_t)e->p;
  ba_engine::La::Snap &S = e->la.snap;
  hipError_t la_snapshot = hipSuccess;
  auto field = [&](auto &live, auto &snap, size_t n, auto member) {
    if (la_snapshot == hipSuccess) la_snapshot = f(live, snap, n, member);
  };
  field(e->dgamma, S.gamma, p, &SsvsParams::snap_gamma);
  field(e->dbeta, S.beta, p, &SsvsParams::snap_beta);
  field(e->dsigsq, S.sigsq, 1, &SsvsParams::snap_sigsq);
  field(e->dperm, S.perm, p, &SsvsParams::snap_perm);
  field(e->dpos, S.pos, 1, &SsvsParams::snap_pos);
  field(e->dfail, S.fail, 1, &SsvsParams::snap_fail);
  field(e->dinc, S.inc, p, &SsvsParams::snap_inc);
  field(e->dbsum, S.bsum, p, &SsvsParams::snap_bsum);
  field(e->dbsumsq, S.bsumsq, p, &SsvsParams::snap_bsumsq);
  field(e->dacc, S.acc, ACC_COUNT, &SsvsParams::snap_acc);
  HIP_TRY(la_snapshot);
  return BA_OK;
}
static int la_snap_alloc(ba_engine *e) {
  const size_t C = (size_t)e->cfg.chains;
  return la_snap_fields(e, [&](auto &, auto &snap, size_t n, auto) { return snap.resize(2 * C * n); });
}
// snapshot set `set` (0 / 1) <-> the live chain state
int la_copy(ba_engine *e, bool save, int set) {
  const size_t C = (size_t)e->cfg.chains;
  if (save) {
    int rc = la_snap_alloc(e);
    if (rc) return rc;
  }
  return la_snap_fields(e, [&](auto &live, auto &snap, size_t n, auto) {
    auto *held = snap.ptr + (size_t)set * C * n;
    return hipMemcpyAsync(save ? held : live.ptr, save ? live.ptr : held, C * n * sizeof(*held),
                          hipMemcpyDeviceToDevice, e->stream);
  });
}

// every launch of the look-ahead has finished (the main stream has caught up with the other
// one) and nothing is ahead any more
static int la_quiesce(ba_engine *e) {
  e->la.ahead = false;
  int rc = pipe_join(e);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BA_OK;
}

// A pipelined batch met a chain that cannot go on as it is (model beyond the launch's
// capacity, an error): everything in flight is dropped, the chains go back to the batch's
// start and the batch runs again the way batches ran before they overlapped -- the same
// draws, with the escalation / error report of that path.  Overlap stays off afterwards.
static int la_redo_batch(ba_engine *e) {
  int rc = la_quiesce(e);
  if (rc) return rc;
  const int served = e->la.served;
  rc = la_copy(e, false, e->la.slot);
  if (!rc) rc = drop_launched_ahead(e);
  if (rc) return rc;
  e->la.pipe = false;
  e->la.cur_piped = false;
  e->la.slot = 0;
  rc = la_copy(e, true, 0);
  if (!rc) rc = sweep_impl(e, e->la.len);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->la.cache.clear();
  e->la.served = served;
  return check_chain_status(e);
}

// Something other than ba_draw_next is about to touch the engine while draws of
// the look-ahead batch are still unserved: put the chains where the caller has
// seen them -- the batch's start, replayed up to the last draw handed out (same
// stream positions, so the same draws).
int la_rewind(ba_engine *e) {
  if (e->la.served >= e->la.avail && !e->la.ahead) {
    la_discard(e);
    return BA_OK;
  }
  HIP_TRY(hipSetDevice(e->cfg.device));
  int rc = la_quiesce(e);
  if (rc) return rc;
  const bool all_served = e->la.served >= e->la.avail;
  const int replay = all_served ? 0 : e->la.served;
  // where to go back to: the start of the batch being served, or -- every draw of it
  // served, the next one already run -- the start of that next one
  const int set = all_served ? (e->la.slot ^ 1) : e->la.slot;
  const bool piped = e->la.cur_piped;
  la_discard(e);
  if (piped) {
    rc = pipe_check(e, true);
    if (!rc) rc = drop_launched_ahead(e);
  } else {
    rc = check_chain_status(e);   // (one launch, run to its end: its stops are dealt with, not dropped)
  }
  if (rc) return rc;
  rc = la_copy(e, false, piped ? set : 0);
  if (rc) return rc;
  e->la.cur_piped = false;
  e->la.slot = 0;
  e->table_ok = false;   // (either way the chains are no longer where the launch left them)
  e->model_ok = false;
  if (replay > 0) {
    rc = sweep_impl(e, replay, /*record=*/false);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = check_chain_status(e);
  }
  return rc;
}

}  // namespace boom_amd

extern "C" {

const char *ba_last_error(void) { return g_error.c_str(); }

int ba_engine_create(const ba_config *cfg, ba_engine **out) {
  if (!cfg || !out) return fail(BA_E_INVALID, "null argument");
  if (cfg->chains <= 0) return fail(BA_E_INVALID, "chains must be positive");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev <= 0)
    return fail(BA_E_HIP, "no HIP device visible: boom_amd has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev)
    return fail(BA_E_INVALID, "device ordinal out of range");
  ba_engine *e = new ba_engine();
  e->cfg = *cfg;
  e->seed = cfg->seed;
  hipError_t err = hipSetDevice(cfg->device);
  if (err == hipSuccess) err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
  if (err != hipSuccess) {
    delete e;
    return fail(BA_E_HIP, std::string("stream creation: ") + hipGetErrorString(err));
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) {
    e->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (prop.maxSharedMemoryPerMultiProcessor > 0)
      e->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
  }
  // the shuffle's LDS-exchange search needs same-address exchanges resolved in
  // lane order; refuse a device that does not
  {
    int *dbad = nullptr, hbad = -1;
    err = hipMalloc((void **)&dbad, sizeof(int));
    if (err == hipSuccess) err = hipMemsetAsync(dbad, 0, sizeof(int), e->stream);
    if (err == hipSuccess) err = launch_lds_exchange_order(e->stream, dbad);
    if (err == hipSuccess) err = hipMemcpyAsync(&hbad, dbad, sizeof(int), hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (dbad) (void)hipFree(dbad);
    if (err != hipSuccess || hbad != 0) {
      (void)hipStreamDestroy(e->stream);
      delete e;
      if (err != hipSuccess) return fail(BA_E_HIP, std::string("device self-test: ") + hipGetErrorString(err));
      return fail(BA_E_HIP, "device self-test: LDS exchanges are not resolved in lane order on this device");
    }
  }
  *out = e;
  return BA_OK;
}

void ba_engine_destroy(ba_engine *e) {
  if (!e) return;
  (void)hipSetDevice(e->cfg.device);
  if (e->stream2) {
    (void)hipStreamSynchronize(e->stream2);
    (void)hipStreamDestroy(e->stream2);
  }
  if (e->ssf_stream) {
    (void)hipStreamSynchronize(e->ssf_stream);
    (void)hipStreamDestroy(e->ssf_stream);
  }
  for (int i = 0; i < 2; ++i) {
    if (e->la.done[i]) (void)hipEventDestroy(e->la.done[i]);
    if (e->ssla.done[i]) (void)hipEventDestroy(e->ssla.done[i]);
  }
  if (e->pipe.stream) {
    (void)hipStreamSynchronize(e->pipe.stream);
    (void)hipStreamDestroy(e->pipe.stream);
    for (int i = 0; i < 4; ++i) (void)hipEventDestroy(e->pipe.ev[i]);
    (void)hipEventDestroy(e->pipe.join_ev);
  }
  if (e->ev_state) (void)hipEventDestroy(e->ev_state);
  if (e->pinned) (void)hipHostFree(e->pinned);
  for (int i = 0; i < 2; ++i)
    if (e->ev_prep[i]) (void)hipEventDestroy(e->ev_prep[i]);
  if (e->stream) {
    (void)hipStreamSynchronize(e->stream);
    (void)hipStreamDestroy(e->stream);
  }
  delete e;
}

int ba_engine_info(const ba_engine *e, int32_t *device, int32_t *chains,
                   int32_t *p) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (device) *device = e->cfg.device;
  if (chains) *chains = e->cfg.chains;
  if (p) *p = e->p;
  return BA_OK;
}

// (work the caller puts on the stream after this call comes after every launch of the engine:
// sweeps that overlap on the engine's second stream are joined first)
void *ba_stream(ba_engine *e) {
  if (!e) return nullptr;
  if (hipSetDevice(e->cfg.device) != hipSuccess) return nullptr;
  if (pipe_join(e) != BA_OK) return nullptr;
  return (void *)e->stream;
}

// ---- measurement: device time per kernel class (ktimer.h) ------------------------
int32_t ba_kernel_classes(void) { return KT_CLASSES; }

const char *ba_kernel_class_name(int32_t cls) {
  static const char *const names[KT_CLASSES] = {
      "ssvs_sweep_kernel", "ssvs_big_kernel", "ssvs_adaptive_kernel", "kalman_simsmooth_kernel",
      "ssm_simsmooth_kernel", "atb_mfma_kernel", "probit_impute_kernel", "logit_impute_kernel",
      "xtwx_cols_kernel<false>+plain_reduce_kernel", "xtwx_cols_kernel<true>+xtwx_cols_reduce_kernel",
      "xtx_mfma_kernel+plane_sum_kernel+col_reduce_kernel", "poisson_impute_kernel",
      "kalman_prepare_kernel", "ss_round_kernel", "student_impute_kernel", "student_sigma_nu_kernel",
      "quantile_impute_kernel", "mlogit_impute_kernel", "student_ss_kernels", "poisson_ss_kernels", "logit_ss_kernels",
      "student_trend_kernels", "ss_filter_kernel", "ar_spike_kernel", "reg_holiday_kernels"};
  return (cls >= 0 && cls < KT_CLASSES) ? names[cls] : "";
}

int ba_set_kernel_timing(ba_engine *e, int32_t enabled) {
  ENGINE_PROLOGUE(e);
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->kt.collect();
  e->kt_enabled = enabled != 0;
  e->kt_overlap = enabled == 2;
  g_kt = e->kt_enabled ? &e->kt : nullptr;
  return BA_OK;
}

int ba_get_kernel_times(ba_engine *e, double *ms, int64_t *launches, int32_t reset) {
  ENGINE_PROLOGUE(e);
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->kt.collect();
  for (int c = 0; c < KT_CLASSES; ++c) {
    if (ms) ms[c] = e->kt.ms[c];
    if (launches) launches[c] = e->kt.launches[c];
    if (reset) { e->kt.ms[c] = 0; e->kt.launches[c] = 0; }
  }
  return BA_OK;
}

// ---------------------------------------------------------------- data
static int set_dimension(ba_engine *e, int p) {
  if (p <= 0 || p > 65535)
    return fail(BA_E_INVALID, "number of predictors must be in [1, 65535]");
  if (e->p != p) {
    e->p = p;
    e->have_slab = e->have_spike = false;
    e->state_ready = false;
  }
  return BA_OK;
}

int ba_upload_regression_suf(ba_engine *e, int32_t p, const double *xtx,
                             const double *xty, double yty, double n,
                             double ybar, const double *xbar) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!xtx || !xty || !xbar) return fail(BA_E_INVALID, "null argument");
  int rc = set_dimension(e, p);
  if (rc) return rc;
  e->xtx.assign(xtx, xtx + (size_t)p * p);
  e->xty.assign(xty, xty + p);
  e->xsum.resize(p);
  for (int j = 0; j < p; ++j) e->xsum[j] = xbar[j] * n;
  e->yty = yty;
  e->n = n;
  e->sumy = ybar * n;
  e->have_suf = true;
  e->device_dirty = true;
  e->data_kind = DATA_REGRESSION;   // (the binomial, Poisson, Student-t and state-space setters say otherwise after this)
  return BA_OK;
}

int ba_build_suf_from_xy_device(ba_engine *e, int64_t n, int32_t p,
                                const void *X_device, const void *y_device) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!X_device || !y_device) return fail(BA_E_INVALID, "null argument");
  if (n <= 0) return fail(BA_E_INVALID, "n must be positive");
  int rc = set_dimension(e, p);
  if (rc) return rc;
  HIP_TRY(e->dxtx.resize((size_t)p * p));
  HIP_TRY(e->dxty.resize(p));
  HIP_TRY(e->dxsum.resize(p));
  HIP_TRY(e->dsufscal.resize(2));
  DevBuf<double> planes;  // split-K partial products (freed after the sync below)
  const int slices = suf_row_slices(n, p);
  if (slices > 1) HIP_TRY(planes.resize((size_t)slices * p * p));
  rc = launch_suf_from_xy(e->stream, n, p, (const double *)X_device,
                          (const double *)y_device, e->dxtx.ptr, e->dxty.ptr,
                          e->dsufscal.ptr, e->dxsum.ptr, planes.ptr);
  if (rc) return fail(BA_E_HIP, "suf kernel launch failed");
  e->xtx.resize((size_t)p * p);
  e->xty.resize(p);
  e->xsum.resize(p);
  double sc[2];
  HIP_TRY(hipMemcpyAsync(e->xtx.data(), e->dxtx.ptr, (size_t)p * p * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(e->xty.data(), e->dxty.ptr, (size_t)p * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(e->xsum.data(), e->dxsum.ptr, (size_t)p * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(sc, e->dsufscal.ptr, 16, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->yty = sc[0];
  e->sumy = sc[1];
  e->n = (double)n;
  e->have_suf = true;
  e->device_dirty = true;
  e->data_kind = DATA_REGRESSION;   // (the binomial, Poisson, Student-t and state-space setters say otherwise after this)
  return BA_OK;
}

// ---- row-sharded build: partial statistics of a shard of rows, summed by the
// caller over its ranks (one all-reduce), then installed on every rank
size_t ba_suf_block_size(int32_t p) { return (size_t)p * p + 2 * (size_t)p + 2; }

int ba_suf_partial_device(ba_engine *e, int64_t n_rows, int32_t p, const void *X_device,
                          const void *y_device, void *block_device) {
  ENGINE_PROLOGUE(e);
  if (!X_device || !y_device || !block_device) return fail(BA_E_INVALID, "null argument");
  if (n_rows <= 0 || p <= 0 || p > 65535) return fail(BA_E_INVALID, "bad shard dimensions");
  double *blk = (double *)block_device;
  DevBuf<double> planes;
  const int slices = suf_row_slices(n_rows, p);
  if (slices > 1) HIP_TRY(planes.resize((size_t)slices * p * p));
  // block layout: [XtX p*p | Xty p | yty, sum y | column sums of X p]
  int rc = launch_suf_from_xy(e->stream, n_rows, p, (const double *)X_device,
                              (const double *)y_device, blk, blk + (size_t)p * p,
                              blk + (size_t)p * p + p, blk + (size_t)p * p + p + 2, planes.ptr);
  if (rc) return fail(BA_E_HIP, "suf kernel launch failed");
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BA_OK;
}

int ba_set_suf_from_block_device(ba_engine *e, int64_t n_total, int32_t p,
                                 const void *block_device) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!block_device) return fail(BA_E_INVALID, "null argument");
  if (n_total <= 0) return fail(BA_E_INVALID, "n must be positive");
  int rc = set_dimension(e, p);
  if (rc) return rc;
  const size_t pp = (size_t)p * p;
  std::vector<double> h(ba_suf_block_size(p));
  HIP_TRY(hipMemcpyAsync(h.data(), block_device, h.size() * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->xtx.assign(h.begin(), h.begin() + pp);
  e->xty.assign(h.begin() + pp, h.begin() + pp + p);
  e->yty = h[pp + p];
  e->sumy = h[pp + p + 1];
  e->xsum.assign(h.begin() + pp + p + 2, h.end());
  e->n = (double)n_total;
  e->have_suf = true;
  e->device_dirty = true;
  e->data_kind = DATA_REGRESSION;   // (the binomial, Poisson, Student-t and state-space setters say otherwise after this)
  return BA_OK;
}

int ba_build_suf_from_xy(ba_engine *e, int64_t n, int32_t p, const double *X,
                         const double *y) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!X || !y) return fail(BA_E_INVALID, "null argument");
  if (n <= 0 || p <= 0) return fail(BA_E_INVALID, "n and p must be positive");
  HIP_TRY(e->dX.resize((size_t)n * p));
  HIP_TRY(e->dy.resize((size_t)n));
  HIP_TRY(hipMemcpyAsync(e->dX.ptr, X, (size_t)n * p * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->dy.ptr, y, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
  int rc = ba_build_suf_from_xy_device(e, n, p, e->dX.ptr, e->dy.ptr);
  e->dX.release();
  e->dy.release();
  return rc;
}

int ba_get_regression_suf(ba_engine *e, double *xtx, double *xty, double *yty,
                          double *n, double *ybar, double *xbar) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!e->have_suf) return fail(BA_E_STATE, "no regression data set");
  const int p = e->p;
  if (xtx) std::memcpy(xtx, e->xtx.data(), (size_t)p * p * 8);
  if (xty) std::memcpy(xty, e->xty.data(), (size_t)p * 8);
  if (yty) *yty = e->yty;
  if (n) *n = e->n;
  if (ybar) *ybar = e->sumy / e->n;
  if (xbar)
    for (int j = 0; j < p; ++j) xbar[j] = e->xsum[j] / e->n;
  return BA_OK;
}

// -------------------------------------------------------------- priors
int ba_set_slab(ba_engine *e, const double *prior_mean,
                const double *unscaled_prior_precision) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (!prior_mean || !unscaled_prior_precision) return fail(BA_E_INVALID, "null argument");
  if (e->p <= 0) return fail(BA_E_STATE, "set the regression data before the priors");
  const int p = e->p;
  e->b.assign(prior_mean, prior_mean + p);
  e->ominv.assign(unscaled_prior_precision, unscaled_prior_precision + (size_t)p * p);
  e->have_slab = true;
  e->device_dirty = true;
  return BA_OK;
}

int ba_set_spike(ba_engine *e, const double *pi, int64_t max_model_size) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (!pi) return fail(BA_E_INVALID, "null argument");
  if (e->p <= 0) return fail(BA_E_STATE, "set the regression data before the priors");
  for (int j = 0; j < e->p; ++j)
    if (!(pi[j] >= 0.0 && pi[j] <= 1.0))
      return fail(BA_E_INVALID, "prior inclusion probabilities must be in [0, 1]");
  e->pi.assign(pi, pi + e->p);
  e->max_model_size = max_model_size;
  e->have_spike = true;
  e->device_dirty = true;
  return BA_OK;
}

int ba_set_sigma_prior(ba_engine *e, double prior_df, double sigma_guess,
                       double sigma_upper_limit) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (sigma_upper_limit < 0) return fail(BA_E_INVALID, "sigma_max must be non-negative.");
  // ChisqModel(df, sigma): alpha = df/2, beta = df sigma^2/2 (ChisqModel.cpp:56-57)
  const double alpha = prior_df / 2.0;
  const double beta = prior_df * sigma_guess * sigma_guess / 2.0;
  e->prior_df = 2 * alpha;
  e->prior_ss = 2 * beta;
  e->sigma_guess = sigma_guess;
  e->sigma_max = sigma_upper_limit;
  e->have_sigma = true;
  return BA_OK;
}

int ba_set_priors_ctor1(ba_engine *e, double prior_nobs, double expected_rsq,
                        double expected_model_size,
                        int32_t first_term_is_intercept) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (!e->have_suf) return fail(BA_E_STATE, "no regression data set");
  if (!(expected_rsq > 0 && expected_rsq < 1)) return fail(BA_E_INVALID, "expected_rsq must be in (0, 1)");
  // BregVsSampler.cpp:37-44, 48-85
  const int p = e->p;
  const double n = e->n, ybar = e->sumy / n;
  const double sst = e->yty - n * ybar * ybar;
  const double sigma_guess = std::sqrt(sst / (n - 1) * (1 - expected_rsq));
  std::vector<double> b(p, 0.0), om((size_t)p * p), pi(p);
  if (first_term_is_intercept) b[0] = ybar;
  for (size_t i = 0; i < (size_t)p * p; ++i) om[i] = e->xtx[i] * (prior_nobs / n);
  double prob = expected_model_size / p;
  if (prob > 1) prob = 1.0;
  std::fill(pi.begin(), pi.end(), prob);
  if (first_term_is_intercept) pi[0] = 1.0;
  int rc = ba_set_slab(e, b.data(), om.data());
  if (!rc) rc = ba_set_spike(e, pi.data(), -1);
  if (!rc) rc = ba_set_sigma_prior(e, prior_nobs, sigma_guess, e->sigma_max);
  return rc;
}

int ba_set_priors_ctor2(ba_engine *e, double prior_sigma_nobs,
                        double prior_sigma_guess, double prior_beta_nobs,
                        double diagonal_shrinkage,
                        double prior_inclusion_probability,
                        int32_t force_intercept) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (!e->have_suf) return fail(BA_E_STATE, "no regression data set");
  // BregVsSampler.cpp:87-142
  if (prior_sigma_guess <= 0)
    return fail(BA_E_INVALID, "illegal value of prior_sigma_guess in constructor to BregVsSampler");
  const double alpha = diagonal_shrinkage;
  if (alpha > 1.0 || alpha < 0.0)
    return fail(BA_E_INVALID, "illegal value of 'diagonal_shrinkage' in BregVsSampler constructor.");
  const int p = e->p;
  const double n = e->n;
  std::vector<double> b(p, 0.0), om((size_t)p * p), pi(p, prior_inclusion_probability);
  b[0] = e->sumy / n;
  for (size_t i = 0; i < (size_t)p * p; ++i) om[i] = e->xtx[i] * (prior_beta_nobs / n);
  if (alpha < 1.0) {
    for (int j = 0; j < p; ++j) {
      const double d = om[(size_t)j * p + j];
      om[(size_t)j * p + j] = d + d * (alpha / (1 - alpha));
    }
    for (auto &v : om) v *= (1 - alpha);
  } else {
    for (int j = 0; j < p; ++j)
      for (int i = 0; i < p; ++i)
        if (i != j) om[(size_t)j * p + i] = 0.0;
  }
  if (force_intercept) pi[0] = 1.0;
  int rc = ba_set_slab(e, b.data(), om.data());
  if (!rc) rc = ba_set_spike(e, pi.data(), -1);
  if (!rc) rc = ba_set_sigma_prior(e, prior_sigma_nobs, prior_sigma_guess, e->sigma_max);
  return rc;
}

int ba_get_priors(ba_engine *e, double *prior_mean, double *ominv, double *pi,
                  double *prior_df, double *prior_ss) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!e->have_slab || !e->have_spike || !e->have_sigma)
    return fail(BA_E_STATE, "priors not set");
  const int p = e->p;
  if (prior_mean) std::memcpy(prior_mean, e->b.data(), (size_t)p * 8);
  if (ominv) std::memcpy(ominv, e->ominv.data(), (size_t)p * p * 8);
  if (pi) std::memcpy(pi, e->pi.data(), (size_t)p * 8);
  if (prior_df) *prior_df = e->prior_df;
  if (prior_ss) *prior_ss = e->prior_ss;
  return BA_OK;
}

int ba_set_options(ba_engine *e, int32_t max_flips, double swap_threshold,
                   int32_t draw_beta, int32_t draw_sigma) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  e->max_flips = max_flips;
  if (swap_threshold != e->swap_threshold) e->device_dirty = true;
  e->swap_threshold = swap_threshold;
  e->draw_beta = draw_beta;
  e->draw_sigma = draw_sigma;
  return BA_OK;
}

int ba_set_tuning(ba_engine *e, int32_t waves_per_chain, int32_t walk_policy,
                  int32_t kcap_start) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!(waves_per_chain == 0 || waves_per_chain == 1 || waves_per_chain == 2 || waves_per_chain == 4))
    return fail(BA_E_INVALID, "waves_per_chain must be 0, 1, 2 or 4");
  if (walk_policy < -1 || walk_policy > 4) return fail(BA_E_INVALID, "walk_policy must be in [-1, 4]");
  if (kcap_start < 0) return fail(BA_E_INVALID, "kcap_start must be non-negative");
  MUTATE(e);
  if (e->state_ready) {
    int rc = set_device(e);
    if (!rc) rc = ba_sync(e);
    if (rc) return rc;
  }
  e->tune_waves = waves_per_chain;
  e->tune_walk_policy = walk_policy;
  e->tune_kcap_start = kcap_start;
  e->device_dirty = true;  // capacity and waves are chosen again
  return BA_OK;
}

// How the sweep kernels rebuild the factors after a single flip (ssvs_params.h).  Either way
// computes the same numbers, so nothing kept on the device -- tables, model blocks, a
// look-ahead batch -- is dropped: the next launch simply reads the new value.
int ba_set_rebuild_policy(ba_engine *e, int32_t policy) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (policy != 0 && policy != 1) return fail(BA_E_INVALID, "rebuild_policy must be 0 or 1");
  e->tune_rebuild_policy = policy;
  return BA_OK;
}

// for the tests of the spill streams (device_rng.h): a slot of a substream hands out `uniforms`
// numbers, not its whole stride (0: the default again).  Changes the draws.
int ba_set_slot_limit(ba_engine *e, int32_t uniforms) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (uniforms < 0 || (uniforms & 1)) return fail(BA_E_INVALID, "uniforms must be even and non-negative");
  MUTATE(e);
  e->slot_limit = uniforms;
  return BA_OK;
}

// --------------------------------------------------------------- state
int ba_set_state(ba_engine *e, int64_t chain, const uint8_t *gamma,
                 const double *beta, double sigsq) {
  ENGINE_PROLOGUE(e);
  if (e->p <= 0) return fail(BA_E_STATE, "set the regression data first");
  if (!gamma) return fail(BA_E_INVALID, "null argument");
  const int64_t C = e->cfg.chains;
  if (chain < -1 || chain >= C) return fail(BA_E_INVALID, "chain index out of range");
  if (latent_data(e->data_kind) && !student_kind(e->data_kind) && sigsq != 1.0)
    return fail(BA_E_INVALID, "the binomial samplers' latent data have unit variance: sigsq must be 1");
  if (chain < 0) la_discard(e);  // every chain is overwritten: nothing to rewind to
  MUTATE(e);
  // launches in flight (and sweeps still owed after a capacity stop) belong to
  // the OLD state: resolve them before it is overwritten.  Setting every chain
  // also clears chain errors (the caller starts over).
  if (e->state_ready) {
    int rc = ba_sync(e);
    if (rc && chain >= 0) return rc;
    if (rc) {
      HIP_TRY(hipMemsetAsync(e->dstatus.ptr, 0, (size_t)C * 4, e->stream));
      HIP_TRY(hipMemsetAsync(e->dtodo.ptr, 0, (size_t)C * 4, e->stream));
    }
  }
  int rc = alloc_chain_state(e);
  if (rc) return rc;
  const size_t p = (size_t)e->p;
  std::vector<double> zeros;
  if (!beta) {
    zeros.assign(p, 0.0);
    beta = zeros.data();
  }
  hipStream_t s = e->stream;
  if (chain < 0) {
    std::vector<uint8_t> G((size_t)C * p);
    std::vector<double> B((size_t)C * p), S((size_t)C, sigsq);
    for (int64_t c = 0; c < C; ++c) {
      std::memcpy(&G[(size_t)c * p], gamma, p);
      std::memcpy(&B[(size_t)c * p], beta, p * 8);
    }
    HIP_TRY(hipMemcpyAsync(e->dgamma.ptr, G.data(), G.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dbeta.ptr, B.data(), B.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dsigsq.ptr, S.data(), S.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
  } else {
    HIP_TRY(hipMemcpyAsync(e->dgamma.ptr + (size_t)chain * p, gamma, p, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dbeta.ptr + (size_t)chain * p, beta, p * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dsigsq.ptr + chain, &sigsq, 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return BA_OK;
}

int ba_get_state(ba_engine *e, int64_t chain, uint8_t *gamma, double *beta,
                 double *sigsq) {
  ENGINE_ACCESSOR_NOJOIN(e);
  if (!e->state_ready) return fail(BA_E_STATE, "no chain state yet");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  if (e->la.served > 0 && e->la.served <= e->la.avail)  // the draw ba_draw_next is serving
    return la_read(e, chain, gamma, beta, sigsq);
  {
    int rcj = pipe_join(e);
    if (rcj) return rcj;
  }
  if (ss_la_serving(e)) {   // the draw ba_ss_draw_next is serving
    const ba_engine::SsLa::Rows *r = nullptr;
    int rcr = ss_la_rows(e, chain, false, &r);
    if (rcr) return rcr;
    const size_t p = (size_t)e->p, row = (size_t)e->ssla.served - 1;
    if (gamma) std::memcpy(gamma, &r->gamma[row * p], p);
    if (beta) std::memcpy(beta, &r->beta[row * p], p * 8);
    if (sigsq) *sigsq = r->sig[row];
    return BA_OK;
  }
  int rc = ba_sync(e);
  if (rc) return rc;
  // (one batch through the pinned staging buffer: beta | sigsq | gamma)
  const size_t p = (size_t)e->p;
  HIP_TRY(pinned_reserve(e, p * 9 + 16));
  double *hb = (double *)e->pinned, *hs = hb + p;
  uint8_t *hg = (uint8_t *)(hs + 1);
  if (gamma) HIP_TRY(hipMemcpyAsync(hg, e->dgamma.ptr + (size_t)chain * p, p, hipMemcpyDeviceToHost, e->stream));
  if (beta) HIP_TRY(hipMemcpyAsync(hb, e->dbeta.ptr + (size_t)chain * p, p * 8, hipMemcpyDeviceToHost, e->stream));
  if (sigsq) HIP_TRY(hipMemcpyAsync(hs, e->dsigsq.ptr + chain, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (gamma) std::memcpy(gamma, hg, p);
  if (beta) std::memcpy(beta, hb, p * 8);
  if (sigsq) *sigsq = *hs;
  return BA_OK;
}

// PosteriorSampler::logpri() of BregVsSampler (BregVsSampler.cpp:380-393) for one
// chain's current state: log p(gamma) + log p(sigma^2) + log N(beta_g | b_g,
// sigma^2 Omega_g).  Host arithmetic on the chain's state and the host copies of
// the priors (a k x k Cholesky): it is interface, not hot path.
int ba_logpri(ba_engine *e, int64_t chain, double *out) {
  ENGINE_ACCESSOR_SERVED(e);   // (ba_get_state below sees the draw being served)
  if (!out) return fail(BA_E_INVALID, "null argument");
  if (!e->have_slab || e->pi.empty()) return fail(BA_E_STATE, "priors are not set");
  const size_t p = (size_t)e->p;
  std::vector<uint8_t> g(p);
  std::vector<double> beta(p);
  double sigsq = 0.0;
  int rc = ba_get_state(e, chain, g.data(), beta.data(), &sigsq);
  if (rc) return rc;
  const double ninf = -std::numeric_limits<double>::infinity();
  std::vector<int> idx;
  for (size_t j = 0; j < p; ++j)
    if (g[j]) idx.push_back((int)j);
  const int k = (int)idx.size();
  // VariableSelectionPrior::logp (VariableSelectionPrior.cpp:271-285)
  double ans = 0.0;
  if (e->max_model_size >= 0 && k > e->max_model_size) ans = ninf;
  for (size_t j = 0; j < p && ans > ninf; ++j) {
    ans += g[j] ? std::log(e->pi[j]) : std::log(1.0 - e->pi[j]);
    if (!std::isfinite(ans)) ans = ninf;
  }
  if (!(ans > ninf)) {
    *out = ninf;
    return BA_OK;
  }
  // GenericGaussianVarianceSampler::log_prior: Gamma(df/2, ss/2) density of
  // 1/sigma^2 and the Jacobian of the reciprocal
  const double a = 0.5 * e->prior_df, b = 0.5 * e->prior_ss, x = 1.0 / sigsq;
  ans += a * std::log(b) - std::lgamma(a) + (a - 1.0) * std::log(x) - b * x - 2.0 * std::log(sigsq);
  if (k > 0) {
    // dmvn(beta_g, b_g, Omega^{-1}_g / sigma^2, log)
    std::vector<double> L((size_t)k * k, 0.0), d(k);
    for (int c = 0; c < k; ++c)
      for (int r = c; r < k; ++r) L[(size_t)r * k + c] = e->ominv[(size_t)idx[c] * p + idx[r]] / sigsq;
    for (int i = 0; i < k; ++i) d[i] = beta[idx[i]] - e->b[idx[i]];
    double quad = 0.0;  // Mdist on the matrix itself, before it is overwritten
    for (int c = 0; c < k; ++c) {
      quad += d[c] * d[c] * L[(size_t)c * k + c];
      for (int r = c + 1; r < k; ++r) quad += 2.0 * d[c] * d[r] * L[(size_t)r * k + c];
    }
    double ld = 0.0;
    for (int c = 0; c < k; ++c) {  // left-looking Cholesky, lower triangle in place
      double s = L[(size_t)c * k + c];
      for (int t = 0; t < c; ++t) s -= L[(size_t)c * k + t] * L[(size_t)c * k + t];
      if (!(s > 0.0)) { ld = ninf; break; }
      const double sd = std::sqrt(s);
      L[(size_t)c * k + c] = sd;
      ld += 2.0 * std::log(sd);
      for (int r = c + 1; r < k; ++r) {
        double v = L[(size_t)r * k + c];
        for (int t = 0; t < c; ++t) v -= L[(size_t)r * k + t] * L[(size_t)c * k + t];
        L[(size_t)r * k + c] = v / sd;
      }
    }
    ans += -0.5 * k * std::log(2.0 * M_PI) + 0.5 * ld - 0.5 * quad;
  }
  *out = ans;
  return BA_OK;
}

int ba_get_states(ba_engine *e, uint8_t *gamma, double *beta, double *sigsq) {
  ENGINE_ACCESSOR_SERVED(e);
  if (!e->state_ready) return fail(BA_E_STATE, "no chain state yet");
  if (ss_la_serving(e)) {
    // the draw being served, every chain: row `served - 1` of every chain's block of the record
    int rcw = ss_la_wait(e);
    if (rcw) return rcw;
    const ba_engine::SsLa &A = e->ssla;
    const size_t p = (size_t)e->p, C = (size_t)e->cfg.chains, L = (size_t)A.len;
    const size_t at = (size_t)A.slot * C * L + (size_t)A.served - 1;
    if (gamma) HIP_TRY(hipMemcpy2D(gamma, p, A.rgamma.ptr + at * p, L * p, p, C, hipMemcpyDeviceToHost));
    if (beta) HIP_TRY(hipMemcpy2D(beta, p * 8, A.rbeta.ptr + at * p, L * p * 8, p * 8, C, hipMemcpyDeviceToHost));
    if (sigsq) HIP_TRY(hipMemcpy2D(sigsq, 8, A.rsig.ptr + at, L * 8, 8, C, hipMemcpyDeviceToHost));
    return BA_OK;
  }
  if (e->la.served > 0 && e->la.served <= e->la.avail && (e->la.served < e->la.avail || e->la.ahead)) {
    // the draw being served, every chain: from the record (the chains themselves are ahead)
    int rcw = la_wait(e);
    if (rcw) return rcw;
    return read_record_row_all(e, e->la.slot * e->la.len + e->la.served - 1, gamma, beta, sigsq);
  }
  int rc = ba_sync(e);
  if (rc) return rc;
  const size_t p = (size_t)e->p, C = (size_t)e->cfg.chains;
  if (gamma) HIP_TRY(hipMemcpy(gamma, e->dgamma.ptr, C * p, hipMemcpyDeviceToHost));
  if (beta) HIP_TRY(hipMemcpy(beta, e->dbeta.ptr, C * p * 8, hipMemcpyDeviceToHost));
  if (sigsq) HIP_TRY(hipMemcpy(sigsq, e->dsigsq.ptr, C * 8, hipMemcpyDeviceToHost));
  return BA_OK;
}

int ba_seed(ba_engine *e, uint64_t seed) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  // sweeps in flight -- and sweeps still owed after a capacity stop -- belong
  // to the old key
  if (e->state_ready) {
    int rc = ba_sync(e);
    if (rc) return rc;
  }
  e->seed = seed;
  const size_t C = (size_t)e->cfg.chains;
  hipStream_t s = e->stream;
  // every sampler of every chain restarts at position 0 of its new stream
  if (e->dpos.ptr) HIP_TRY(hipMemsetAsync(e->dpos.ptr, 0, C * 8, s));
  if (e->dpos_sss.ptr) HIP_TRY(hipMemsetAsync(e->dpos_sss.ptr, 0, C * 8, s));
  if (e->dpos_ada.ptr) HIP_TRY(hipMemsetAsync(e->dpos_ada.ptr, 0, C * 8, s));
  if (e->dpos_level.ptr) HIP_TRY(hipMemsetAsync(e->dpos_level.ptr, 0, C * 8, s));
  if (e->dpos_var.ptr) HIP_TRY(hipMemsetAsync(e->dpos_var.ptr, 0, C * SSG_MAX_VAR * 8, s));
  e->lat.draws = 0;
  if (e->dpos_state.ptr) HIP_TRY(hipMemsetAsync(e->dpos_state.ptr, 0, C * 8, s));
  if (e->dpos_forecast.ptr) HIP_TRY(hipMemsetAsync(e->dpos_forecast.ptr, 0, C * 8, s));
  if (e->dslt_pos.ptr) HIP_TRY(hipMemsetAsync(e->dslt_pos.ptr, 0, C * 8, s));
  if (e->dslt_count.ptr) HIP_TRY(hipMemsetAsync(e->dslt_count.ptr, 0, C * 8, s));
  HIP_TRY(hipStreamSynchronize(s));
  return BA_OK;
}

}  // extern "C"

namespace boom_amd {

// A change of sampler (BregVs <-> SpikeSlab) or of the XtX scale inside V has
// to wait for the launches in flight (they may still be escalated).
int switch_mode(ba_engine *e, int mode, double v_scale) {
  if (e->cur_mode == mode && e->v_scale_want == v_scale) return BA_OK;
  if (e->state_ready) {
    int rc = ba_sync(e);
    if (rc) return rc;
  }
  e->cur_mode = mode;
  e->table_ok = false;
  e->model_ok = false;
  if (e->v_scale_want != v_scale) {
    e->v_scale_want = v_scale;
    e->device_dirty = true;
  }
  return BA_OK;
}

// ---- which sweep serves which data ------------------------------------------------------
// indexed by DataKind: what a family's entry point says while the engine holds other data ...
static const char *const kSetDataFirst[] = {nullptr,
                                            "call ba_ss_set_data first",
                                            "call ba_probit_set_data first",
                                            "call ba_logit_set_data first",
                                            "call ba_poisson_set_data first",
                                            "call ba_student_set_data first",
                                            "call ba_quantile_set_data first",
                                            "call ba_mlogit_set_data first",
                                            "call ba_ss_student_set_data first",
                                            "call ba_ss_poisson_set_data first",
                                            "call ba_ss_logit_set_data first"};
// ... and where the data in hand send a caller of another family's entry point
static const char *const kUseSweep[] = {nullptr,
                                        "state-space data are set: use ba_ss_sweep",
                                        "binomial data are set: use ba_probit_sweep",
                                        "binomial data are set: use ba_logit_sweep",
                                        "Poisson data are set: use ba_poisson_sweep",
                                        "Student-t regression data are set: use ba_student_sweep",
                                        "quantile regression data are set: use ba_quantile_sweep",
                                        "multinomial logit data are set: use ba_mlogit_sweep",
                                        "Student-t state-space data are set: use ba_ss_student_sweep",
                                        "Poisson state-space data are set: use ba_ss_poisson_sweep",
                                        "logit state-space data are set: use ba_ss_logit_sweep"};

const char *set_data_first(DataKind wants) { return kSetDataFirst[wants]; }

// Every cell is BA_E_STATE; tests/test_data_kind_gpu.py holds the whole matrix.
int sweep_refusal(const ba_engine *e, DataKind wants, bool sss) {
  const DataKind have = e->data_kind;
  if (have == wants) return BA_OK;
  // (the quantile sampler's column and row: every other sweep names ba_quantile_sweep, and
  // ba_quantile_sweep asks for its own data whatever else is set)
  // (so with the multinomial logit sampler's)
  // (and the state space Student, Poisson and logit families')
  if (have == DATA_QUANTILE || have == DATA_MLOGIT || have == DATA_SS_STUDENT || have == DATA_SS_POISSON ||
      have == DATA_SS_LOGIT)
    return fail(BA_E_STATE, kUseSweep[have]);
  if (wants == DATA_STATE_SPACE || wants == DATA_QUANTILE || wants == DATA_MLOGIT || wants == DATA_SS_STUDENT ||
      wants == DATA_SS_POISSON || wants == DATA_SS_LOGIT)
    return fail(BA_E_STATE, kSetDataFirst[wants]);
  if (have == DATA_STUDENT) return fail(BA_E_STATE, kUseSweep[have]);
  if (wants == DATA_REGRESSION) {   // ba_sweep, ba_draw_next, ba_adaptive_sweep; ba_sss_sweep
    if (have == DATA_STATE_SPACE) return fail(BA_E_STATE, kUseSweep[have]);
    return fail(BA_E_STATE,
                sss ? "binomial data are set: use ba_logit_sweep / ba_probit_sweep (a sweep without the imputation is not a draw of those samplers)"
                    : "binomial data are set: use ba_logit_sweep / ba_probit_sweep (the regression sampler has no meaning on latent data)");
  }
  // ba_student_sweep names the sweep of whatever data are set, ba_logit_sweep that of Poisson
  // data (which run on the logit sampler's machinery); the others ask for their own data
  if (have != DATA_REGRESSION && (wants == DATA_STUDENT || (wants == DATA_LOGIT && have == DATA_POISSON)))
    return fail(BA_E_STATE, kUseSweep[have]);
  return fail(BA_E_STATE, kSetDataFirst[wants]);
}

// ---- one double per chain (chain == -1: every chain) --------------------------------------
int write_per_chain(ba_engine *e, double *dev, int64_t chain, double value) {
  const size_t C = (size_t)e->cfg.chains;
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (chain < 0) {
    std::vector<double> v(C, value);
    HIP_TRY(hipMemcpy(dev, v.data(), C * 8, hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy(dev + chain, &value, 8, hipMemcpyHostToDevice));
  }
  return BA_OK;
}
int read_per_chain(ba_engine *e, const double *dev, int64_t chain, double *out) {
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (chain < 0) HIP_TRY(hipMemcpy(out, dev, (size_t)e->cfg.chains * 8, hipMemcpyDeviceToHost));
  else HIP_TRY(hipMemcpy(out, dev + chain, 8, hipMemcpyDeviceToHost));
  return BA_OK;
}

// ------------------------------------------------------------ hot path
// la_half >= 0: a look-ahead batch that overlaps its neighbours -- recorded into that half of
// the draw record, the chains' state on entry saved into that snapshot set (the caller has
// checked la_can_overlap)
static int sweep_impl(ba_engine *e, int32_t nsweeps, bool record, int la_half) {
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = sweep_refusal(e, DATA_REGRESSION);
  if (rc) return rc;
  rc = switch_mode(e, 0, 1.0);
  if (rc) return rc;
  rc = upload_shared(e);
  if (rc) return rc;
  rc = alloc_chain_state(e);
  if (rc) return rc;
  if (record && e->trace_stride > 0 && nsweeps > e->trace_stride)
    return fail(BA_E_INVALID, "nsweeps exceeds the enabled trace length");
  HIP_TRY(e->dmodel.resize(2 * (size_t)e->cfg.chains * ssvs_scalar_layout(64).total));
  SsvsParams P;
  fill_params(e, P);
  if (!record) {  // (the record buffers belong to the look-ahead batches)
    P.trace_sigsq = P.trace_logp = P.trace_k = nullptr;
    P.rec_idx = nullptr;
    P.rec_beta = nullptr;
    P.trace_stride = 0;
    P.trace_idx = nullptr;   // ... and nothing of the record is valid any more (ba_predict checks)
    if (e->trace_stride > 0)
      HIP_TRY(hipMemsetAsync(e->dtrace_idx.ptr, 0, (size_t)e->cfg.chains * 4, e->stream));
  }
  const SsvsLds lay = ssvs_lds_layout(e->p, e->kcap);
  if (lay.total > e->lds_per_cu)
    return fail(BA_E_INVALID, "problem does not fit the LDS working set");
  if (record && e->trace_stride > 0 && la_half < 0)  // traces are those of the last ba_sweep call
    HIP_TRY(hipMemsetAsync(e->dtrace_idx.ptr, 0, (size_t)e->cfg.chains * 4, e->stream));
  if (la_half >= 0) {
    P.trace_row0 = la_half * e->la.len;
    (void)la_snap_fields(e, [&](auto &, auto &snap, size_t n, auto member) {   // (saved into set la_half)
      P.*member = snap.ptr + (size_t)la_half * (size_t)e->cfg.chains * n;
      return hipSuccess;
    });
  }
#ifndef BA_PIPELINE
#define BA_PIPELINE 1
#endif
  // Consecutive ba_sweep calls with nothing in between: the launches alternate between two
  // streams and hand the chains over one by one (ssvs_kernel.hip), so that the next launch
  // fills the slots the current one's early finishers leave instead of waiting for its
  // slowest chain.  Only while every chain's workgroup is resident at once, no trace is
  // recorded (its cursor is reset per call) and no chain lives in the large-model kernel.
  int group = 0;   // chains resident at once
  const bool all_fit = chains_fit(e, lay.total, &group);
  const bool pipelined = BA_PIPELINE && nsweeps > 0 && (e->trace_stride == 0 || la_half >= 0) && !e->big_active &&
                         all_fit && (!e->kt_enabled || e->kt_overlap);
  if (la_half >= 0 && !pipelined) return fail(BA_E_STATE, "look-ahead batch cannot overlap");
  if (!pipelined) {
    // More chains than the machine holds (round 4).  The chains go out in GROUPS of what fits
    // at once, the groups alternating between the engine's two streams: group g + 1's
    // workgroups move into the slots group g's early finishers leave -- different chains,
    // so no hand-over is needed -- and a group's next launch follows its last one on the
    // same stream.  (Rounds 1-3: one launch of more workgroups than fit -- a few workgroups
    // of the last round then start a whole round late on this machine, 53 ms per
    // 2048-chain launch where two launches of 1024 take 46 -- or, for exactly two or three
    // groups, separate launches one after the other, each as long as its slowest chain.)
    const int C = e->cfg.chains;
    const bool groups = BA_PIPELINE && nsweeps > 0 && e->cur_mode != 2 && !e->big_active && !all_fit &&
                        e->trace_stride == 0 && (!e->kt_enabled || e->kt_overlap);
    if (groups) {
      int rco = pipe_open(e);
      if (rco) return rco;
      if (!(e->pipe.on && e->pipe.groups)) {
        int rcj = pipe_join(e);
        if (rcj) return rcj;
        // (the other stream behind everything the main stream holds so far: uploads, mutators)
        HIP_TRY(hipEventRecord(e->pipe.ev[0], e->stream));
        HIP_TRY(hipStreamWaitEvent(e->pipe.stream, e->pipe.ev[0], 0));
      }
      SsvsParams Pg = P;
      int g = 0;
      for (int first = 0; first < C; first += group, ++g) {
        Pg.chain_first = first;
        Pg.chain_count = std::min(group, C - first);
        HIP_TRY(launch_ssvs_sweep((g & 1) ? e->pipe.stream : e->stream, Pg, (int)nsweeps));
      }
      e->pipe.on = true;
      e->pipe.groups = true;
    } else {
      int rcj = pipe_join(e);
      if (rcj) return rcj;
      HIP_TRY(launch_sweeps(e, P, (int)nsweeps));
    }
  } else {
    const size_t C = (size_t)e->cfg.chains, qlen = C + 2;
    int rco = pipe_open(e);
    if (rco) return rco;
    if (e->pipe.q.count != 4 * qlen) {
      HIP_TRY(hipStreamSynchronize(e->stream));
      HIP_TRY(e->pipe.q.resize(4 * qlen));
      HIP_TRY(e->pipe.err.resize(1));
      HIP_TRY(hipMemset(e->pipe.err.ptr, 0, 4));
    }
    const int k = e->pipe.on ? e->pipe.k : 0;     // (a new pipeline starts on the main stream)
    hipStream_t st = (k & 1) ? e->pipe.stream : e->stream;
    int32_t *qout = e->pipe.q.ptr + (size_t)(k & 3) * qlen;
    // the queue this launch fills: emptied on its own stream (after the launch two before
    // it, whose hand-over to the launch before it used the queue four back at the latest)
    HIP_TRY(hipMemsetAsync(qout, 0, 8, st));
    HIP_TRY(hipMemsetAsync(qout + 2, 0xFF, C * 4, st));
    HIP_TRY(hipEventRecord(e->pipe.ev[k & 3], st));
    P.q_out = qout;
    P.q_error = e->pipe.err.ptr;
    if (k > 0) {
      P.q_in = e->pipe.q.ptr + (size_t)((k - 1) & 3) * qlen;
      // (... which the previous launch's stream has emptied before that launch)
      HIP_TRY(hipStreamWaitEvent(st, e->pipe.ev[(k - 1) & 3], 0));
    }
    HIP_TRY(launch_ssvs_sweep(st, P, (int)nsweeps));
    if (la_half >= 0) HIP_TRY(hipEventRecord(e->la.done[la_half], st));
    e->pipe.on = true;
    e->pipe.unchecked = true;
    e->pipe.k = k + 1;
  }
  e->table_ok = true;  // until anything but another ba_sweep touches the engine
  e->model_ok = true;
  return BA_OK;
}
}  // namespace boom_amd

extern "C" {

int ba_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE_NOJOIN(e);
  if (e->la.served < e->la.avail || e->data_kind != DATA_REGRESSION || e->cur_mode != 0) {
    int rcj = pipe_join(e);   // (anything but a plain continuation)
    if (rcj) return rcj;
  }
  // unserved look-ahead draws: the sweeps asked for here come after the last one served
  int rc = la_rewind(e);
  if (rc) return rc;
  return sweep_impl(e, nsweeps, /*record=*/e->la.len <= 1);
}

int ba_set_lookahead(ba_engine *e, int32_t lookahead) {
  ENGINE_PROLOGUE(e);
  if (lookahead < 1) return fail(BA_E_INVALID, "lookahead must be at least 1");
  MUTATE(e);
  if (lookahead > 1) {
    // (room for two batches: the one being served and the one launched ahead of it)
    int rc = ba_enable_draws(e, 2 * lookahead);
    if (rc) return rc;
  }
  e->la.len = lookahead;
  e->la.pipe = true;
  return BA_OK;
}

// can the next look-ahead batch overlap its neighbours (sweep_impl's conditions)
static bool la_can_overlap(const ba_engine *e) {
  if (!BA_PIPELINE || !e->la.pipe || e->big_active || (e->kt_enabled && !e->kt_overlap) || e->kcap <= 0) return false;
  return chains_fit(e, ssvs_lds_layout(e->p, e->kcap).total);
}

int ba_draw_next(ba_engine *e) {
  ENGINE_PROLOGUE_NOJOIN(e);
  if (e->la.len <= 1) return ba_sweep(e, 1);
  if (e->la.served == e->la.avail) {
    // the record is used up: on to the next batch
    if (e->la.ahead) {
      // ... which is already running (or done): the other half of the record
      e->la.slot ^= 1;
      e->la.ahead = false;
      la_discard(e);
      e->la.cur_piped = true;
    } else {
      // ... from the chains' current state
      int rc = pipe_join(e);
      if (rc) return rc;
      la_discard(e);
      rc = switch_mode(e, 0, 1.0);
      if (!rc) rc = upload_shared(e);
      if (!rc) rc = alloc_chain_state(e);
      if (rc) return rc;
      if (!e->la.done[0]) {
        HIP_TRY(hipEventCreateWithFlags(&e->la.done[0], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->la.done[1], hipEventDisableTiming));
      }
      e->la.slot = 0;
      // (a batch that overlaps: its workgroups take the snapshot themselves)
      e->la.cur_piped = la_can_overlap(e);
      rc = e->la.cur_piped ? la_snap_alloc(e) : la_copy(e, true, 0);
      if (!rc) rc = sweep_impl(e, e->la.len, true, e->la.cur_piped ? 0 : -1);
      if (rc) return rc;
    }
    e->la.avail = e->la.len;
    // the batch after this one goes out now, into the other half
    if (e->la.cur_piped && la_can_overlap(e)) {
      int rc = sweep_impl(e, e->la.len, true, e->la.slot ^ 1);
      if (rc) return rc;
      e->la.ahead = true;
    }
  }
  ++e->la.served;
  return BA_OK;
}

int ba_sync(ba_engine *e) {
  ENGINE_ACCESSOR_SERVED(e);
  // (while ba_ss_draw_next serves a batch the chains run ahead on purpose: what the caller
  // waits for is the batch being served)
  if (ss_la_serving(e)) return ss_la_wait(e);
  HIP_TRY(hipStreamSynchronize(e->stream));   // (also the caller's own work on ba_stream())
  if (e->clean_seq == e->api_seq) return BA_OK;   // (no call since the last clean check: the status words are as they were)
  int rc = pipe_check(e);
  if (rc) return rc;
  const uint64_t seq = e->api_seq;   // (a catch-up inside the check is the check's own business)
  rc = check_chain_status(e);
  // (only at top level or from an accessor: a call in progress may enqueue more after this)
  if (rc == BA_OK && e->api_depth == 0) e->clean_seq = seq;
  return rc;
}

int ba_log_model_prob(ba_engine *e, int32_t ngamma, const uint8_t *gammas,
                      double *out) {
  ENGINE_PROLOGUE(e);
  if (!gammas || !out || ngamma <= 0) return fail(BA_E_INVALID, "bad argument");
  // the regression model's own sufficient statistics: in state-space mode they
  // are per chain and move every sweep, so there is no one answer
  if (e->data_kind == DATA_STATE_SPACE || e->data_kind == DATA_SS_STUDENT || e->data_kind == DATA_SS_POISSON ||
      e->data_kind == DATA_SS_LOGIT)
    return fail(BA_E_STATE, "ba_log_model_prob is not defined once state-space data are set (per-chain sufficient statistics)");
  // BregVsSampler's V = Omega^{-1} + XtX (a SpikeSlabSampler launch with a fixed
  // slab precision leaves XtX / sigma^2 in it)
  int rc = switch_mode(e, 0, 1.0);
  if (rc) return rc;
  rc = upload_shared(e);
  if (rc) return rc;
  rc = alloc_chain_state(e);
  if (rc) return rc;
  const size_t p = (size_t)e->p;
  DevBuf<uint8_t> dg;
  DevBuf<double> dout;
  DevBuf<int32_t> dst;
  HIP_TRY(dg.resize((size_t)ngamma * p));
  HIP_TRY(dout.resize(ngamma));
  HIP_TRY(dst.resize(ngamma));
  HIP_TRY(hipMemcpyAsync(dg.ptr, gammas, (size_t)ngamma * p, hipMemcpyHostToDevice, e->stream));
  SsvsParams P;
  fill_params(e, P);
  // this entry evaluates arbitrary models: use the largest working set
  P.kcap = 64;
  while (P.kcap > 8 && ssvs_lds_layout(e->p, P.kcap).total > e->lds_per_cu) P.kcap -= 8;
  HIP_TRY(launch_ssvs_logp(e->stream, P, (const uint8_t *)dg.ptr, (int)ngamma,
                           dout.ptr, dst.ptr));
  std::vector<int32_t> st(ngamma);
  HIP_TRY(hipMemcpyAsync(out, dout.ptr, (size_t)ngamma * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(st.data(), dst.ptr, (size_t)ngamma * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  // vectors of more models than the LDS kernel holds: the large-model build, a few at
  // a time (each has a model block of two k x k factors in HBM)
  std::vector<int32_t> big;
  for (int i = 0; i < ngamma; ++i)
    if (st[i] == CHAIN_MODEL_TOO_LARGE) big.push_back(i);
  if (!big.empty()) {
    int kmax = 0;
    for (int32_t i : big) {
      int k = 0;
      for (size_t j = 0; j < p; ++j) k += gammas[(size_t)i * p + j] ? 1 : 0;
      kmax = std::max(kmax, k);
    }
    const int kcap = ((kmax + 63) / 64) * 64;
    if (kcap > BIG_KCAP_MAX || ssvs_big_lds_layout(e->p, kcap).total > e->lds_per_cu)
      return fail(BA_E_MODEL_TOO_LARGE, status_message(CHAIN_MODEL_TOO_LARGE));
    const size_t block = ssvs_scalar_layout(kcap).total, xs = (size_t)kcap * 64;
    const size_t batch = std::max<size_t>(1, std::min<size_t>(big.size(), ((size_t)256 << 20) / ((block + xs) * 8)));
    DevBuf<double> dmodel_ws, dxs_ws;
    DevBuf<int32_t> dwhich;
    HIP_TRY(dmodel_ws.resize(batch * block));
    HIP_TRY(dxs_ws.resize(batch * xs));
    HIP_TRY(dwhich.resize(big.size()));
    HIP_TRY(hipMemcpyAsync(dwhich.ptr, big.data(), big.size() * 4, hipMemcpyHostToDevice, e->stream));
    for (size_t b0 = 0; b0 < big.size(); b0 += batch) {
      const size_t nb = std::min(batch, big.size() - b0);
      HIP_TRY(launch_ssvs_big_logp(e->stream, P, kcap, (const uint8_t *)dg.ptr, dwhich.ptr + b0, (int)nb,
                                   dmodel_ws.ptr, dxs_ws.ptr, dout.ptr, dst.ptr));
    }
    HIP_TRY(hipMemcpyAsync(out, dout.ptr, (size_t)ngamma * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(st.data(), dst.ptr, (size_t)ngamma * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  for (int i = 0; i < ngamma; ++i)
    if (st[i] != CHAIN_OK) return fail(status_code(st[i]), status_message(st[i]));
  return BA_OK;
}

// ----------------------------------------------------------- summaries
int ba_reset_summaries(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  if (!e->state_ready) return BA_OK;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p;
  hipStream_t s = e->stream;
  HIP_TRY(hipMemsetAsync(e->dinc.ptr, 0, C * p * 4, s));
  HIP_TRY(hipMemsetAsync(e->dbsum.ptr, 0, C * p * 8, s));
  HIP_TRY(hipMemsetAsync(e->dbsumsq.ptr, 0, C * p * 8, s));
  std::vector<double> acc(C * ACC_COUNT, 0.0);
  for (size_t c = 0; c < C; ++c)
    acc[c * ACC_COUNT + ACC_MIN_MARGIN] = std::numeric_limits<double>::infinity();
  HIP_TRY(hipMemcpyAsync(e->dacc.ptr, acc.data(), acc.size() * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  return BA_OK;
}

int ba_summaries_device(ba_engine *e, void *out_device) {
  ENGINE_PROLOGUE(e);
  if (!out_device) return fail(BA_E_INVALID, "null argument");
  if (!e->state_ready) return fail(BA_E_STATE, "no chain state yet");
  SsvsParams P;
  fill_params(e, P);
  HIP_TRY(launch_ssvs_reduce_summaries(e->stream, P, (double *)out_device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BA_OK;
}

int ba_get_summaries(ba_engine *e, double *inclusion_count, double *beta_sum,
                     double *beta_sumsq, double *scalars) {
  ENGINE_PROLOGUE(e);
  int rc = ba_summaries_device(e, e->dsummary.ptr);
  if (rc) return rc;
  const size_t p = (size_t)e->p;
  std::vector<double> h(3 * p + SUMMARY_SCALARS);
  HIP_TRY(hipMemcpy(h.data(), e->dsummary.ptr, h.size() * 8, hipMemcpyDeviceToHost));
  if (inclusion_count) std::memcpy(inclusion_count, &h[0], p * 8);
  if (beta_sum) std::memcpy(beta_sum, &h[p], p * 8);
  if (beta_sumsq) std::memcpy(beta_sumsq, &h[2 * p], p * 8);
  if (scalars) std::memcpy(scalars, &h[3 * p], SUMMARY_SCALARS * 8);
  return BA_OK;
}

int ba_enable_traces(ba_engine *e, int32_t max_sweeps) {
  ENGINE_PROLOGUE(e);
  if (max_sweeps < 0) return fail(BA_E_INVALID, "max_sweeps must be non-negative");
  {  // (the recording buffers are the look-ahead's as well)
    int rc = la_rewind(e);
    if (rc) return rc;
    e->la.len = 1;
  }
  const size_t C = (size_t)e->cfg.chains;
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(e->dtr_sig.resize(C * max_sweeps));
  HIP_TRY(e->dtr_logp.resize(C * max_sweeps));
  HIP_TRY(e->dtr_k.resize(C * max_sweeps));
  e->drec_idx.release();
  e->drec_beta.release();
  e->trace_stride = max_sweeps;
  return BA_OK;
}

int ba_enable_draws(ba_engine *e, int32_t max_sweeps) {
  int rc = ba_enable_traces(e, max_sweeps);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains;
  e->rec_cap = std::max(64, e->big_active ? e->big_kcap : 0);
  HIP_TRY(e->drec_idx.resize(C * max_sweeps * e->rec_cap));
  HIP_TRY(e->drec_beta.resize(C * max_sweeps * e->rec_cap));
  return BA_OK;
}

}  // extern "C"

namespace boom_amd {
// rows [row0, row0 + nrows) of one chain's record, expanded to dense gamma / beta
static int read_record(ba_engine *e, int64_t c, int row0, int nrows, uint8_t *gamma,
                       double *beta, double *sigsq) {
  const size_t p = (size_t)e->p, cap = (size_t)e->rec_cap;
  const size_t base = (size_t)c * e->trace_stride + row0;
  std::vector<double> ks(nrows), sig(nrows), b((size_t)nrows * cap);
  std::vector<uint16_t> idx((size_t)nrows * cap);
  HIP_TRY(hipMemcpy(ks.data(), e->dtr_k.ptr + base, (size_t)nrows * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sig.data(), e->dtr_sig.ptr + base, (size_t)nrows * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(idx.data(), e->drec_idx.ptr + base * cap, idx.size() * 2, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(b.data(), e->drec_beta.ptr + base * cap, b.size() * 8, hipMemcpyDeviceToHost));
  if (gamma) std::memset(gamma, 0, (size_t)nrows * p);
  if (beta) std::memset(beta, 0, (size_t)nrows * p * 8);
  for (int s = 0; s < nrows; ++s) {
    const int k = (int)ks[s];
    if (k < 0 || (size_t)k > cap) return fail(BA_E_STATE, "corrupt draw record");
    for (int m = 0; m < k; ++m) {
      const size_t j = idx[(size_t)s * cap + m];
      if (j >= p) return fail(BA_E_STATE, "corrupt draw record");
      if (gamma) gamma[(size_t)s * p + j] = 1;
      if (beta) beta[(size_t)s * p + j] = b[(size_t)s * cap + m];
    }
    if (sigsq) sigsq[s] = sig[s];
  }
  return BA_OK;
}

// one row of EVERY chain's record (the draw ba_draw_next is serving)
static int read_record_row_all(ba_engine *e, int row, uint8_t *gamma, double *beta, double *sigsq) {
  const size_t p = (size_t)e->p, cap = (size_t)e->rec_cap, C = (size_t)e->cfg.chains;
  const size_t stride = (size_t)e->trace_stride;
  std::vector<double> ks(C), sig(C), b(C * cap);
  std::vector<uint16_t> idx(C * cap);
  HIP_TRY(hipMemcpy2D(ks.data(), 8, e->dtr_k.ptr + row, stride * 8, 8, C, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy2D(sig.data(), 8, e->dtr_sig.ptr + row, stride * 8, 8, C, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy2D(idx.data(), cap * 2, e->drec_idx.ptr + (size_t)row * cap, stride * cap * 2,
                      cap * 2, C, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy2D(b.data(), cap * 8, e->drec_beta.ptr + (size_t)row * cap, stride * cap * 8,
                      cap * 8, C, hipMemcpyDeviceToHost));
  if (gamma) std::memset(gamma, 0, C * p);
  if (beta) std::memset(beta, 0, C * p * 8);
  for (size_t c = 0; c < C; ++c) {
    const int k = (int)ks[c];
    if (k < 0 || (size_t)k > cap) return fail(BA_E_STATE, "corrupt draw record");
    for (int m = 0; m < k; ++m) {
      const size_t j = idx[c * cap + m];
      if (j >= p) return fail(BA_E_STATE, "corrupt draw record");
      if (gamma) gamma[c * p + j] = 1;
      if (beta) beta[c * p + j] = b[c * cap + m];
    }
    if (sigsq) sigsq[c] = sig[c];
  }
  return BA_OK;
}
}  // namespace boom_amd

extern "C" {

int ba_get_draws(ba_engine *e, int64_t chain, int32_t nsweeps, uint8_t *gamma,
                 double *beta, double *sigsq) {
  ENGINE_PROLOGUE(e);
  if (e->trace_stride <= 0 || e->drec_idx.count == 0)
    return fail(BA_E_STATE, "draw recording is not enabled");
  if (nsweeps <= 0 || nsweeps > e->trace_stride) return fail(BA_E_INVALID, "nsweeps out of range");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = ba_sync(e);
  if (rc) return rc;
  return read_record(e, chain, 0, nsweeps, gamma, beta, sigsq);
}

int ba_predict(ba_engine *e, int32_t first_draw, int32_t ndraws, int32_t nnew, const double *newX,
               double *out) {
  ENGINE_PROLOGUE(e);
  if (e->trace_stride <= 0 || e->drec_idx.count == 0)
    return fail(BA_E_STATE, "draw recording is not enabled");
  if (!newX || !out || nnew <= 0) return fail(BA_E_INVALID, "bad argument");
  if (first_draw < 0 || ndraws <= 0 || first_draw + ndraws > e->trace_stride)
    return fail(BA_E_INVALID, "draw range out of the record");
  if (ndraws > 65535 || e->cfg.chains > 65535) return fail(BA_E_INVALID, "too many draws or chains for one call");
  int rc = ba_sync(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains;
  {
    // only rows that the last recorded call actually wrote hold a draw
    std::vector<int32_t> rows(C);
    HIP_TRY(hipMemcpy(rows.data(), e->dtrace_idx.ptr, C * 4, hipMemcpyDeviceToHost));
    const int32_t have = *std::min_element(rows.begin(), rows.end());
    if (first_draw + ndraws > have)
      return fail(BA_E_INVALID, "draw range extends beyond the draws recorded by the last sweep call");
  }
  DevBuf<double> dX, dout;
  HIP_TRY(dX.resize((size_t)nnew * e->p));
  HIP_TRY(dout.resize(C * (size_t)ndraws * nnew));
  HIP_TRY(hipMemcpyAsync(dX.ptr, newX, (size_t)nnew * e->p * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(launch_predict(e->stream, e->dtr_k.ptr, e->drec_idx.ptr, e->drec_beta.ptr, e->trace_stride,
                         e->rec_cap, first_draw, ndraws, (int)C, e->p, dX.ptr, nnew, dout.ptr));
  HIP_TRY(hipMemcpyAsync(out, dout.ptr, C * (size_t)ndraws * nnew * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BA_OK;
}

int ba_get_coefficient_traces(ba_engine *e, int32_t nsweeps, int32_t nvars,
                              const int32_t *vars, double *out) {
  ENGINE_PROLOGUE(e);
  if (e->trace_stride <= 0 || e->drec_idx.count == 0)
    return fail(BA_E_STATE, "draw recording is not enabled");
  if (nsweeps <= 0 || nsweeps > e->trace_stride) return fail(BA_E_INVALID, "nsweeps out of range");
  if (nvars <= 0 || !vars || !out) return fail(BA_E_INVALID, "bad argument");
  for (int v = 0; v < nvars; ++v)
    if (vars[v] < 0 || vars[v] >= e->p) return fail(BA_E_INVALID, "variable index out of range");
  int rc = ba_sync(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, cap = (size_t)e->rec_cap, stride = (size_t)e->trace_stride;
  std::vector<int> slot(e->p, -1);
  for (int v = 0; v < nvars; ++v) slot[vars[v]] = v;
  std::vector<double> ks(nsweeps), b((size_t)nsweeps * cap);
  std::vector<uint16_t> idx((size_t)nsweeps * cap);
  std::memset(out, 0, C * (size_t)nvars * nsweeps * 8);
  for (size_t c = 0; c < C; ++c) {
    const size_t base = c * stride;
    HIP_TRY(hipMemcpy(ks.data(), e->dtr_k.ptr + base, (size_t)nsweeps * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(idx.data(), e->drec_idx.ptr + base * cap, idx.size() * 2, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b.data(), e->drec_beta.ptr + base * cap, b.size() * 8, hipMemcpyDeviceToHost));
    for (int s = 0; s < nsweeps; ++s) {
      const int k = (int)ks[s];
      for (int m = 0; m < k && (size_t)m < cap; ++m) {
        const int v = slot[idx[(size_t)s * cap + m] % (size_t)e->p];
        if (v >= 0) out[(c * nvars + v) * nsweeps + s] = b[(size_t)s * cap + m];
      }
    }
    // a variable named more than once: slot[] holds its last place, the others get that path too
    for (int v = 0; v < nvars; ++v) {
      const int last = slot[vars[v]];
      if (last != v)
        std::memcpy(out + (c * nvars + v) * nsweeps, out + (c * nvars + last) * nsweeps, (size_t)nsweeps * 8);
    }
  }
  return BA_OK;
}

int ba_get_traces(ba_engine *e, int32_t nsweeps, double *sigsq, double *logp,
                  double *model_size) {
  ENGINE_PROLOGUE(e);
  if (e->trace_stride <= 0) return fail(BA_E_STATE, "traces are not enabled");
  if (nsweeps <= 0 || nsweeps > e->trace_stride) return fail(BA_E_INVALID, "nsweeps out of range");
  int rc = ba_sync(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains;
  auto fetch = [&](double *dst, const double *src) -> hipError_t {
    if (!dst) return hipSuccess;
    return hipMemcpy2D(dst, (size_t)nsweeps * 8, src, (size_t)e->trace_stride * 8,
                       (size_t)nsweeps * 8, C, hipMemcpyDeviceToHost);
  };
  HIP_TRY(fetch(sigsq, e->dtr_sig.ptr));
  HIP_TRY(fetch(logp, e->dtr_logp.ptr));
  HIP_TRY(fetch(model_size, e->dtr_k.ptr));
  return BA_OK;
}

// ------------------------------------------- SpikeSlabSampler (sigma^2 given)
int ba_set_sigsq(ba_engine *e, int64_t chain, double sigsq) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!(sigsq > 0)) return fail(BA_E_INVALID, "sigsq must be positive");
  if (latent_data(e->data_kind) && !student_kind(e->data_kind) && sigsq != 1.0)
    return fail(BA_E_INVALID, "the binomial samplers' latent data have unit variance: sigsq must be 1");
  int rc = alloc_chain_state(e);
  if (rc) return rc;
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  return write_per_chain(e, e->dsigsq.ptr, chain, sigsq);
}

int ba_sss_set_slab(ba_engine *e, const double *mu, const double *precision,
                    int32_t precision_scales_with_sigsq, int32_t max_flips) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  int rc = ba_set_slab(e, mu, precision);
  if (rc) return rc;
  e->sss_slab_scales = precision_scales_with_sigsq ? 1 : 0;
  e->sss_max_flips = max_flips;
  if (!e->have_sigma) {  // the sigma prior plays no role given sigma^2
    e->prior_df = 1.0;
    e->prior_ss = 1.0;
    e->have_sigma = true;
  }
  return BA_OK;
}

int ba_sss_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = sweep_refusal(e, DATA_REGRESSION, /*sss=*/true);
  if (rc) return rc;
  if (!e->have_slab) return fail(BA_E_STATE, "call ba_sss_set_slab first");
  rc = alloc_chain_state(e);
  if (rc) return rc;
  double v_scale = 1.0;
  if (!e->sss_slab_scales) {
    // a slab precision that does not scale with sigma^2 makes V = P + XtX /
    // sigma^2 chain specific; the shared-matrix engine takes one sigma^2 for
    // all chains in this case (it is 1 for the logit / probit / Poisson users)
    const size_t C = (size_t)e->cfg.chains;
    rc = ba_sync(e);
    if (rc) return rc;
    std::vector<double> s2(C);
    HIP_TRY(hipMemcpy(s2.data(), e->dsigsq.ptr, C * 8, hipMemcpyDeviceToHost));
    for (size_t c = 1; c < C; ++c)
      if (s2[c] != s2[0])
        return fail(BA_E_INVALID, "a slab precision independent of sigma^2 needs the same sigma^2 in every chain");
    v_scale = 1.0 / s2[0];
  }
  rc = switch_mode(e, 1, v_scale);
  if (rc) return rc;
  rc = upload_shared(e);
  if (rc) return rc;
  HIP_TRY(e->dmodel.resize(2 * (size_t)e->cfg.chains * ssvs_scalar_layout(64).total));
  SsvsParams P;
  fill_params(e, P);
  if (e->trace_stride > 0)
    HIP_TRY(hipMemsetAsync(e->dtrace_idx.ptr, 0, (size_t)e->cfg.chains * 4, e->stream));
  HIP_TRY(launch_sweeps(e, P, (int)nsweeps));
  return BA_OK;
}

// ------------------------ AdaptiveSpikeSlabRegressionSampler (birth / death)
static int ada_prepare(ba_engine *e) {
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p;
  if (e->dada_birth.count == C * p) return BA_OK;
  HIP_TRY(e->dada_birth.resize(C * p));
  HIP_TRY(e->dada_death.resize(C * p));
  HIP_TRY(e->dada_iter.resize(C));
  HIP_TRY(e->dada_ws.resize(C * 4 * p));   // (the large-model kernel's: cumulative rates, the sweep's undo copy)
  HIP_TRY(e->dpos_ada.resize(C));
  std::vector<double> ones(C * p, 1.0);   // birth_rates_, death_rates_ start at 1
  HIP_TRY(hipMemcpyAsync(e->dada_birth.ptr, ones.data(), C * p * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->dada_death.ptr, ones.data(), C * p * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemsetAsync(e->dada_iter.ptr, 0, C * 8, e->stream));
  HIP_TRY(hipMemsetAsync(e->dpos_ada.ptr, 0, C * 8, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BA_OK;
}

int ba_adaptive_set_options(ba_engine *e, int32_t max_flips, double step_size,
                            double target_acceptance_rate) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (step_size == 0 || step_size < -1) return fail(BA_E_INVALID, "Step size must be positive.");
  if (target_acceptance_rate == 0 || target_acceptance_rate >= 1 || target_acceptance_rate < -1)
    return fail(BA_E_INVALID, "Target acceptance rate must be strictly between 0 and 1.");
  MUTATE(e);
  if (max_flips >= 0) e->ada_max_flips = max_flips;
  if (step_size > 0) e->ada_step = step_size;
  if (target_acceptance_rate > 0) e->ada_target = target_acceptance_rate;
  return BA_OK;
}

int ba_adaptive_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = sweep_refusal(e, DATA_REGRESSION);
  if (rc) return rc;
  rc = alloc_chain_state(e);
  if (rc) return rc;
  rc = switch_mode(e, 2, 1.0);
  if (rc) return rc;
  rc = upload_shared(e);
  if (rc) return rc;
  rc = ada_prepare(e);
  if (rc) return rc;
  if (e->trace_stride > 0 && nsweeps > e->trace_stride)
    return fail(BA_E_INVALID, "nsweeps exceeds the enabled trace length");
  HIP_TRY(e->dmodel.resize(2 * (size_t)e->cfg.chains * ssvs_scalar_layout(64).total));
  SsvsParams P;
  fill_params(e, P);
  if (ssvs_ada_lds_layout(e->p, e->kcap).total > e->lds_per_cu)
    return fail(BA_E_INVALID, "problem does not fit the LDS working set of the adaptive kernel");
  if (e->trace_stride > 0)
    HIP_TRY(hipMemsetAsync(e->dtrace_idx.ptr, 0, (size_t)e->cfg.chains * 4, e->stream));
  HIP_TRY(launch_sweeps(e, P, (int)nsweeps));
  return BA_OK;
}

int ba_adaptive_get_rates(ba_engine *e, int64_t chain, double *birth_rates,
                          double *death_rates, uint64_t *iteration_count) {
  ENGINE_PROLOGUE(e);
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  if (e->dada_birth.count == 0) return fail(BA_E_STATE, "no adaptive sweep yet");
  int rc = ba_sync(e);
  if (rc) return rc;
  const size_t p = (size_t)e->p;
  if (birth_rates) HIP_TRY(hipMemcpy(birth_rates, e->dada_birth.ptr + (size_t)chain * p, p * 8, hipMemcpyDeviceToHost));
  if (death_rates) HIP_TRY(hipMemcpy(death_rates, e->dada_death.ptr + (size_t)chain * p, p * 8, hipMemcpyDeviceToHost));
  if (iteration_count) HIP_TRY(hipMemcpy(iteration_count, e->dada_iter.ptr + chain, 8, hipMemcpyDeviceToHost));
  return BA_OK;
}

}  // extern "C"
