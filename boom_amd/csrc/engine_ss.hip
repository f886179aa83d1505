// Host side of the state-space samplers (bsts), the core: the launch parameters, ss_prepare, the data
// and the local-level model on the Kalman kernels and the round kernel, the rounds of a call
// (ss_sweep_impl), the catch-up of parked chains, and the plain accessors.
#include "engine_internal.h"

namespace boom_amd {

// per chain: K (m T) | state (m T) | smoothed disturbances (nvar T) | normals (<= (nvar + 1) T + m + 1)
int64_t ssm_work_stride(const ba_engine &e) {
  // (the template kernel keeps four disturbance series and up to five normals a step)
  // (general kernel: a smoothed-disturbance series per state-error row, and as many normals a step + 1)
  const int64_t per_step = std::max(2 * e.ssg.m + 2 * std::max(e.ssg.nvar, e.ssg.nerr) + 1, 2 * e.ssg.m + 9);
  return per_step * e.T + SSG_MAX_STATE + 72;
}

void fill_ss_params(ba_engine *e, SsParams &S) {
  std::memset(&S, 0, sizeof(S));  // (only_ran = nullptr: every chain)
  S.T = e->T;
  S.slot_limit = e->slot_limit;
  S.p = e->p;
  S.chains = e->cfg.chains;
  S.chain_first = 0;
  S.chain_count = e->cfg.chains;
  S.chain_offset = e->cfg.chain_offset;
  S.y = e->dss_y.ptr;
  S.X = e->dss_X.ptr;
  S.observed = e->dss_obs.ptr;
  S.Xt = e->dss_Xt.ptr;
  S.yt = e->dss_yt.ptr;
  S.obs_mask = e->dss_obs_mask.ptr;
  S.lane_major = ss_lane_major(*e) ? 1 : 0;
  S.TP = (int32_t)ss_pitch(*e);
  S.gamma = e->dgamma.ptr;
  S.beta = e->dbeta.ptr;
  S.sigsq = e->dsigsq.ptr;
  S.level_sigsq = e->dlev_sigsq.ptr;
  S.level_n = e->dlev_n.ptr;
  S.level_sumsq = e->dlev_sumsq.ptr;
  S.level_prior_df = e->level_prior_df;
  S.level_prior_ss = e->level_prior_ss;
  S.level_sigma_max = e->level_sigma_max;
  S.a0 = e->ss_a0;
  S.P0 = e->ss_P0;
  S.seed_lo = (uint32_t)e->seed;
  S.seed_hi = (uint32_t)(e->seed >> 32);
  S.pos_level = e->dpos_level.ptr;
  S.pos_state = e->dpos_state.ptr;
  S.status = e->dstatus.ptr;
  S.scratch = e->dss_scratch.ptr;
  S.scratch_stride = (int64_t)SS_SCRATCH_ARRAYS * (int64_t)ss_pitch(*e);
  S.xty = e->dxty_c.ptr;
  S.yty = e->dyty_c.ptr;
  S.nobs = e->dnobs_c.ptr;
  S.xte_planes = e->dxte_planes.ptr;
  S.prepared = 0;
  S.prep_n = e->dprep_n.ptr;
  S.prep_pos_state = e->dprep_pos_state.ptr;
  S.prep_pos_level = e->dprep_pos_level.ptr;
  S.prep_level_sigsq = e->dprep_level.ptr;
  S.zbuf = e->ss_zbuf;
  S.level_used = e->ssla.lev_used.ptr;
  if (e->ssm_set) {
    S.ssm.spec = reinterpret_cast<const SsgSpec *>(e->dssg_spec.ptr);
    S.ssm.m = e->ssg.m;
    S.ssm.nblocks = e->ssg.nblocks;
    S.ssm.nvar = e->ssg.nvar;
    S.ssm.nar = e->ssg.nar;
    S.ssm.ld = e->ssg.ld;
    S.ssm.bl = e->ssg.bl;
    S.ssm.nerr = e->ssg.nerr;
    S.ssm.ndyn = ssg_dyn_columns(e->ssg);
    if (e->ssg_kernel_choice == 1 || e->ssg_kernel_choice == 3)
      ssg_template_shape(e->ssg, &S.ssm.tpl_trend, &S.ssm.tpl_nseasons, &S.ssm.tpl_ar_lags);
    S.ssm.glob = 0;
    for (int b = 0; b < e->ssg.nblocks; ++b)
      if (e->ssg.blk[b].kind == SSG_TRIG || e->ssg.blk[b].kind == SSG_SEMILOCAL) S.ssm.glob = 1;
    S.ssm.var_sigsq = e->dssm_sigsq.ptr;
    S.ssm.var_n = e->dssm_n.ptr;
    S.ssm.var_ss = e->dssm_ss.ptr;
    S.ssm.pos_var = e->dpos_var.ptr;
    S.ssm.ar_phi = e->dar_phi.ptr;
    S.ssm.ar_suf = e->dar_suf.ptr;
    S.ssm.work = e->dssm_work.ptr;
    S.ssm.work_stride = ssm_work_stride(*e);
    if (e->ssg.student_block) {
      S.qw = e->dslt_w.ptr;
      S.qw_stride = 2 * (int64_t)e->T;
    }
    if (ssg_has(e->ssg, SSG_HAS_CALENDAR)) {
      S.cal = e->dhol_cal.ptr;   // (packed by hol_prepare, which every entry point that launches passes first)
      S.cal_count = e->hol_cal_count;
    }
    if (ssg_has(e->ssg, SSG_HAS_DYNREG)) {
      S.dyn = e->ddyn.ptr;   // (packed by hol_prepare too)
      S.dyn_rows = e->dyn_rows;
      S.dyn_cols = ssg_dyn_columns(e->ssg);
    }
    if (!e->rh_models.empty()) {
      // regression holiday models: every chain's series less their effects (rh_draw_kernel writes it)
      S.y = e->drh_y.ptr;
      S.y_stride = e->T;
      S.ssm.tpl_trend = S.ssm.tpl_nseasons = S.ssm.tpl_ar_lags = 0;   // (whatever ba_ss_set_tuning asked for)
    }
  }
}

// the list's regression holiday models (false: it has none)
bool fill_rh_params(ba_engine *e, RhParams &R) {
  R = RhParams{};
  if (!e->ssm_set || e->rh_models.empty()) return false;
  R.nmodels = (int32_t)e->rh_models.size();
  R.ncoef = e->rh_first[R.nmodels];
  R.nsteps = e->rh_nsteps;
  R.count = e->rh_count;
  R.table = e->drh_table.ptr;
  R.steps = e->drh_steps.ptr;
  R.counts = e->drh_counts.ptr;
  R.coef = e->drh_coef.ptr;
  R.totals = e->drh_totals.ptr;
  R.pos = e->drh_pos.ptr;
  R.y = e->drh_y.ptr;
  R.y_shared = e->dss_y.ptr;
  for (int k = 0; k <= RH_MAX_MODELS; ++k) R.first[k] = e->rh_first[k];
  for (int k = 0; k < R.nmodels; ++k) {
    R.prior_mean[k] = e->rh_models[(size_t)k].prior_mean;
    R.prior_sd[k] = e->rh_models[(size_t)k].prior_sd;
  }
  return true;
}

// the hierarchical ones among the list's regression holiday models (false: it has none)
bool fill_rhh_params(ba_engine *e, RhhParams &Q) {
  Q = RhhParams{};
  if (!e->ssm_set) return false;
  Q.nmodels = (int32_t)e->rh_models.size();
  for (int k = 0; k < Q.nmodels; ++k) {
    const RhModel &m = e->rh_models[(size_t)k];
    if (!m.hier) continue;
    Q.mask |= 1 << k;
    Q.width[k] = m.width;
    Q.nhol[k] = (int32_t)m.widths.size();
    Q.nu0[k] = m.nu0;
  }
  Q.hyper = e->drhh_hyper.ptr;
  Q.mu = e->drhh_mu.ptr;
  Q.omega = e->drhh_omega.ptr;
  Q.pos = e->drhh_pos.ptr;
  return Q.mask != 0;
}

// the list's spike-and-slab autoregressions (false: it has none)
bool fill_ar_spike_params(ba_engine *e, ArSpikeParams &U) {
  U = ArSpikeParams{};
  if (!e->ssm_set) return false;
  for (int b = 0; b < e->ssg.nblocks; ++b)
    if (e->ssg.blk[b].ar_spike) U.block[U.nspike++] = b;
  U.prior = reinterpret_cast<const ArSpikePrior *>(e->dar_spike_prior.ptr);
  U.gamma = reinterpret_cast<uint8_t *>(e->dar_gamma.ptr);
  return U.nspike > 0;
}

void fill_slt_params(ba_engine *e, SltParams &U) {
  U.w = e->dslt_w.ptr;
  U.res = e->dslt_res.ptr;
  U.nu = e->dslt_nu.ptr;
  U.wsuf = e->dslt_wsuf.ptr;
  U.pos = e->dslt_pos.ptr;
  U.count = e->dslt_count.ptr;
  for (int c = 0; c < 2; ++c) {
    U.nu_kind[c] = e->slt_nu_kind[c];
    U.nu_a[c] = e->slt_nu_a[c];
    U.nu_b[c] = e->slt_nu_b[c];
  }
}

// the state half of a state-space sweep: the structural kernel when a trend /
// seasonal specification is set, the local-level kernel otherwise
static hipError_t launch_state_models(ba_engine *e, const SsParams &S, int draw);
static hipError_t launch_state_kernel(ba_engine *e, const SsParams &S, int draw) {
  ArSpikeParams V;
  if (draw && fill_ar_spike_params(e, V)) {
    // the spike-and-slab autoregressions' samplers, ahead of the state kernel (which draws the
    // other state models' at its head and passes these by)
    hipError_t err = launch_ar_spike(e->stream, S, V);
    if (err != hipSuccess) return err;
  }
  RhParams R;
  if (fill_rh_params(e, R)) {
    // the regression holiday models: their sampler and the chains' series ahead of the state kernel (the
    // series every time: a setter may have changed the coefficients), their observe_state behind it
    // (a hierarchical model's sampler first: the plain kernel takes its coefficients as they then are and
    // writes the series from all models', in model order)
    RhhParams Q;
    const bool hier = fill_rhh_params(e, Q);
    hipError_t err = (draw && hier) ? launch_rhh_draw(e->stream, S, R, Q) : hipSuccess;
    if (err == hipSuccess) err = launch_rh_draw(e->stream, S, R, draw, Q.mask);
    if (err == hipSuccess) err = launch_state_models(e, S, draw);
    if (err == hipSuccess) err = launch_rh_observe(e->stream, S, R);
    return err;
  }
  return launch_state_models(e, S, draw);
}
static hipError_t launch_state_models(ba_engine *e, const SsParams &S, int draw) {
  if (e->ssm_set && e->ssg.student_block) {
    // a Student local linear trend: its sampler with the other state models' (they are drawn at the
    // head of the state kernel, every one from its own stream), and observe_state -- the new weights
    // and the block's statistics -- once the state draw is there
    SltParams U;
    fill_slt_params(e, U);
    hipError_t err = draw ? launch_slt_params(e->stream, S, U) : hipSuccess;
    if (err == hipSuccess) err = launch_ssm_simsmooth(e->stream, S, draw);
    if (err == hipSuccess) err = launch_slt_weights(e->stream, S, U);
    return err;
  }
  return e->ssm_set ? launch_ssm_simsmooth(e->stream, S, draw)
                    : launch_kalman_simsmooth(e->stream, S, draw);
}

// The same for the state-space path, where a chain's sweeps alternate with the
// Kalman kernel: a chain that outgrew the capacity sat out the rest of the call
// (its SSVS launches booked the sweeps, its Kalman launches were skipped), so
// it is caught up one (SSVS, Kalman) pair at a time; chains that owe nothing
// leave both kernels at once.
int ss_escalate(ba_engine *e, std::vector<int32_t> &st) {
  const size_t C = (size_t)e->cfg.chains;
  for (;;) {
    bool any = false;
    for (size_t c = 0; c < C; ++c) any = any || (st[c] == CHAIN_MODEL_TOO_LARGE);
    if (!any) return BA_OK;
    if (e->cfg.max_model_size_hint > 0) return BA_OK;  // stays an error
    const bool to_big = e->kcap >= cap_limit(*e);
    if (to_big) {
      int stuck = 0;
      int rc = grow_big(e, &stuck);
      if (rc) return rc;
      if (stuck) return BA_OK;
    } else {
      e->kcap += 16;
      e->waves = choose_waves(*e, e->kcap);
    }
    std::vector<int32_t> todo(C);
    HIP_TRY(hipMemcpy(todo.data(), e->dtodo.ptr, C * 4, hipMemcpyDeviceToHost));
    int rounds = 0;
    for (size_t c = 0; c < C; ++c) {
      if (st[c] == CHAIN_MODEL_TOO_LARGE) {
        if (!to_big) st[c] = CHAIN_OK;   // (the large-model kernel takes parked chains as they are)
        rounds = std::max(rounds, (int)todo[c]);
      }
    }
    HIP_TRY(hipMemcpyAsync(e->dstatus.ptr, st.data(), C * 4, hipMemcpyHostToDevice, e->stream));
    SsvsParams P;
    fill_params(e, P);
    P.run_limit = 1;
    P.ran = e->dran.ptr;
    SsParams S;
    fill_ss_params(e, S);
    S.only_ran = e->dran.ptr;
    for (int r = 0; r < rounds; ++r) {
      HIP_TRY(launch_sweeps(e, P, 0));
      HIP_TRY(launch_state_kernel(e, S, 1));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(st.data(), e->dstatus.ptr, C * 4, hipMemcpyDeviceToHost));
  }
}

// what every state-space entry point passes before it launches: the refusals, the calendars, the
// chains' buffers for the current specification and their initial values
int ss_prepare(ba_engine *e, DataKind kind) {
  int rc = sweep_refusal(e, kind);
  if (rc) return rc;
  if (!e->ss_level_set && !e->ssm_set)
    return fail(BA_E_STATE, "call ba_ss_set_local_level or ba_ss_set_structural first");
  rc = ss_refused(e, kind, SSG_USE_LAUNCH);
  if (rc) return rc;
  rc = hol_prepare(e);
  if (rc) return rc;
  rc = upload_shared(e);
  if (rc) return rc;
  rc = alloc_chain_state(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, T = ss_pitch(*e);
  if (e->dss_scratch.count != C * SS_SCRATCH_ARRAYS * T) {
    HIP_TRY(e->dss_scratch.resize(C * SS_SCRATCH_ARRAYS * T));
    HIP_TRY(e->dxty_c.resize(C * p));
    HIP_TRY(e->dyty_c.resize(C));
    HIP_TRY(e->dnobs_c.resize(C));
    HIP_TRY(e->dlev_sigsq.resize(C));
    HIP_TRY(e->dlev_n.resize(C));
    HIP_TRY(e->dlev_sumsq.resize(C));
    HIP_TRY(e->dpos_level.resize(C));
    HIP_TRY(e->dpos_state.resize(C));
    HIP_TRY(e->dpos_forecast.resize(C));
    HIP_TRY(hipMemsetAsync(e->dpos_forecast.ptr, 0, C * 8, e->stream));
    HIP_TRY(e->dprep_n.resize(2 * C));
    HIP_TRY(e->dprep_pos_state.resize(2 * C));
    HIP_TRY(e->dprep_pos_level.resize(2 * C));
    HIP_TRY(e->dprep_level.resize(2 * C));
    HIP_TRY(hipMemsetAsync(e->dprep_n.ptr, 0, 2 * C * 4, e->stream));
    e->ss_zbuf = 0;
    HIP_TRY(e->dxte_planes.resize((size_t)xte_planes((int64_t)T) * C * p));
    // regression suf starts as the data's own (before the first impute_state)
    std::vector<double> xty(C * p), yty(C, e->yty), nobs(C, e->n),
        lev(C, e->ss_initial_level_sigsq);
    for (size_t c = 0; c < C; ++c) std::memcpy(&xty[c * p], e->xty.data(), p * 8);
    hipStream_t s = e->stream;
    HIP_TRY(hipMemcpyAsync(e->dxty_c.ptr, xty.data(), xty.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dyty_c.ptr, yty.data(), C * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dnobs_c.ptr, nobs.data(), C * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dlev_sigsq.ptr, lev.data(), C * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(e->dlev_n.ptr, 0, C * 8, s));
    HIP_TRY(hipMemsetAsync(e->dlev_sumsq.ptr, 0, C * 8, s));
    HIP_TRY(hipMemsetAsync(e->dpos_level.ptr, 0, C * 8, s));
    HIP_TRY(hipMemsetAsync(e->dpos_state.ptr, 0, C * 8, s));
    HIP_TRY(hipMemsetAsync(e->dss_scratch.ptr, 0, C * SS_SCRATCH_ARRAYS * T * 8, s));
    if (e->ssm_set) {
      const size_t NV = SSG_MAX_VAR;
      HIP_TRY(e->dssm_sigsq.resize(C * NV));
      HIP_TRY(e->dssm_n.resize(C * NV));
      HIP_TRY(e->dssm_ss.resize(C * NV));
      HIP_TRY(e->dpos_var.resize(C * NV));
      HIP_TRY(e->dssm_work.resize(C * (size_t)ssm_work_stride(*e)));
      HIP_TRY(e->dssg_spec.resize(sizeof(SsgSpec)));
      HIP_TRY(hipMemcpy(e->dssg_spec.ptr, &e->ssg, sizeof(SsgSpec), hipMemcpyHostToDevice));
      std::vector<double> v0(C * NV);
      for (size_t c = 0; c < C; ++c)
        for (size_t i = 0; i < NV; ++i) v0[c * NV + i] = e->ssg_initial_sigsq[i];
      HIP_TRY(hipMemcpy(e->dssm_sigsq.ptr, v0.data(), C * NV * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemsetAsync(e->dssm_n.ptr, 0, C * NV * 8, s));
      HIP_TRY(hipMemsetAsync(e->dssm_ss.ptr, 0, C * NV * 8, s));
      HIP_TRY(hipMemsetAsync(e->dpos_var.ptr, 0, C * NV * 8, s));
      HIP_TRY(hipMemsetAsync(e->dssm_work.ptr, 0, C * (size_t)ssm_work_stride(*e) * 8, s));
      if (e->ssg.nar > 0) {
        HIP_TRY(e->dar_phi.resize(C * SSG_MAX_AR * AR_MAX));
        HIP_TRY(e->dar_suf.resize(C * SSG_MAX_AR * AR_SUF_STRIDE));
        std::vector<double> ph(C * SSG_MAX_AR * AR_MAX, 0.0);
        for (size_t c = 0; c < C; ++c)
          for (int a = 0; a < SSG_MAX_AR; ++a)
            for (int i = 0; i < AR_MAX; ++i) ph[(c * SSG_MAX_AR + a) * AR_MAX + i] = e->ssg_initial_phi[a][i];
        HIP_TRY(hipMemcpy(e->dar_phi.ptr, ph.data(), ph.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(e->dar_suf.ptr, 0, C * SSG_MAX_AR * AR_SUF_STRIDE * 8, s));
      }
      e->dar_gamma.release();
      {
        // ArModel(lags) includes every lag (add_all), whatever the initial coefficients are
        std::vector<uint8_t> g(C * SSG_MAX_AR * AR_MAX, 0);
        bool any = false;
        for (int b = 0; b < e->ssg.nblocks; ++b) {
          const SsgBlock &k = e->ssg.blk[b];
          if (!k.ar_spike) continue;
          any = true;
          for (size_t c = 0; c < C; ++c)
            for (int i = 0; i < k.lags; ++i) g[(c * SSG_MAX_AR + k.ar_index) * AR_MAX + i] = 1;
        }
        if (any) {
          HIP_TRY(e->dar_gamma.resize(g.size() / 8));
          HIP_TRY(hipMemcpy(e->dar_gamma.ptr, g.data(), g.size(), hipMemcpyHostToDevice));
          HIP_TRY(e->dar_spike_prior.resize(sizeof(e->ar_spike_prior)));
          HIP_TRY(hipMemcpy(e->dar_spike_prior.ptr, e->ar_spike_prior, sizeof(e->ar_spike_prior), hipMemcpyHostToDevice));
        }
      }
      if (e->ssg.student_block) {
        // a new StudentLocalLinearTrendStateModel: weights 1, no residuals, empty statistics
        const size_t TT = (size_t)e->T;
        HIP_TRY(e->dslt_w.resize(C * 2 * TT));
        HIP_TRY(e->dslt_res.resize(C * 2 * TT));
        HIP_TRY(e->dslt_nu.resize(C * 2));
        HIP_TRY(e->dslt_wsuf.resize(C * 6));
        HIP_TRY(e->dslt_pos.resize(C));
        HIP_TRY(e->dslt_count.resize(C));
        std::vector<double> one(C * 2 * TT, 1.0), nu0(C * 2);
        for (size_t c = 0; c < C; ++c) { nu0[2 * c] = e->slt_initial_nu[0]; nu0[2 * c + 1] = e->slt_initial_nu[1]; }
        HIP_TRY(hipMemcpy(e->dslt_w.ptr, one.data(), one.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->dslt_nu.ptr, nu0.data(), nu0.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(e->dslt_res.ptr, 0, C * 2 * TT * 8, s));
        HIP_TRY(hipMemsetAsync(e->dslt_wsuf.ptr, 0, C * 6 * 8, s));
        HIP_TRY(hipMemsetAsync(e->dslt_pos.ptr, 0, C * 8, s));
        HIP_TRY(hipMemsetAsync(e->dslt_count.ptr, 0, C * 8, s));
      }
    }
    if (e->ssm_set && !e->rh_models.empty()) {
      // new RegressionHolidayStateModels: the initial coefficients, empty totals (as the variance
      // statistics before the first state draw), the sampler's stream at its start
      HIP_TRY(e->drh_coef.resize(C * RH_MAX_COEF));
      HIP_TRY(e->drh_totals.resize(C * RH_MAX_COEF));
      HIP_TRY(e->drh_pos.resize(C));
      std::vector<double> c0(C * RH_MAX_COEF, 0.0);
      for (size_t c = 0; c < C; ++c)
        for (size_t k = 0; k < e->rh_models.size(); ++k)
          std::copy(e->rh_models[k].initial.begin(), e->rh_models[k].initial.end(), c0.begin() + c * RH_MAX_COEF + e->rh_first[k]);
      HIP_TRY(hipMemcpy(e->drh_coef.ptr, c0.data(), c0.size() * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemsetAsync(e->drh_totals.ptr, 0, C * RH_MAX_COEF * 8, s));
      HIP_TRY(hipMemsetAsync(e->drh_pos.ptr, 0, C * 8, s));
      // ... and the hierarchical ones' hyperparameters, mu and Omega as the models were added with
      const size_t W = RHH_MAX_WIDTH, MU = RH_MAX_MODELS * W, OM = RH_MAX_MODELS * W * W;
      HIP_TRY(e->drhh_hyper.resize(RH_MAX_MODELS * RHH_HYPER_STRIDE));
      HIP_TRY(e->drhh_mu.resize(C * MU));
      HIP_TRY(e->drhh_omega.resize(C * OM));
      HIP_TRY(e->drhh_pos.resize(C));
      std::vector<double> hy(RH_MAX_MODELS * RHH_HYPER_STRIDE, 0.0), mu0(C * MU, 0.0), om0(C * OM, 0.0);
      for (size_t k = 0; k < e->rh_models.size(); ++k) {
        const RhModel &m = e->rh_models[k];
        if (!m.hier) continue;
        const size_t d = (size_t)m.width;
        double *h = hy.data() + k * RHH_HYPER_STRIDE;
        for (size_t r = 0; r < d; ++r) {
          h[RHH_HYPER_SINV0MU0 + r] = m.sinv0mu0[r];
          for (size_t c2 = 0; c2 < d; ++c2) {
            h[RHH_HYPER_SINV0 + r * W + c2] = m.sinv0[r * d + c2];
            h[RHH_HYPER_S0 + r * W + c2] = m.s0[r * d + c2];
          }
        }
        for (size_t c = 0; c < C; ++c)
          for (size_t r = 0; r < d; ++r) {
            mu0[c * MU + k * W + r] = m.initial_mu[r];
            for (size_t c2 = 0; c2 < d; ++c2) om0[c * OM + k * W * W + r * W + c2] = m.initial_omega[r * d + c2];
          }
      }
      HIP_TRY(hipMemcpy(e->drhh_hyper.ptr, hy.data(), hy.size() * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(e->drhh_mu.ptr, mu0.data(), mu0.size() * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(e->drhh_omega.ptr, om0.data(), om0.size() * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemsetAsync(e->drhh_pos.ptr, 0, C * 8, s));
    }
    HIP_TRY(hipStreamSynchronize(s));  // (the host vectors above go out of scope)
    e->ss_initialized = false;
  }
  HIP_TRY(e->dmodel.resize(2 * (size_t)e->cfg.chains * ssvs_scalar_layout(64).total));
  return BA_OK;
}

}  // namespace boom_amd

extern "C" {

int ba_ss_set_data(ba_engine *e, int32_t T, int32_t p, const double *y,
                   const double *X, const uint8_t *observed) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!y || !X) return fail(BA_E_INVALID, "null argument");
  if (T <= 0 || p <= 0) return fail(BA_E_INVALID, "T and p must be positive");
  // The regression model's fixed XtX (and the initial Xty, ...) are over the
  // OBSERVED rows only: missing points never update the sufficient statistics
  // (StateSpaceRegressionModel.cpp:100-125, SufstatDataPolicy.hpp:166-167).
  std::vector<double> Xo((size_t)T * p), yo(T);
  std::vector<uint8_t> obs(T, 1);
  double nobs = 0;
  e->rh_count = 0;   // (the regression holidays' counts and series follow the data)
  for (int t = 0; t < T; ++t) {
    if (observed) obs[t] = observed[t] ? 1 : 0;
    nobs += obs[t];
    yo[t] = obs[t] ? y[t] : 0.0;
  }
  for (int j = 0; j < p; ++j)
    for (int t = 0; t < T; ++t)
      Xo[(size_t)j * T + t] = obs[t] ? X[(size_t)j * T + t] : 0.0;
  int rc = ba_build_suf_from_xy(e, T, p, Xo.data(), yo.data());
  if (rc) return rc;
  e->n = nobs;
  e->T = T;
  HIP_TRY(e->dss_y.resize(T));
  HIP_TRY(e->dss_X.resize((size_t)T * p));
  HIP_TRY(e->dss_obs.resize(T));
  HIP_TRY(hipMemcpy(e->dss_y.ptr, y, (size_t)T * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->dss_X.ptr, X, (size_t)T * p * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->dss_obs.ptr, obs.data(), T, hipMemcpyHostToDevice));
  e->ss_observed = obs;
  if (T <= LM_TP) {
    std::vector<double> Xt((size_t)LM_TP * p, 0.0), yt(LM_TP, 0.0);
    std::vector<uint32_t> mask(LM_THREADS, 0u);
    for (int t = 0; t < T; ++t) {
      yt[lm_at(t)] = y[t];
      if (obs[t]) mask[t / LM_BS] |= 1u << (t % LM_BS);
    }
    for (int j = 0; j < p; ++j)
      for (int t = 0; t < T; ++t) Xt[(size_t)j * LM_TP + lm_at(t)] = X[(size_t)j * T + t];
    HIP_TRY(e->dss_yt.resize(LM_TP));
    HIP_TRY(e->dss_Xt.resize((size_t)LM_TP * p));
    HIP_TRY(e->dss_obs_mask.resize(LM_THREADS));
    HIP_TRY(hipMemcpy(e->dss_yt.ptr, yt.data(), (size_t)LM_TP * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->dss_Xt.ptr, Xt.data(), (size_t)LM_TP * p * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->dss_obs_mask.ptr, mask.data(), LM_THREADS * 4, hipMemcpyHostToDevice));
  } else {
    e->dss_yt.release();
    e->dss_Xt.release();
    e->dss_obs_mask.release();
  }
  e->ss_initialized = false;
  e->dss_scratch.release();
  e->device_dirty = true;
  e->data_kind = DATA_STATE_SPACE;
  return BA_OK;
}

int ba_ss_set_local_level(ba_engine *e, double level_df, double level_sigma_guess,
                          double level_sigma_upper_limit,
                          double initial_state_mean,
                          double initial_state_variance,
                          double initial_level_sigma) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (level_sigma_upper_limit < 0 || initial_state_variance < 0)
    return fail(BA_E_INVALID, "sigma_max must be non-negative.");
  // ChisqModel(df, sigma_guess): 2 alpha = df, 2 beta = df sigma^2
  e->level_prior_df = 2 * (level_df / 2.0);
  e->level_prior_ss = 2 * (level_df * level_sigma_guess * level_sigma_guess / 2.0);
  e->level_sigma_max = level_sigma_upper_limit;
  e->ss_a0 = initial_state_mean;
  e->ss_P0 = initial_state_variance;
  e->ss_initial_level_sigsq = initial_level_sigma * initial_level_sigma;
  e->ss_level_set = true;
  e->ssm_set = false;
  e->dss_scratch.release();
  return BA_OK;
}

// diagnostic, changes no draw: 0 = the general kernel also where the shape-specialised one
// applies (the two are compared by the tests), 1 = the default
int ba_ss_set_tuning(ba_engine *e, int32_t kernel) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (kernel < 0 || kernel > 7 || kernel == 2)
    return fail(BA_E_INVALID, "kernel must be 0, 1, 3, 4, 5, 6 or 7 (2, four chains per wavefront, was removed: it never won)");
  MUTATE(e);
  // 4 / 5: the local-level rounds as the separate launches of rounds 1-4 / as the round
  // kernel (the default where it applies); the structural kernels' choice stays
  // 6 / 7: the round kernel's diagnostic notes (printed when a chain stops) on / off
  if (kernel >= 6) e->round_debug = kernel == 6;
  else if (kernel >= 4) e->ss_round_enabled = kernel == 5;
  else e->ssg_kernel_choice = kernel;
  return BA_OK;
}

// one chain's state draw, T x m (step t at [t * m, (t + 1) * m))
int ba_ss_get_state_draw(ba_engine *e, int64_t chain, double *state) {
  ENGINE_ACCESSOR_SERVED(e);
  if (!ss_kind(e->data_kind) || !e->ssm_set || e->dssm_work.count == 0)
    return fail(BA_E_STATE, "no structural state-space run yet");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  if (!state) return fail(BA_E_INVALID, "null argument");
  if (ss_la_serving(e)) {
    if (ss_la_registered(e, chain)) {
      const ba_engine::SsLa::Rows *r = nullptr;
      int rcr = ss_la_rows(e, chain, true, &r);
      if (rcr) return rcr;
      const size_t SD = e->ssla.state_doubles;
      std::memcpy(state, &r->state[((size_t)e->ssla.served - 1) * SD], SD * 8);
      return BA_OK;
    }
    ss_la_want_state(e, chain);
    int rcs = ss_la_settle(e);
    if (rcs) return rcs;
  }
  int rc = ba_sync(e);
  if (rc) return rc;
  const size_t T = (size_t)e->T, m = (size_t)e->ssg.m;
  HIP_TRY(pinned_reserve(e, m * T * 8));
  HIP_TRY(hipMemcpyAsync(e->pinned, e->dssm_work.ptr + (size_t)chain * ssm_work_stride(*e) + m * T, m * T * 8,
                         hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::memcpy(state, e->pinned, m * T * 8);
  return BA_OK;
}

int ba_ss_get_structural(ba_engine *e, int64_t chain, double *state, double *variances,
                         double *suf_n, double *suf_ss) {
  ENGINE_ACCESSOR_SERVED(e);
  if (!ss_kind(e->data_kind) || !e->ssm_set || e->dssm_work.count == 0)
    return fail(BA_E_STATE, "no structural state-space run yet");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  if ((variances || suf_n || suf_ss) && e->ssg_template_var[0] < 0)
    return fail(BA_E_STATE, "the state was not set with ba_ss_set_structural: use ba_ss_get_state_model");
  if (ss_la_serving(e)) {
    if (!suf_n && !suf_ss && (!state || ss_la_registered(e, chain))) {
      const ba_engine::SsLa::Rows *r = nullptr;
      int rcr = ss_la_rows(e, chain, state != nullptr, &r);
      if (rcr) return rcr;
      const size_t row = (size_t)e->ssla.served - 1, SD = e->ssla.state_doubles;
      if (state) std::memcpy(state, &r->state[row * SD], SD * 8);
      if (variances)
        for (int i = 0; i < 3; ++i) {
          const int vi = e->ssg_template_var[i];
          variances[i] = vi >= 0 ? r->var[row * e->ssla.nvar + vi] : 0.0;
        }
      return BA_OK;
    }
    if (state) ss_la_want_state(e, chain);
    int rcs = ss_la_settle(e);
    if (rcs) return rcs;
  }
  if (state) {
    const int rc = ba_ss_get_state_draw(e, chain, state);
    if (rc) return rc;
  }
  int rc = ba_sync(e);
  if (rc) return rc;
  // (one batch through the pinned staging buffer: variances | n | sums of squares)
  const size_t NV = SSG_MAX_VAR;
  HIP_TRY(pinned_reserve(e, 3 * NV * 8));
  double *hv = (double *)e->pinned;
  HIP_TRY(hipMemcpyAsync(hv, e->dssm_sigsq.ptr + chain * NV, NV * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(hv + NV, e->dssm_n.ptr + chain * NV, NV * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(hv + 2 * NV, e->dssm_ss.ptr + chain * NV, NV * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int i = 0; i < 3; ++i) {
    const int vi = e->ssg_template_var[i];
    // (an unused slot reports what it was given: the initial value, no statistics)
    if (variances) variances[i] = vi >= 0 ? hv[vi] : 0.0;
    if (suf_n) suf_n[i] = vi >= 0 ? hv[NV + vi] : 0.0;
    if (suf_ss) suf_ss[i] = vi >= 0 ? hv[2 * NV + vi] : 0.0;
  }
  return BA_OK;
}

int ba_ss_impute_state(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  e->table_ok = false;
  int rc = ss_prepare(e);
  if (rc) return rc;
  SsParams S;
  fill_ss_params(e, S);
  HIP_TRY(launch_state_kernel(e, S, 0));
  e->ss_initialized = true;
  return BA_OK;
}

}  // extern "C"

namespace boom_amd {

#ifdef BA_RSTAMPS
static double *g_round_stamps = nullptr;
static size_t g_round_stamps_n = 0;
#endif
// The round kernel (ss_round_kernel.hip) serves the local-level model on a series of at most
// LM_TP steps while every chain is in the LDS sweep kernel's range; how many chains one launch
// can take (0: the separate launches instead).
static int ss_round_chains(ba_engine *e) {
  if (!e->ss_round_enabled || e->ssm_set || !ss_lane_major(*e) || e->big_active || e->cur_mode != 0) return 0;
  if (e->kcap != 16 && e->kcap != 32 && e->kcap != 48) return 0;
  int &res = e->ss_round_resident[e->kcap / 16];
  if (res == 0) {
    res = -1;
    if (ss_round_lds(e->p, e->kcap) <= (size_t)e->lds_per_cu / 2) {   // (two chains to a CU at least)
      SsvsParams P{};
      SsParams S{};
      SsRoundParams F{};
      P.kcap = e->kcap;
      P.p = e->p;
      int n = 0;
      if (launch_ss_round(e->stream, P, S, F, &n) == hipSuccess && n > 0) res = n;
      if (e->round_debug) std::fprintf(stderr, "round kernel: kcap %d lds %zu resident %d\n", e->kcap, ss_round_lds(e->p, e->kcap), n);
    }
  }
  return res > 0 ? std::min<int>(res, e->cfg.chains) : 0;
}

// `rounds` rounds of every chain: one launch per group of co-resident chains and per
// SS_ROUND_MAX_ROUNDS rounds; round i of the call goes to row rec_first + i of the record
static int ss_round_launches(ba_engine *e, SsvsParams &P, SsParams &S, int rounds, int rec_slot) {
  const int per = ss_round_chains(e), C = e->cfg.chains;
  const size_t ctl = (size_t)SS_ROUND_MAX_ROUNDS * (1 + 2 * (size_t)per);   // (ticket | sizes | diagnostic variants: a done count per tile)
  const size_t mem = (size_t)SS_ROUND_MAX_ROUNDS * ((size_t)per * SS_ROUND_TILE + 2 * SS_ROUND_TILE);
  if (e->dround_ctl.count != ctl) HIP_TRY(e->dround_ctl.resize(ctl));
  if (e->dround_members.count != mem) HIP_TRY(e->dround_members.resize(mem));
  SsRoundParams F{};
  F.close_ticks = 100000;   // 1 ms: a tile is short of members only when another launch shares the machine (ss_round_kernel.hip)
  F.ticket = e->dround_ctl.ptr;
  F.sizes = F.ticket + SS_ROUND_MAX_ROUNDS;
  F.members = e->dround_members.ptr;
  F.planes = e->dxte_planes.ptr;
  if (e->round_debug) {
    if (e->dround_debug.count == 0) {
      HIP_TRY(e->dround_debug.resize(16 * 17 + 64));
      HIP_TRY(hipMemset(e->dround_debug.ptr, 0, (16 * 17 + 64) * 4));
    }
    F.debug = e->dround_debug.ptr;
  }
#ifdef BA_RSTAMPS
  {  // (diagnostic build: printed per call by tools/ss_round_phases.py through BA_RSTAMPS_DUMP)
    static DevBuf<double> stamps;
    if (stamps.count != (size_t)C * 16) {
      HIP_TRY(stamps.resize((size_t)C * 16));
      HIP_TRY(hipMemsetAsync(stamps.ptr, 0, (size_t)C * 16 * 8, e->stream));
    }
    F.stamps = stamps.ptr;
    g_round_stamps = stamps.ptr;
    g_round_stamps_n = (size_t)C * 16;
  }
#endif
  if (rec_slot >= 0) {
    ba_engine::SsLa &A = e->ssla;
    F.rgamma = A.rgamma.ptr;
    F.rbeta = A.rbeta.ptr;
    F.rsig = A.rsig.ptr;
    F.rvar = A.rvar.ptr;
    F.rstate = A.rstate.ptr;
    F.reg_of_chain = e->dround_reg.ptr;
    F.rec_slot = rec_slot;
    F.rec_len = A.len;
    F.nreg = (int32_t)A.reg.size();
  }
  for (int g0 = 0; g0 < C; g0 += per) {
    const int gc = std::min(per, C - g0);
    SsvsParams Pg = P;
    SsParams Sg = S;
    Pg.chain_first = Sg.chain_first = g0;
    Pg.chain_count = Sg.chain_count = gc;
    for (int r0 = 0; r0 < rounds; r0 += SS_ROUND_MAX_ROUNDS) {
      F.rounds = std::min<int>(SS_ROUND_MAX_ROUNDS, rounds - r0);
      F.rec_first = r0;
#ifdef BA_RSTAMPS
      { static int seq = 0; F.debug_seq = ++seq; }
#endif
      HIP_TRY(hipMemsetAsync(e->dround_ctl.ptr, 0, ctl * 4, e->stream));
      HIP_TRY(hipMemsetAsync(e->dround_members.ptr, 0xff, mem * 4, e->stream));
      HIP_TRY(launch_ss_round(e->stream, Pg, Sg, F, nullptr));
      Pg.model_keep = 1;   // (from here on the chains' model blocks are their own last launch's)
    }
  }
  P.model_keep = 1;
  e->model_ok = true;
  return BA_OK;
}

// nsweeps x StateSpacePosteriorSampler::draw on every chain; rec_slot >= 0: every round's
// draw goes to that half of the look-ahead's record
int ss_sweep_impl(ba_engine *e, int32_t nsweeps, int rec_slot) {
  e->table_ok = false;
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = ss_prepare(e);
  if (rc) return rc;
  SsvsParams P;
  fill_params(e, P);
  SsParams S;
  fill_ss_params(e, S);
  // StateSpacePosteriorSampler::draw (StateSpacePosteriorSampler.cpp:42-64)
  if (!e->ss_initialized) {
    HIP_TRY(launch_state_kernel(e, S, 0));
    e->ss_initialized = true;
  }
  // The local-level state draw in two pieces: what does not depend on the round's
  // regression sweep (level variance, the normals) is done ahead on a second stream into
  // the chains' other normals buffer -- the step for round i + 1 goes out behind round
  // i's state draw, beside its X'e GEMM, its plane sum and the start of round i + 1's
  // SSVS launch (kalman_prepare_kernel).
  if (nsweeps > 0 && ss_round_chains(e) > 0) return ss_round_launches(e, P, S, nsweeps, rec_slot);
  const bool ahead = !e->ssm_set && nsweeps > 0;
  if (ahead && !e->stream2) {
    {
      int rcs = concurrent_stream(e, &e->stream2);
      if (rcs) return rcs;
    }
    HIP_TRY(hipEventCreateWithFlags(&e->ev_state, hipEventDisableTiming));
    for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&e->ev_prep[i], hipEventDisableTiming));
  }
  auto prepare_ahead = [&](int zbuf) -> hipError_t {
    // (after everything enqueued on the main stream so far: the chains' status words of the
    // sweep just launched, the buffer's last reader)
    hipError_t err = hipEventRecord(e->ev_state, e->stream);
    if (err != hipSuccess) return err;
    err = hipStreamWaitEvent(e->stream2, e->ev_state, 0);
    if (err != hipSuccess) return err;
    SsParams A = S;
    A.zbuf = zbuf;
    err = launch_kalman_prepare(e->stream2, A, 1);
    if (err != hipSuccess) return err;
    return hipEventRecord(e->ev_prep[zbuf], e->stream2);
  };
  if (ahead) {
    HIP_TRY(prepare_ahead(e->ss_zbuf));   // the call's first round: nothing to run beside
    S.prepared = 1;
  }
  for (int i = 0; i < nsweeps; ++i) {
    HIP_TRY(launch_sweeps(e, P, 1));                  // observation model
    if (ahead) {
      const int cur = e->ss_zbuf;
      HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_prep[cur], 0));
      S.zbuf = cur;
      HIP_TRY(launch_kalman_main(e->stream, S, 1));   // state models, state
      // (the state draw's wavefronts fill the register files -- 2 x 256 registers to a
      // SIMD -- so a prepare step launched beside it only delays it: it goes out behind)
      if (i + 1 < nsweeps) HIP_TRY(prepare_ahead(cur ^ 1));
      // ... and the regression's X'e: inside a call the plane sum is left to the next
      // round's sweep launch (one wave per chain on this path)
      const bool fold = i + 1 < nsweeps && !e->big_active && e->waves == 1 && e->cur_mode != 2;
      HIP_TRY(launch_kalman_xte(e->stream, S, fold));
      P.xty_planes = fold ? e->dxte_planes.ptr : nullptr;
      P.xty_nplanes = xte_planes((int64_t)S.TP);
      P.xty_plane_stride = (int64_t)e->cfg.chains * e->p;
      e->ss_zbuf = cur ^ 1;
    } else {
      HIP_TRY(launch_state_kernel(e, S, 1));          // state models, state
    }
    if (rec_slot >= 0) HIP_TRY(ss_la_record(e, rec_slot, i));
    P.model_keep = 1;  // from here on the chains' model blocks are their own last launch's
    e->model_ok = true;
  }
  return BA_OK;
}

}  // namespace boom_amd

extern "C" {

int ba_ss_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);   // (unserved look-ahead draws: the rounds asked for here come after the last one served)
  return ss_sweep_impl(e, nsweeps, -1);
}

int ba_ss_get_state(ba_engine *e, int64_t chain, double *state,
                    double *level_sigsq, double *level_n, double *level_sumsq) {
  ENGINE_ACCESSOR_SERVED(e);
  if (e->data_kind != DATA_STATE_SPACE || e->dss_scratch.count == 0) return fail(BA_E_STATE, "no state-space run yet");
  if (e->ssm_set) return fail(BA_E_STATE, "a structural state is set: use ba_ss_get_structural");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  if (ss_la_serving(e)) {
    if (!level_n && !level_sumsq && (!state || ss_la_registered(e, chain))) {
      // the draw ba_ss_draw_next is serving, from the record
      const ba_engine::SsLa::Rows *r = nullptr;
      int rcr = ss_la_rows(e, chain, state != nullptr, &r);
      if (rcr) return rcr;
      const size_t row = (size_t)e->ssla.served - 1, T = (size_t)e->T, SD = e->ssla.state_doubles;
      if (level_sigsq) *level_sigsq = r->var[row];
      if (state) {
        const double *src = &r->state[row * SD];
        if (ss_lane_major(*e)) {
          for (size_t t = 0; t < T; ++t) state[t] = src[(size_t)lm_at((int)t)];
        } else {
          std::memcpy(state, src, T * 8);
        }
      }
      return BA_OK;
    }
    if (state) ss_la_want_state(e, chain);
    int rcs = ss_la_settle(e);   // (not in the record: the chains go back to the draw being served)
    if (rcs) return rcs;
  }
  int rc = ba_sync(e);
  if (rc) return rc;
  // (one batch through the pinned staging buffer: state | level variance | n | sum of squares)
  const size_t T = (size_t)e->T, TP = ss_pitch(*e);
  HIP_TRY(pinned_reserve(e, (TP + 3) * 8));
  double *hstate = (double *)e->pinned, *hl = hstate + TP;
  if (state)
    HIP_TRY(hipMemcpyAsync(hstate, e->dss_scratch.ptr + ((size_t)chain * SS_SCRATCH_ARRAYS + SS_STATE_ARRAY) * TP,
                           (ss_lane_major(*e) ? TP : T) * 8, hipMemcpyDeviceToHost, e->stream));
  if (level_sigsq) HIP_TRY(hipMemcpyAsync(hl, e->dlev_sigsq.ptr + chain, 8, hipMemcpyDeviceToHost, e->stream));
  if (level_n) HIP_TRY(hipMemcpyAsync(hl + 1, e->dlev_n.ptr + chain, 8, hipMemcpyDeviceToHost, e->stream));
  if (level_sumsq) HIP_TRY(hipMemcpyAsync(hl + 2, e->dlev_sumsq.ptr + chain, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (state) {
    if (ss_lane_major(*e)) {
      for (size_t t = 0; t < T; ++t) state[t] = hstate[(size_t)lm_at((int)t)];
    } else {
      std::memcpy(state, hstate, T * 8);
    }
  }
  if (level_sigsq) *level_sigsq = hl[0];
  if (level_n) *level_n = hl[1];
  if (level_sumsq) *level_sumsq = hl[2];
  return BA_OK;
}

int ba_ss_set_level_sigsq(ba_engine *e, int64_t chain, double sigsq) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  int rc = ss_prepare(e);
  if (rc) return rc;
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  return write_per_chain(e, e->dlev_sigsq.ptr, chain, sigsq);
}

int ba_ss_get_chain_suf(ba_engine *e, int64_t chain, double *xty, double *yty,
                        double *n) {
  ENGINE_PROLOGUE(e);
  if (e->data_kind != DATA_STATE_SPACE || e->dxty_c.count == 0) return fail(BA_E_STATE, "no state-space run yet");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = ba_sync(e);
  if (rc) return rc;
  const size_t p = (size_t)e->p;
  if (xty) HIP_TRY(hipMemcpy(xty, e->dxty_c.ptr + (size_t)chain * p, p * 8, hipMemcpyDeviceToHost));
  if (yty) HIP_TRY(hipMemcpy(yty, e->dyty_c.ptr + chain, 8, hipMemcpyDeviceToHost));
  if (n) HIP_TRY(hipMemcpy(n, e->dnobs_c.ptr + chain, 8, hipMemcpyDeviceToHost));
  return BA_OK;
}

}  // extern "C"

#ifdef BA_RSTAMPS
// diagnostic build only (tools/build/libboomamd_rstamps.so): the round kernel's phase ticks
// since the last call, chains x 2 x 8, and reset
extern "C" int ba_debug_round_stamps(double *out, int64_t n) {
  using namespace boom_amd;
  if (!g_round_stamps) return -1;
  const size_t m = std::min<size_t>((size_t)n, g_round_stamps_n);
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  if (hipMemcpy(out, g_round_stamps, m * 8, hipMemcpyDeviceToHost) != hipSuccess) return -2;
  if (hipMemset(g_round_stamps, 0, g_round_stamps_n * 8) != hipSuccess) return -2;
  return (int)m;
}
#endif
