// Host side of the state-space samplers (bsts): ba_ss_*.  The local-level model on the
// Kalman kernels and the round kernel, the structural models (a list of state models,
// ssm_kernel.hip), the look-ahead of ba_ss_draw_next with its record, the forecast.
#include "engine_internal.h"

namespace boom_amd {

// per chain: K (m T) | state (m T) | smoothed disturbances (nvar T) | normals (<= (nvar + 1) T + m + 1)
static int64_t ssm_work_stride(const ba_engine &e) {
  // (the template kernel keeps four disturbance series and up to five normals a step)
  // (general kernel: a smoothed-disturbance series per state-error row, and as many normals a step + 1)
  const int64_t per_step = std::max(2 * e.ssg.m + 2 * std::max(e.ssg.nvar, e.ssg.nerr) + 1, 2 * e.ssg.m + 9);
  return per_step * e.T + SSG_MAX_STATE + 72;
}

// does the list hold an autoregression with a spike-and-slab prior (ar_spike_kernel.hip)?
static bool ssg_has_ar_spike(const SsgSpec &q) {
  for (int i = 0; i < q.nblocks; ++i)
    if (q.blk[i].ar_spike) return true;
  return false;
}

// does the list hold a random-walk holiday (the general kernel's HD instances, a calendar per block)?
static bool ssg_has_holiday(const SsgSpec &q) {
  for (int i = 0; i < q.nblocks; ++i)
    if (q.blk[i].holiday) return true;
  return false;
}

// does the list hold a calendar seasonal (ssg_is_calendar: the same instances, the same table)?
static bool ssg_has_calendar_seasonal(const SsgSpec &q) {
  for (int i = 0; i < q.nblocks; ++i)
    if (ssg_is_calendar(q.blk[i])) return true;
  return false;
}
// ... a block of either kind: the list has a calendar
static bool ssg_has_calendar(const SsgSpec &q) { return ssg_has_holiday(q) || ssg_has_calendar_seasonal(q); }

// does the block list have the shape the template kernel is compiled for?
// [local level | local linear trend] [seasonal, duration 1] [autoregression], m <= 16
static void ssg_template_shape(const SsgSpec &q, int32_t *trend, int32_t *nseasons, int32_t *ar_lags) {
  *trend = *nseasons = *ar_lags = 0;
  if (q.nblocks < 1 || q.nblocks > 3 || q.m > 16) return;
  if (q.student_block) return;   // (a Student local linear trend: the general kernel's QT instances)
  if (ssg_has_ar_spike(q)) return;   // (a spike-and-slab autoregression: the general kernel passes its sampler by)
  if (ssg_has_calendar(q)) return;   // (a random-walk holiday or a calendar seasonal: the general kernel's HD instances)
  for (int i = 0; i < q.nblocks; ++i)
    if (q.blk[i].nvar == 0) return;   // (a static intercept: the general kernel)
  int b = 0, tr = 0, ns = 0, lags = 0;
  if (q.blk[0].kind == SSG_LOCAL_LEVEL) tr = 1;
  else if (q.blk[0].kind == SSG_LOCAL_LINEAR_TREND) tr = 2;
  else return;
  b = 1;
  if (b < q.nblocks && q.blk[b].kind == SSG_SEASONAL) {
    if (q.blk[b].duration != 1) return;
    ns = q.blk[b].nseasons;
    ++b;
  }
  if (b < q.nblocks && q.blk[b].kind == SSG_AR) {
    lags = q.blk[b].lags;
    ++b;
  }
  if (b != q.nblocks) return;
  *trend = tr;
  *nseasons = ns;
  *ar_lags = lags;
}

// the local-level path of a series of at most LM_TP steps runs lane-major
// (kalman_lm_kernel): its scratch arrays have pitch LM_TP
// the kinds that hold a series and a state (the Gaussian, the Student-t, the Poisson and the logit observation model)
static bool ss_kind(DataKind k) { return k == DATA_STATE_SPACE || k == DATA_SS_STUDENT || k == DATA_SS_POISSON || k == DATA_SS_LOGIT; }

static bool ss_lane_major(const ba_engine &e) { return !e.ssm_set && e.T <= LM_TP; }
static size_t ss_pitch(const ba_engine &e) { return ss_lane_major(e) ? (size_t)LM_TP : (size_t)e.T; }

static void fill_ss_params(ba_engine *e, SsParams &S) {
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
    if (ssg_has_calendar(e->ssg)) {
      S.cal = e->dhol_cal.ptr;   // (packed by hol_prepare, which every entry point that launches passes first)
      S.cal_count = e->hol_cal_count;
    }
  }
}

static const char *const HOLIDAY_FAMILY_REFUSAL =
    "the random-walk holiday is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";
static const char *const HOLIDAY_STUDENT_TREND_REFUSAL =
    "a list that holds both a random-walk holiday and a Student local linear trend is not built";
static const char *const CALSEAS_FAMILY_REFUSAL =
    "the calendar seasonal is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";
static const char *const CALSEAS_STUDENT_TREND_REFUSAL =
    "a list that holds both a calendar seasonal and a Student local linear trend is not built";

// The calendars of the random-walk holidays and the calendar seasonals: every such block needs one
// that covers the series and `extra` steps beyond it (a forecast's horizon); the packed table -- and
// the calendar seasonals' prefix counts -- go to the device when a calendar has changed.  Nothing
// runs on a default calendar.
static int hol_prepare(ba_engine *e, int64_t extra = 0) {
  if (!e->ssm_set || !ssg_has_calendar(e->ssg)) return BA_OK;
  int64_t count = -1;
  for (int b = 0; b < e->ssg.nblocks; ++b) {
    const bool seas = ssg_is_calendar(e->ssg.blk[b]);
    if (!e->ssg.blk[b].holiday && !seas) continue;
    const int64_t n = seas ? (int64_t)e->season_calendar[b].size() : (int64_t)e->hol_calendar[b].size();
    const char *what = seas ? "season" : "holiday";
    char buf[240];
    if (n == 0) {
      if (seas)
        std::snprintf(buf, sizeof buf, "state model %d is a calendar seasonal without a calendar: call ba_ss_set_season_calendar first", b);
      else
        std::snprintf(buf, sizeof buf, "state model %d is a random-walk holiday without a calendar: call ba_ss_set_holiday_calendar first", b);
      return fail(BA_E_STATE, buf);
    }
    if (n < (int64_t)e->T) {
      std::snprintf(buf, sizeof buf, "the %s calendar of state model %d has %lld entries, the series has %d time points",
                    what, b, (long long)n, (int)e->T);
      return fail(BA_E_STATE, buf);
    }
    if (n < (int64_t)e->T + extra) {
      std::snprintf(buf, sizeof buf, "the %s calendar of state model %d has %lld entries: a forecast of horizon %lld needs %lld (the series' %d and the horizon)",
                    what, b, (long long)n, (long long)extra, (long long)((int64_t)e->T + extra), (int)e->T);
      return fail(BA_E_INVALID, buf);
    }
    count = count < 0 ? n : std::min(count, n);
  }
  // (the table's words, then -- a calendar seasonal in the list -- nblocks rows of int32 prefix counts)
  const bool any_seas = ssg_has_calendar_seasonal(e->ssg);
  const size_t nstarted = any_seas ? (size_t)e->ssg.nblocks * (size_t)count : 0;
  const size_t words = (size_t)count + (nstarted + 1) / 2;
  if (e->hol_cal_count == count && e->dhol_cal.count == words) return BA_OK;
  std::vector<uint64_t> packed(words, 0);
  std::fill(packed.begin(), packed.begin() + count, (uint64_t)SSG_CAL_NONE);
  int32_t *started = reinterpret_cast<int32_t *>(packed.data() + count);
  for (int b = 0; b < e->ssg.nblocks; ++b) {
    if (ssg_is_calendar(e->ssg.blk[b])) {
      // (entry 0 is never read: no step leads into time 0)
      int32_t *row = started + (size_t)b * (size_t)count;
      int32_t run = 0;
      for (int64_t t = 1; t < count; ++t) {
        if (e->season_calendar[b][(size_t)t]) {
          packed[(size_t)t] |= (uint64_t)SSG_CAL_SEASON << (8 * b);
          ++run;
        }
        row[t] = run;
      }
      continue;
    }
    if (!e->ssg.blk[b].holiday) continue;
    for (int64_t t = 0; t < count; ++t) {
      const int32_t k = e->hol_calendar[b][(size_t)t];
      if (k >= 0) packed[(size_t)t] = (packed[(size_t)t] & ~(0xffull << (8 * b))) | ((uint64_t)k << (8 * b));
    }
  }
  HIP_TRY(hipStreamSynchronize(e->stream));   // (nothing in flight reads the tables that are replaced)
  HIP_TRY(e->dhol_cal.resize(words));
  HIP_TRY(hipMemcpy(e->dhol_cal.ptr, packed.data(), words * 8, hipMemcpyHostToDevice));
  e->hol_cal_count = count;
  return BA_OK;
}

static const char *const AUTOAR_FAMILY_REFUSAL =
    "the spike-and-slab autoregression is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";

// the list's spike-and-slab autoregressions (false: it has none)
static bool fill_ar_spike_params(ba_engine *e, ArSpikeParams &U) {
  U = ArSpikeParams{};
  if (!e->ssm_set) return false;
  for (int b = 0; b < e->ssg.nblocks; ++b)
    if (e->ssg.blk[b].ar_spike) U.block[U.nspike++] = b;
  U.prior = reinterpret_cast<const ArSpikePrior *>(e->dar_spike_prior.ptr);
  U.gamma = reinterpret_cast<uint8_t *>(e->dar_gamma.ptr);
  return U.nspike > 0;
}

static const char *const SLT_FAMILY_REFUSAL =
    "the Student local linear trend is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";

static void fill_slt_params(ba_engine *e, SltParams &U) {
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
static hipError_t launch_state_kernel(ba_engine *e, const SsParams &S, int draw) {
  ArSpikeParams V;
  if (draw && fill_ar_spike_params(e, V)) {
    // the spike-and-slab autoregressions' samplers, ahead of the state kernel (which draws the
    // other state models' at its head and passes these by)
    hipError_t err = launch_ar_spike(e->stream, S, V);
    if (err != hipSuccess) return err;
  }
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

// ---- look-ahead on the bsts path --------------------------------------------------------
static int ss_sweep_impl(ba_engine *e, int32_t nsweeps, int rec_slot);

// what a round leaves for the callers' loop, copied into the record: one workgroup per
// chain (gamma, beta, sigma^2, the state models' variances and coefficients), then one per
// registered chain (its state path)
struct SsRecParams {
  int32_t C, p, nvar, nphi, nreg, L, row;   // row: slot * L + round
  int64_t var_stride, phi_stride, state_stride, state_doubles;
  const uint8_t *gamma;
  const double *beta, *sigsq, *var, *phi, *state;
  const int32_t *reg;
  uint8_t *rgamma;
  double *rbeta, *rsig, *rvar, *rphi, *rstate;
};
static __global__ __launch_bounds__(256) void ss_record_kernel(SsRecParams R) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int slot = R.row / R.L, i = R.row % R.L;
  if (b < R.C) {
    const size_t at = ((size_t)slot * R.C + b) * R.L + i;
    const size_t p = (size_t)R.p;
    for (size_t j = tid; j < p; j += 256) {
      R.rgamma[at * p + j] = R.gamma[(size_t)b * p + j];
      R.rbeta[at * p + j] = R.beta[(size_t)b * p + j];
    }
    if (tid == 0) R.rsig[at] = R.sigsq[b];
    if (tid < R.nvar) R.rvar[at * R.nvar + tid] = R.var[(size_t)b * R.var_stride + tid];
    if (tid < R.nphi) R.rphi[at * R.nphi + tid] = R.phi[(size_t)b * R.phi_stride + tid];
  } else {
    const int r = b - R.C;
    const size_t c = (size_t)R.reg[r];
    const size_t at = ((size_t)slot * R.nreg + r) * R.L + i;
    const double *src = R.state + c * (size_t)R.state_stride;
    double *dst = R.rstate + at * (size_t)R.state_doubles;
    for (int64_t j = tid; j < R.state_doubles; j += 256) dst[j] = src[j];
  }
}

static bool ss_la_on(const ba_engine *e) { return e->ssla.len > 1; }
// (while the look-ahead itself calls entry points: they do not settle it again)
struct SsLaBusy {
  ba_engine::SsLa &a;
  explicit SsLaBusy(ba_engine::SsLa &la) : a(la) { a.busy = true; }
  ~SsLaBusy() { a.busy = false; }
};
bool ss_la_serving(const ba_engine *e) { return e->ssla.len > 1 && e->ssla.avail > 0 && !e->ssla.busy; }

static hipError_t ss_la_record(ba_engine *e, int slot, int round) {
  ba_engine::SsLa &A = e->ssla;
  SsRecParams R{};
  R.C = e->cfg.chains;
  R.p = e->p;
  R.nvar = (int32_t)A.nvar;
  R.nphi = (int32_t)A.nphi;
  R.nreg = (int32_t)A.reg.size();
  R.L = A.len;
  R.row = slot * A.len + round;
  R.gamma = e->dgamma.ptr;
  R.beta = e->dbeta.ptr;
  R.sigsq = e->dsigsq.ptr;
  if (e->ssm_set) {
    R.var = e->dssm_sigsq.ptr;
    R.var_stride = SSG_MAX_VAR;
    R.phi = e->dar_phi.ptr;
    R.phi_stride = SSG_MAX_AR * AR_MAX;
    R.state = e->dssm_work.ptr + (size_t)e->ssg.m * e->T;
    R.state_stride = ssm_work_stride(*e);
  } else {
    R.var = e->ssla.lev_used.ptr;   // (the live value may be the NEXT round's: drawn ahead)
    R.var_stride = 1;
    R.phi = nullptr;
    R.phi_stride = 0;
    R.state = e->dss_scratch.ptr + (size_t)SS_STATE_ARRAY * ss_pitch(*e);
    R.state_stride = (int64_t)SS_SCRATCH_ARRAYS * (int64_t)ss_pitch(*e);
  }
  R.state_doubles = (int64_t)A.state_doubles;
  R.reg = A.dreg.ptr;
  R.rgamma = A.rgamma.ptr;
  R.rbeta = A.rbeta.ptr;
  R.rsig = A.rsig.ptr;
  R.rvar = A.rvar.ptr;
  R.rphi = A.rphi.ptr;
  R.rstate = A.rstate.ptr;
  hipLaunchKernelGGL(ss_record_kernel, dim3((unsigned)(R.C + R.nreg)), dim3(256), 0, e->stream, R);
  return hipGetLastError();
}

// The state-space half of what a snapshot holds -- THE list: f(live array, elements, words),
// the doubles (into SsLa::snap) in this order, then the stream positions (words: into
// SsLa::snap_pos).  ss_la_alloc sizes the two buffers by a pass over it, ss_la_copy walks
// them by the same pass (a field whose live array is not allocated keeps its place).
//   level (sigsq, n, sumsq) | xty | yty | nobs [| state models: sigsq, n, ss | phi | ar suf]
//   positions: level | state [| state models' | the autoregressions' inclusion indicators]
template <class F>
static int ss_snap_fields(const ba_engine *e, F f) {
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p;
  hipError_t ss_snapshot = hipSuccess;
  auto field = [&](auto *live, size_t n) {
    static_assert(sizeof(*live) == 8, "doubles and 64-bit stream positions");
    if (ss_snapshot == hipSuccess)
      ss_snapshot = f((void *)live, n, std::is_integral<std::remove_pointer_t<decltype(live)>>::value);
  };
  field(e->dlev_sigsq.ptr, C);
  field(e->dlev_n.ptr, C);
  field(e->dlev_sumsq.ptr, C);
  field(e->dxty_c.ptr, C * p);
  field(e->dyty_c.ptr, C);
  field(e->dnobs_c.ptr, C);
  if (e->ssm_set) {
    field(e->dssm_sigsq.ptr, C * SSG_MAX_VAR);
    field(e->dssm_n.ptr, C * SSG_MAX_VAR);
    field(e->dssm_ss.ptr, C * SSG_MAX_VAR);
    field(e->dar_phi.ptr, e->ssg.nar > 0 ? C * SSG_MAX_AR * AR_MAX : 0);
    field(e->dar_suf.ptr, e->ssg.nar > 0 ? C * SSG_MAX_AR * AR_SUF_STRIDE : 0);
  }
  field(e->dpos_level.ptr, C);
  field(e->dpos_state.ptr, C);
  if (e->ssm_set) field(e->dpos_var.ptr, C * SSG_MAX_VAR);
  // (the spike-and-slab autoregressions' inclusion indicators: bytes, held and copied as words)
  if (e->ssm_set) field(e->dar_gamma.ptr, ssg_has_ar_spike(e->ssg) ? C * SSG_MAX_AR * AR_MAX / 8 : 0);
  HIP_TRY(ss_snapshot);
  return BA_OK;
}

// the record's and the snapshots' buffers for the current specification
static int ss_la_alloc(ba_engine *e) {
  ba_engine::SsLa &A = e->ssla;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, L = (size_t)A.len;
  A.nvar = e->ssm_set ? (size_t)e->ssg.nvar : 1;
  A.nphi = e->ssm_set ? (size_t)e->ssg.nar * AR_MAX : 0;
  A.state_doubles = e->ssm_set ? (size_t)e->ssg.m * e->T : ss_pitch(*e);
  {
    // chains whose state path was read since the last allocation join the record while their
    // rows fit in 2 GiB (m = 64, T = 2048, 256 rounds: half a gigabyte per chain); the others
    // keep being read by going back to the draw being served
    const double per_chain = 2.0 * (double)L * (double)A.state_doubles * 8.0;
    for (int32_t w : A.want)
      if (((double)A.reg.size() + 1.0) * per_chain <= 2147483648.0) A.reg.push_back(w);
    A.want.clear();
  }
  const size_t nreg = A.reg.size();
  HIP_TRY(A.rgamma.resize(2 * C * L * p));
  HIP_TRY(A.rbeta.resize(2 * C * L * p));
  HIP_TRY(A.rsig.resize(2 * C * L));
  HIP_TRY(A.rvar.resize(2 * C * L * A.nvar));
  HIP_TRY(A.rphi.resize(2 * C * L * std::max<size_t>(A.nphi, 1)));
  HIP_TRY(A.rstate.resize(2 * nreg * L * A.state_doubles));
  HIP_TRY(A.dreg.resize(nreg));
  HIP_TRY(A.lev_used.resize(C));
  HIP_TRY(hipMemcpy(A.dreg.ptr, A.reg.data(), nreg * 4, hipMemcpyHostToDevice));
  {  // (the round kernel's view of the same list: chain -> its index among the registered)
    std::vector<int32_t> of(C, -1);
    for (size_t r = 0; r < nreg; ++r) of[(size_t)A.reg[r]] = (int32_t)r;
    HIP_TRY(e->dround_reg.resize(C));
    HIP_TRY(hipMemcpy(e->dround_reg.ptr, of.data(), C * 4, hipMemcpyHostToDevice));
  }
  A.snap_doubles = A.snap_words = 0;
  (void)ss_snap_fields(e, [&](void *, size_t n, bool words) {
    (words ? A.snap_words : A.snap_doubles) += n;
    return hipSuccess;
  });
  HIP_TRY(A.snap.resize(2 * A.snap_doubles));
  HIP_TRY(A.snap_pos.resize(2 * A.snap_words));
  for (int i = 0; i < 2; ++i)
    if (!A.done[i]) HIP_TRY(hipEventCreateWithFlags(&A.done[i], hipEventDisableTiming));
  return BA_OK;
}

// snapshot set `set` <-> the live chain state (both halves: the regression's by la_copy)
static int ss_la_copy(ba_engine *e, bool save, int set) {
  ba_engine::SsLa &A = e->ssla;
  int rc = la_copy(e, save, set);
  if (rc) return rc;
  char *held[2] = {(char *)(A.snap.ptr + (size_t)set * A.snap_doubles), (char *)(A.snap_pos.ptr + (size_t)set * A.snap_words)};
  return ss_snap_fields(e, [&](void *live, size_t n, bool words) {
    void *cur = held[words];
    held[words] += n * 8;
    if (!live || !n) return hipSuccess;
    return hipMemcpyAsync(save ? cur : live, save ? live : cur, n * 8, hipMemcpyDeviceToDevice, e->stream);
  });
}

// enqueue one batch into half `slot`: the snapshot of where it starts, then `len` rounds,
// each followed by its record
static int ss_la_launch(ba_engine *e, int slot) {
  ba_engine::SsLa &A = e->ssla;
  SsLaBusy busy(A);
  int rc = ss_la_copy(e, true, slot);
  if (!rc) rc = ss_sweep_impl(e, A.cur, slot);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(A.done[slot], e->stream));
  return BA_OK;
}

static void ss_la_reset(ba_engine *e) {
  ba_engine::SsLa &A = e->ssla;
  A.avail = A.served = 0;
  A.slot = 0;
  A.ahead = false;
  A.synced = false;
  A.cache.clear();
}

// The chains as the caller has seen them: nothing of the look-ahead left in flight.  The
// batch being served is restored to its start and replayed up to the draw handed out
// last (same stream positions, so the same draws).
int ss_la_settle(ba_engine *e) {
  ba_engine::SsLa &A = e->ssla;
  if (A.len <= 1 || A.busy || A.avail == 0) return BA_OK;
  SsLaBusy busy(A);
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->stream2) HIP_TRY(hipStreamSynchronize(e->stream2));
  const int served = A.served, slot = A.slot;
  const bool at_end = served >= A.avail && !A.ahead;   // the chains ARE at the draw served last
  // (With the whole batch handed out and the next one running, the next batch's own snapshot
  // IS the chains at the draw served last -- but not the state PATH of that draw, which a
  // forecast or another chain's state read asks for and only the replay brings back: the
  // batch is replayed then too.)
  ss_la_reset(e);
  if (at_end) return check_chain_status(e);   // (nothing dropped, nothing replayed: free)
  // a rewind and a replay follow (see SsLa::cur: whoever made this necessary may do so after
  // every draw, so the batches get shorter)
  A.clean = false;
  if (A.cur <= 2 && A.cur > 1) A.probe_wait = std::min(1024, A.probe_wait * 2);
  A.cur = std::max(1, A.cur / 2);
  A.calm = 0;
  int rc = ss_la_copy(e, false, slot);
  if (!rc) rc = drop_launched_ahead(e);
  if (rc) return rc;
  if (served > 0) {
    rc = ss_sweep_impl(e, served, -1);
    if (rc) return rc;
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  return check_chain_status(e);
}

// the batch being served is complete and every chain went through it; a batch in which
// a chain stopped (capacity, an error) is run again round by round, with the stops dealt
// with where they happen -- the same draws
int ss_la_wait(ba_engine *e) {
  ba_engine::SsLa &A = e->ssla;
  if (A.synced) return BA_OK;
  HIP_TRY(hipEventSynchronize(A.done[A.slot]));
  bool ok = true;
  int rc = all_chains_ok(e, &ok);
  if (rc) return rc;
  if (!ok) {
    SsLaBusy busy(A);
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->stream2) HIP_TRY(hipStreamSynchronize(e->stream2));
    const int slot = A.slot;
    A.ahead = false;
    rc = ss_la_copy(e, false, slot);
    if (!rc) rc = drop_launched_ahead(e);
    if (rc) return rc;
    rc = ss_la_copy(e, true, slot);   // (the same starting point, for a later settle)
    for (int i = 0; i < A.avail && !rc; ++i) {
      rc = ss_sweep_impl(e, 1, -1);
      if (!rc) HIP_TRY(hipStreamSynchronize(e->stream));
      if (!rc) rc = check_chain_status(e);   // (escalates, catches the chain up, reports errors)
      if (!rc) HIP_TRY(ss_la_record(e, slot, i));
    }
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    A.cache.clear();
  }
  A.synced = true;
  return BA_OK;
}

// one chain's rows of the batch being served, on the host (one set of copies per batch)
int ss_la_rows(ba_engine *e, int64_t c, bool want_state, const ba_engine::SsLa::Rows **out) {
  ba_engine::SsLa &A = e->ssla;
  int rc = ss_la_wait(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, L = (size_t)A.len;
  auto it = A.cache.find(c);
  if (it == A.cache.end()) {
    ba_engine::SsLa::Rows r;
    r.gamma.resize(L * p); r.beta.resize(L * p); r.sig.resize(L); r.var.resize(L * A.nvar); r.phi.resize(L * A.nphi);
    const size_t at = ((size_t)A.slot * C + (size_t)c) * L;
    HIP_TRY(hipMemcpy(r.gamma.data(), A.rgamma.ptr + at * p, L * p, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.beta.data(), A.rbeta.ptr + at * p, L * p * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.sig.data(), A.rsig.ptr + at, L * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.var.data(), A.rvar.ptr + at * A.nvar, L * A.nvar * 8, hipMemcpyDeviceToHost));
    if (A.nphi) HIP_TRY(hipMemcpy(r.phi.data(), A.rphi.ptr + at * A.nphi, L * A.nphi * 8, hipMemcpyDeviceToHost));
    it = A.cache.emplace(c, std::move(r)).first;
  }
  if (want_state && !it->second.has_state) {
    size_t ri = 0;
    while (ri < A.reg.size() && A.reg[ri] != c) ++ri;
    if (ri == A.reg.size()) return fail(BA_E_STATE, "the chain's state path is not in the look-ahead's record");
    it->second.state.resize(L * A.state_doubles);
    const size_t at = ((size_t)A.slot * A.reg.size() + ri) * L;
    HIP_TRY(hipMemcpy(it->second.state.data(), A.rstate.ptr + at * A.state_doubles, L * A.state_doubles * 8,
                      hipMemcpyDeviceToHost));
    it->second.has_state = true;
  }
  *out = &it->second;
  return BA_OK;
}
static bool ss_la_registered(const ba_engine *e, int64_t c) {
  for (int32_t r : e->ssla.reg)
    if (r == c) return true;
  return false;
}
// A chain whose state path was asked for and is not in the record: this read goes back to the
// draw being served (ss_la_settle), the batches from here on record the chain too -- a caller
// that reads chain c after every draw pays for it once, not every time.
// (the list the device buffers are sized by, `reg`, changes in ss_la_alloc only; the state
// record is bounded there)
static void ss_la_want_state(ba_engine *e, int64_t c) {
  ba_engine::SsLa &A = e->ssla;
  if (ss_la_registered(e, c)) return;
  for (int32_t w : A.want)
    if (w == c) return;
  if (A.reg.size() + A.want.size() < 32) A.want.push_back((int32_t)c);
}

}  // namespace boom_amd

extern "C" {

// --------------------------------------------------- state space (kalman)
static int ss_prepare(ba_engine *e, DataKind kind = DATA_STATE_SPACE) {
  int rc = sweep_refusal(e, kind);
  if (rc) return rc;
  if (!e->ss_level_set && !e->ssm_set)
    return fail(BA_E_STATE, "call ba_ss_set_local_level or ba_ss_set_structural first");
  if (kind != DATA_STATE_SPACE && e->ssm_set && e->ssg.student_block) return fail(BA_E_STATE, SLT_FAMILY_REFUSAL);
  if (kind != DATA_STATE_SPACE && e->ssm_set && ssg_has_ar_spike(e->ssg)) return fail(BA_E_STATE, AUTOAR_FAMILY_REFUSAL);
  if (kind != DATA_STATE_SPACE && e->ssm_set && ssg_has_holiday(e->ssg)) return fail(BA_E_STATE, HOLIDAY_FAMILY_REFUSAL);
  if (kind != DATA_STATE_SPACE && e->ssm_set && ssg_has_calendar_seasonal(e->ssg)) return fail(BA_E_STATE, CALSEAS_FAMILY_REFUSAL);
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
    HIP_TRY(hipStreamSynchronize(s));  // (the host vectors above go out of scope)
    e->ss_initialized = false;
  }
  HIP_TRY(e->dmodel.resize(2 * (size_t)e->cfg.chains * ssvs_scalar_layout(64).total));
  return BA_OK;
}

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

}  // extern "C"

namespace boom_amd {
// the scalars of the specification that follow from the block list
static void ssg_finish(SsgSpec &q) {
  // P's leading dimension: odd (a lane per column and a lane per row both conflict-free), and
  // one of the four values ssg_simsmooth_kernel is compiled for
  q.ld = q.m <= 16 ? 17 : (q.m <= 32 ? 33 : (q.m <= 60 ? 61 : 65));
  // state-error rows: one per variance slot, except that a trig block's every component has one
  q.nerr = 0;
  for (int i = 0; i < q.nblocks; ++i) {
    q.blk[i].err0 = q.nerr;
    q.nerr += q.blk[i].kind == SSG_TRIG ? q.blk[i].dim
              : ((q.blk[i].kind == SSG_LOCAL_LINEAR_TREND || q.blk[i].kind == SSG_SEMILOCAL) ? 2 : 1);
  }
  // steps per block of the passes: the most that leaves FOUR workgroups to a CU's 160 KB of
  // LDS (all 1024 chains of a launch resident; at m = 59 sixteen steps left room for three,
  // and the launch ran as two rounds), never below 8; see ssg_pass_lds_doubles
  q.bl = 64;
  while (q.bl > 8 && (2 * q.bl * q.m + q.m * q.ld + q.bl * (q.nerr + 1) + SSG_MAX_STATE + 8 +
                      q.nar * AR_MAX * (AR_MAX + 1)) * 8 > 39 * 1024)
    q.bl /= 2;
}
// ArModel's constructor: "Attempt to initialize ArModel with an illegal value of the
// autoregression coefficients." (the quick bound, then the step-down recursion)
static bool ar_stationary_host(const double *phi, int lags) {
  double a[AR_MAX], b[AR_MAX], sum = 0;
  for (int i = 0; i < lags; ++i) { a[i] = phi[i]; sum += std::fabs(a[i]); }
  if (sum < 1) return true;
  for (int k = lags; k >= 1; --k) {
    const double r = a[k - 1];
    if (!(std::fabs(r) < 1)) return false;
    for (int j = 0; j + 1 < k; ++j) b[j] = (a[j] + r * a[k - 2 - j]) / (1 - r * r);
    for (int j = 0; j + 1 < k; ++j) a[j] = b[j];
  }
  return true;
}
// the Philox sampler id of variance parameter v of the block about to be appended: level 1,
// slope 6, seasonal 7, autoregression 12 for the first block of its family (local level
// and local linear trend are one family), + 16 for every earlier block of the family
static int ssg_stream_id(const SsgSpec &q, int kind, int v) {
  // (a semilocal trend's level variance is of the level family; its NonzeroMeanAr1Sampler a
  // family of its own, id 14)
  if (kind == SSG_SEMILOCAL && v == 1) {
    int occ = 0;
    for (int i = 0; i < q.nblocks; ++i) occ += q.blk[i].kind == SSG_SEMILOCAL;
    return 14 + 16 * occ;
  }
  // (a random-walk holiday's sampler: a family of its own, id 8)
  if (kind == SSG_HOLIDAY) {
    int occ = 0;
    for (int i = 0; i < q.nblocks; ++i) occ += q.blk[i].holiday != 0;
    return 8 + 16 * occ;
  }
  auto family = [](int k) { return (k == SSG_LOCAL_LINEAR_TREND || k == SSG_SEMILOCAL) ? (int)SSG_LOCAL_LEVEL : k; };
  const int fam = family(kind);
  int occ = 0;
  for (int i = 0; i < q.nblocks; ++i) {
    const int k = q.blk[i].kind;
    if (q.blk[i].nvar == 0) continue;   // (a static intercept has no sampler: it is in no family)
    if (q.blk[i].holiday) continue;     // (stored as a local level, but not of the level family)
    if (i == q.student_block - 1) continue;   // (a Student trend's sampler reads SLT_PARAM_STREAM: in no family either)
    if (family(k) == fam) ++occ;
  }
  const int base = kind == SSG_SEASONAL ? 7 : (kind == SSG_AR ? 12 : (kind == SSG_TRIG ? 13 : (v == 0 ? 1 : 6)));
  return base + 16 * occ;
}
// model->add_state(...) on the engine's copy of the specification
static int ssg_add(ba_engine *e, int32_t kind, const int32_t *iparams, const double *var_df,
                   const double *var_sigma_guess, const double *var_sigma_upper_limit,
                   const double *var_initial_sigma, const double *initial_phi,
                   const double *initial_state_mean, const double *initial_state_variance) {
  SsgSpec &q = e->ssg;
  const bool is_static = kind == SSG_STATIC_INTERCEPT;   // (no parameter: the var_* arrays are not read)
  if ((!is_static && (!var_df || !var_sigma_guess || !var_sigma_upper_limit || !var_initial_sigma)) ||
      !initial_state_mean || !initial_state_variance)
    return fail(BA_E_INVALID, "null argument");
  if (q.nblocks >= SSG_MAX_BLOCKS) return fail(BA_E_INVALID, "more than 8 state models");
  const bool is_student = kind == SSG_STUDENT_TREND;
  const bool is_autoar = kind == SSG_AUTO_AR;
  if (is_autoar) kind = SSG_AR;   // (stored as an autoregression with SsgBlock::ar_spike set)
  const bool is_holiday = kind == SSG_HOLIDAY;   // (stored as a local level of dimension width with SsgBlock::holiday set)
  const bool is_calendar = kind == SSG_CALENDAR_SEASONAL;
  if (is_calendar) kind = SSG_SEASONAL;   // (stored as a seasonal with phase SSG_PHASE_CALENDAR: one family, one sampler id)
  SsgBlock k{};
  k.kind = kind;
  k.nvar = 1;
  k.duration = 1;
  k.ar_index = -1;
  switch (kind) {
    case SSG_LOCAL_LEVEL: k.dim = 1; break;
    case SSG_LOCAL_LINEAR_TREND: k.dim = 2; k.nvar = 2; break;
    case SSG_SEASONAL: {
      if (!iparams) return fail(BA_E_INVALID, "null argument");
      // SeasonalStateModelBase: "'nseasons' must be positive"; one season has no state
      if (iparams[0] < 2) return fail(BA_E_INVALID, "nseasons must be at least 2");
      if (is_calendar) {
        // the calendar seasonal: iparams = {nseasons}; its season starts come through
        // ba_ss_set_season_calendar (duration and phase stay 1 and 0 and are not read for it)
        if (e->data_kind == DATA_SS_STUDENT || e->data_kind == DATA_SS_POISSON || e->data_kind == DATA_SS_LOGIT)
          return fail(BA_E_STATE, CALSEAS_FAMILY_REFUSAL);
        if (q.student_block) return fail(BA_E_STATE, CALSEAS_STUDENT_TREND_REFUSAL);
        k.nseasons = iparams[0];
        k.dim = k.nseasons - 1;
        k.phase = SSG_PHASE_CALENDAR;
        break;
      }
      if (iparams[1] < 1) return fail(BA_E_INVALID, "season_duration must be positive");
      // (the kernels keep a block's duration and its running phase in 16-bit fields)
      if (iparams[1] > 65535) return fail(BA_E_INVALID, "season_duration exceeds 65535");
      k.nseasons = iparams[0];
      k.duration = iparams[1];
      // new_season(t): (t - time_of_first_observation) is a multiple of the duration
      k.phase = ((iparams[2] % k.duration) + k.duration) % k.duration;
      k.dim = k.nseasons - 1;
      break;
    }
    case SSG_HOLIDAY:
      // RandomWalkHolidayStateModel: iparams = {width}, the holiday's maximum window width; its
      // calendar comes through ba_ss_set_holiday_calendar
      if (!iparams) return fail(BA_E_INVALID, "null argument");
      if (iparams[0] < 1 || iparams[0] > SSG_MAX_STATE - 1)
        return fail(BA_E_INVALID, "a random-walk holiday's width must lie in [1, 63]");
      if (e->data_kind == DATA_SS_STUDENT || e->data_kind == DATA_SS_POISSON || e->data_kind == DATA_SS_LOGIT)
        return fail(BA_E_STATE, HOLIDAY_FAMILY_REFUSAL);
      if (q.student_block) return fail(BA_E_STATE, HOLIDAY_STUDENT_TREND_REFUSAL);
      k.kind = SSG_LOCAL_LEVEL;
      k.dim = iparams[0];
      k.holiday = 1;
      break;
    case SSG_STATIC_INTERCEPT:
      // StaticInterceptStateModel: T = 1, RQR = 0, nothing to learn and no sampler -- a local
      // level whose variance (a slot of its own, never drawn) is 0
      k.kind = SSG_LOCAL_LEVEL;
      k.dim = 1;
      k.nvar = 0;
      break;
    case SSG_TRIG:
      // TrigStateModel: "At least one frequency needed ..."; the rotations as the transition
      // matrix holds them: (cos, sin) per frequency in initial_phi
      if (!iparams || !initial_phi) return fail(BA_E_INVALID, "null argument");
      if (iparams[0] < 1) return fail(BA_E_INVALID, "At least one frequency needed to initialize TrigStateModel.");
      if (2 * iparams[0] > SSG_MAX_STATE) return fail(BA_E_INVALID, "state dimension exceeds 64");
      k.nfreq = iparams[0];
      k.dim = 2 * k.nfreq;
      break;
    case SSG_SEMILOCAL:
      // SemilocalLinearTrendStateModel(level, slope): iparams = {force_stationary,
      // force_ar1_positive}; initial_phi = {slope mean prior mu, sigma, AR(1) coefficient prior mu,
      // sigma, initial mu, initial phi}
      if (!iparams || !initial_phi) return fail(BA_E_INVALID, "null argument");
      if (iparams[1] && !iparams[0])
        return fail(BA_E_INVALID, "force_ar1_positive without force_stationary (a one-sided truncation of the slope's "
                                  "AR(1) coefficient) is not built");
      if (!(initial_phi[1] > 0) || !(initial_phi[3] > 0)) return fail(BA_E_INVALID, "the slope's prior standard deviations must be positive");
      if (q.nar >= SSG_MAX_AR) return fail(BA_E_INVALID, "more than 4 autoregression / semilocal state models");
      k.dim = 3;
      k.nvar = 2;
      k.ar_index = q.nar;
      k.sl_truncate = iparams[0] != 0;
      k.sl_positive = iparams[1] != 0;
      break;
    case SSG_STUDENT_TREND: {
      // StudentLocalLinearTrendStateModel(sigma_level, nu_level, sigma_slope, nu_slope): initial_phi =
      // {nu_level prior kind, a, b, nu_slope prior kind, a, b, initial nu_level, initial nu_slope}; on
      // the device a local linear trend block (SsgSpec::student_block names it) with weights
      if (!initial_phi) return fail(BA_E_INVALID, "null argument");
      if (q.student_block) return fail(BA_E_INVALID, "at most one Student local linear trend per list of state models");
      if (ssg_has_holiday(q)) return fail(BA_E_STATE, HOLIDAY_STUDENT_TREND_REFUSAL);
      if (ssg_has_calendar_seasonal(q)) return fail(BA_E_STATE, CALSEAS_STUDENT_TREND_REFUSAL);
      if (e->data_kind == DATA_SS_STUDENT || e->data_kind == DATA_SS_POISSON || e->data_kind == DATA_SS_LOGIT)
        return fail(BA_E_STATE, SLT_FAMILY_REFUSAL);
      for (int c = 0; c < 2; ++c) {
        const double pk = initial_phi[3 * c], a = initial_phi[3 * c + 1], b = initial_phi[3 * c + 2], nu = initial_phi[6 + c];
        if (pk != STUDENT_NU_UNIFORM && pk != STUDENT_NU_GAMMA) return fail(BA_E_INVALID, "nu prior kind must be 0 (uniform) or 1 (gamma)");
        if (pk == STUDENT_NU_UNIFORM ? !(a < b) || !std::isfinite(a) || !std::isfinite(b) : !(a > 0) || !(b > 0))
          return fail(BA_E_INVALID, "nu prior: uniform needs a < b, gamma needs positive shape and rate");
        const bool ok = std::isfinite(nu) && nu > 0 && (pk != STUDENT_NU_UNIFORM || (nu >= a && nu <= b));
        if (!ok) return fail(BA_E_INVALID, "the initial nu must be positive and have positive prior density");
      }
      k.kind = SSG_LOCAL_LINEAR_TREND;
      k.dim = 2;
      k.nvar = 2;
      break;
    }
    case SSG_AR:
      if (!iparams) return fail(BA_E_INVALID, "null argument");
      if (iparams[0] < 1) return fail(BA_E_INVALID, "lags must be positive");
      if (iparams[0] > AR_MAX) return fail(BA_E_INVALID, "more than 16 lags");
      if (q.nar >= SSG_MAX_AR) return fail(BA_E_INVALID, "more than 4 autoregression state models");
      k.lags = iparams[0];
      k.dim = k.lags;
      k.ar_index = q.nar;
      if (is_autoar) {
        // ArStateModel + ArSpikeSlabSampler: iparams = {lags, truncate, max_flips, allow_model_selection};
        // initial_phi = {coefficients, slab mean, inclusion probabilities (lags each), slab precision (lags x lags)}
        if (!initial_phi) return fail(BA_E_INVALID, "null argument");
        if (e->data_kind == DATA_SS_STUDENT || e->data_kind == DATA_SS_POISSON || e->data_kind == DATA_SS_LOGIT)
          return fail(BA_E_STATE, AUTOAR_FAMILY_REFUSAL);
        const int L = k.lags;
        const double *mu = initial_phi + L, *pi = initial_phi + 2 * L, *om = initial_phi + 3 * L;
        ArSpikePrior R{};
        for (int i = 0; i < L; ++i) {
          if (!std::isfinite(mu[i])) return fail(BA_E_INVALID, "the slab's mean must be finite");
          if (!(pi[i] >= 0.0 && pi[i] <= 1.0)) return fail(BA_E_INVALID, "prior inclusion probabilities must lie in [0, 1]");
          R.mu[i] = mu[i];
          R.pi[i] = pi[i];
          R.log_pi[i] = std::log(pi[i]);
          R.log_1mpi[i] = std::log(1 - pi[i]);
        }
        double ch[AR_MAX][AR_MAX] = {};
        for (int i = 0; i < L; ++i)
          for (int j = 0; j < L; ++j) {
            const double a = om[(size_t)j * L + i], b = om[(size_t)i * L + j];
            if (!std::isfinite(a) || !(std::fabs(a - b) <= 1e-12 * (std::fabs(a) + std::fabs(b))))
              return fail(BA_E_INVALID, "the slab's precision must be symmetric positive definite");
            R.siginv[i * AR_MAX + j] = a;
          }
        for (int j = 0; j < L; ++j) {
          for (int i = j; i < L; ++i) {
            double sacc = R.siginv[i * AR_MAX + j];
            for (int t = 0; t < j; ++t) sacc -= ch[i][t] * ch[j][t];
            if (i == j) {
              if (!(sacc > 0.0)) return fail(BA_E_INVALID, "the slab's precision must be symmetric positive definite");
              ch[j][j] = std::sqrt(sacc);
            } else {
              ch[i][j] = sacc / ch[j][j];
            }
          }
        }
        R.truncate = iparams[1] != 0;
        R.max_flips = iparams[2];
        R.select = iparams[3] != 0;
        if (R.truncate && !ar_stationary_host(initial_phi, L))
          return fail(BA_E_INVALID, "the initial autoregression coefficients are not stationary");
        e->ar_spike_prior[k.ar_index] = R;
        k.ar_spike = 1;
      }
      break;
    default:
      return fail(BA_E_INVALID, "state model kind must be 1 (local level), 2 (local linear trend), 3 (seasonal), 4 (autoregression), 5 (static intercept), 6 (trig), 7 (semilocal linear trend), 8 (Student local linear trend), 9 (spike-and-slab autoregression), 10 (random-walk holiday) or 11 (calendar seasonal)");
  }
  const int nslot = is_static ? 1 : k.nvar;   // variance slots the block takes
  if (q.m + k.dim > SSG_MAX_STATE) return fail(BA_E_INVALID, "state dimension exceeds 64");
  if (q.nvar + nslot > SSG_MAX_VAR) return fail(BA_E_INVALID, "more than 16 variance parameters");
  for (int v = 0; v < k.nvar; ++v) {
    if (var_sigma_upper_limit[v] < 0) return fail(BA_E_INVALID, "sigma_max must be non-negative.");
    if ((kind == SSG_AR || kind == SSG_SEMILOCAL || is_student) && !(var_initial_sigma[v] > 0))
      return fail(BA_E_INVALID, "initial sigma must be positive");
  }
  for (int i = 0; i < k.dim; ++i) {
    // (a multivariate initial state goes through a Cholesky factor in the reference: it
    // needs a positive variance; the local level model alone does not)
    const bool ok = initial_state_variance[i] > 0.0 ||
                    ((kind == SSG_LOCAL_LEVEL || is_static) && !is_holiday && initial_state_variance[i] == 0.0) ||
                    (kind == SSG_SEMILOCAL && i == 2);   // (the slope's long-run mean: a parameter, variance 0 whatever is passed)
    if (!ok) return fail(BA_E_INVALID, "initial state variances must be positive");
  }
  if (kind == SSG_AR && !is_autoar && initial_phi && !ar_stationary_host(initial_phi, k.lags))
    return fail(BA_E_INVALID, "the initial autoregression coefficients are not stationary");
  k.first = q.m;
  k.var0 = q.nvar;
  for (int v = 0; v < k.nvar; ++v) {
    const int vi = k.var0 + v;
    // ChisqModel(df, sigma_guess): 2 alpha = df, 2 beta = df sigma^2
    q.prior_df[vi] = 2 * (var_df[v] / 2.0);
    q.prior_ss[vi] = 2 * (var_df[v] * var_sigma_guess[v] * var_sigma_guess[v] / 2.0);
    q.sigma_max[vi] = var_sigma_upper_limit[v];
    e->ssg_initial_sigsq[vi] = var_initial_sigma[v] * var_initial_sigma[v];
    k.sid[v] = is_student ? (int)SLT_PARAM_STREAM : ssg_stream_id(q, kind, v);
  }
  if (is_static) {
    // (the slot: variance 0, a sampler that is never run)
    q.prior_df[k.var0] = 0.0;
    q.prior_ss[k.var0] = 0.0;
    q.sigma_max[k.var0] = std::numeric_limits<double>::infinity();
    e->ssg_initial_sigsq[k.var0] = 0.0;
  }
  for (int i = 0; i < k.dim; ++i) {
    q.a0[k.first + i] = initial_state_mean[i];
    q.P0[k.first + i] = initial_state_variance[i];
    q.trig_c[k.first + i] = kind == SSG_TRIG ? initial_phi[2 * (i / 2)] : 0.0;
    q.trig_s[k.first + i] = kind == SSG_TRIG ? initial_phi[2 * (i / 2) + 1] : 0.0;
  }
  if (kind == SSG_AR) {
    for (int i = 0; i < AR_MAX; ++i)
      e->ssg_initial_phi[k.ar_index][i] = (initial_phi && i < k.lags) ? initial_phi[i] : 0.0;
    q.nar += 1;
  }
  if (kind == SSG_SEMILOCAL) {
    for (int i = 0; i < AR_MAX; ++i) e->ssg_initial_phi[k.ar_index][i] = 0.0;
    e->ssg_initial_phi[k.ar_index][0] = initial_phi[5];   // phi
    e->ssg_initial_phi[k.ar_index][1] = initial_phi[4];   // mu
    for (int i = 0; i < 4; ++i) q.sl_prior[k.ar_index][i] = initial_phi[i];
    // initial_state_mean()[2] = slope->mu() (per chain, per draw: the kernel's), variance 0
    q.a0[k.first + 2] = initial_phi[4];
    q.P0[k.first + 2] = 0.0;
    q.nar += 1;
  }
  if (is_holiday) e->hol_calendar[q.nblocks].clear();   // (no calendar yet)
  if (is_calendar) e->season_calendar[q.nblocks].clear();
  if (is_student) {
    q.student_block = q.nblocks + 1;
    for (int c = 0; c < 2; ++c) {
      e->slt_nu_kind[c] = (int)initial_phi[3 * c];
      e->slt_nu_a[c] = initial_phi[3 * c + 1];
      e->slt_nu_b[c] = initial_phi[3 * c + 2];
      e->slt_initial_nu[c] = initial_phi[6 + c];
    }
  }
  q.blk[q.nblocks] = k;
  q.nblocks += 1;
  q.m += k.dim;
  q.nvar += nslot;
  ssg_finish(q);
  e->ssm_set = true;
  e->ss_level_set = false;
  e->dss_scratch.release();
  return BA_OK;
}
static void ssg_clear(ba_engine *e) {
  e->ssg = SsgSpec{};
  for (int b = 0; b < SSG_MAX_BLOCKS; ++b) { e->hol_calendar[b].clear(); e->season_calendar[b].clear(); }
  e->hol_cal_count = 0;
  for (int i = 0; i < 3; ++i) e->ssg_template_var[i] = -1;
  e->ssg_template_ar = -1;
  e->ssm_set = false;
  e->dss_scratch.release();
}
}  // namespace boom_amd

extern "C" {

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

int ba_ss_clear_state_models(ba_engine *e) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  ssg_clear(e);
  return BA_OK;
}

int ba_ss_add_state_model(ba_engine *e, int32_t kind, const int32_t *iparams, const double *var_df,
                          const double *var_sigma_guess, const double *var_sigma_upper_limit,
                          const double *var_initial_sigma, const double *initial_phi,
                          const double *initial_state_mean, const double *initial_state_variance) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (e->ss_level_set) ssg_clear(e);   // (a local-level specification is replaced, not extended)
  e->ss_level_set = false;
  return ssg_add(e, kind, iparams, var_df, var_sigma_guess, var_sigma_upper_limit, var_initial_sigma,
                 initial_phi, initial_state_mean, initial_state_variance);
}

int ba_ss_state_dimension(ba_engine *e, int32_t *state_dimension, int32_t *nblocks) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (state_dimension) *state_dimension = e->ssm_set ? e->ssg.m : (e->ss_level_set ? 1 : 0);
  if (nblocks) *nblocks = e->ssm_set ? e->ssg.nblocks : (e->ss_level_set ? 1 : 0);
  return BA_OK;
}

// a random-walk holiday's calendar: entry t is -1 (time t is not in the holiday's window) or the
// position of time t in the window, in [0, width)
int ba_ss_set_holiday_calendar(ba_engine *e, int32_t block, const int32_t *position, int64_t count) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!position || count <= 0) return fail(BA_E_INVALID, "bad argument");
  if (!e->ssm_set || block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  const SsgBlock &k = e->ssg.blk[block];
  if (ssg_is_calendar(k)) return fail(BA_E_INVALID, "not a random-walk holiday state model: a calendar seasonal's calendar goes through ba_ss_set_season_calendar");
  if (!k.holiday) return fail(BA_E_INVALID, "not a random-walk holiday state model");
  for (int64_t t = 0; t < count; ++t)
    if (position[t] < -1 || position[t] >= k.dim) {
      char buf[160];
      std::snprintf(buf, sizeof buf, "holiday calendar entry %lld is %d: it must be -1 (inactive) or a position in [0, %d)",
                    (long long)t, (int)position[t], (int)k.dim);
      return fail(BA_E_INVALID, buf);
    }
  e->hol_calendar[block].assign(position, position + count);
  e->hol_cal_count = 0;   // (packed again by the next call that launches)
  return BA_OK;
}

// position == nullptr: the count alone
int ba_ss_get_holiday_calendar(ba_engine *e, int32_t block, int32_t *position, int64_t *count) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!e->ssm_set || block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  if (!e->ssg.blk[block].holiday) return fail(BA_E_INVALID, "not a random-walk holiday state model");
  const std::vector<int32_t> &c = e->hol_calendar[block];
  if (count) *count = (int64_t)c.size();
  if (position && !c.empty()) std::memcpy(position, c.data(), c.size() * sizeof(int32_t));
  return BA_OK;
}

// a calendar seasonal's calendar: entry t is 1 where time t starts a new season, else 0 (entry 0 is
// never read: no step leads into time 0)
int ba_ss_set_season_calendar(ba_engine *e, int32_t block, const uint8_t *new_season, int64_t count) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!new_season || count <= 0) return fail(BA_E_INVALID, "bad argument");
  if (!e->ssm_set || block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  if (!ssg_is_calendar(e->ssg.blk[block])) return fail(BA_E_INVALID, "not a calendar seasonal state model");
  for (int64_t t = 0; t < count; ++t)
    if (new_season[t] > 1) {
      char buf[160];
      std::snprintf(buf, sizeof buf, "season calendar entry %lld is %d: it must be 0 or 1 (time t starts a new season)",
                    (long long)t, (int)new_season[t]);
      return fail(BA_E_INVALID, buf);
    }
  e->season_calendar[block].assign(new_season, new_season + count);
  e->hol_cal_count = 0;   // (packed again by the next call that launches)
  return BA_OK;
}

// new_season == nullptr: the count alone
int ba_ss_get_season_calendar(ba_engine *e, int32_t block, uint8_t *new_season, int64_t *count) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!e->ssm_set || block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  if (!ssg_is_calendar(e->ssg.blk[block])) return fail(BA_E_INVALID, "not a calendar seasonal state model");
  const std::vector<uint8_t> &c = e->season_calendar[block];
  if (count) *count = (int64_t)c.size();
  if (new_season && !c.empty()) std::memcpy(new_season, c.data(), c.size());
  return BA_OK;
}

// MonthlyAnnualCycle's calendar from the date of the first observation (proleptic Gregorian): out[t] = 1
// where the day `t` days after (year, month, day) is the first of a month
int ba_monthly_cycle_calendar(int32_t year, int32_t month, int32_t day, int64_t count, uint8_t *out) {
  if (!out || count < 0) return fail(BA_E_INVALID, "bad argument");
  auto leap = [](int64_t y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; };
  auto days_in = [&](int64_t y, int mo) {
    static const int len[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    return len[mo - 1] + ((mo == 2 && leap(y)) ? 1 : 0);
  };
  if (month < 1 || month > 12 || day < 1 || day > days_in(year, month)) return fail(BA_E_INVALID, "not a date of the Gregorian calendar");
  int64_t y = year;
  int mo = month, d = day;
  for (int64_t t = 0; t < count; ++t) {
    out[t] = d == 1 ? 1 : 0;
    if (++d > days_in(y, mo)) {
      d = 1;
      if (++mo > 12) { mo = 1; ++y; }
    }
  }
  return BA_OK;
}

int ba_ss_set_structural(ba_engine *e, int32_t trend, int32_t nseasons, const double *var_df,
                         const double *var_sigma_guess, const double *var_sigma_upper_limit,
                         const double *var_initial_sigma, const double *initial_state_mean,
                         const double *initial_state_variance) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (!var_df || !var_sigma_guess || !var_sigma_upper_limit || !var_initial_sigma ||
      !initial_state_mean || !initial_state_variance)
    return fail(BA_E_INVALID, "null argument");
  if (trend != 1 && trend != 2) return fail(BA_E_INVALID, "trend must be 1 (local level) or 2 (local linear trend)");
  if (nseasons != 0 && nseasons < 2) return fail(BA_E_INVALID, "nseasons must be 0 or at least 2");
  const int m = trend + (nseasons > 0 ? nseasons - 1 : 0);
  if (m > SSG_MAX_STATE) return fail(BA_E_INVALID, "state dimension exceeds 64");
  for (int i = 0; i < 3; ++i) {
    const bool used = i == 0 || (i == 1 && trend == 2) || (i == 2 && nseasons > 0);
    if (used && var_sigma_upper_limit[i] < 0) return fail(BA_E_INVALID, "sigma_max must be non-negative.");
  }
  ssg_clear(e);
  int rc = ssg_add(e, trend == 2 ? SSG_LOCAL_LINEAR_TREND : SSG_LOCAL_LEVEL, nullptr, var_df, var_sigma_guess,
                   var_sigma_upper_limit, var_initial_sigma, nullptr, initial_state_mean, initial_state_variance);
  if (!rc && nseasons > 0) {
    const int32_t ip[3] = {nseasons, 1, 0};
    rc = ssg_add(e, SSG_SEASONAL, ip, var_df + 2, var_sigma_guess + 2, var_sigma_upper_limit + 2,
                 var_initial_sigma + 2, nullptr, initial_state_mean + trend, initial_state_variance + trend);
  }
  if (rc) {
    ssg_clear(e);
    return rc;
  }
  e->ssg_template_var[0] = 0;
  e->ssg_template_var[1] = trend == 2 ? 1 : -1;
  e->ssg_template_var[2] = nseasons > 0 ? trend : -1;
  return BA_OK;
}

int ba_ss_add_ar(ba_engine *e, int32_t lags, double prior_df, double sigma_guess,
                 double sigma_upper_limit, double initial_sigma, const double *initial_phi,
                 const double *initial_state_mean, const double *initial_state_variance) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (!e->ssm_set) return fail(BA_E_STATE, "call ba_ss_set_structural first");
  if (e->ssg_template_ar >= 0) return fail(BA_E_STATE, "the state already has an autoregression block");
  if (!initial_state_mean || !initial_state_variance) return fail(BA_E_INVALID, "null argument");
  if (lags < 1) return fail(BA_E_INVALID, "lags must be positive");
  const int32_t ip[3] = {lags, 0, 0};
  const int rc = ssg_add(e, SSG_AR, ip, &prior_df, &sigma_guess, &sigma_upper_limit, &initial_sigma, initial_phi,
                         initial_state_mean, initial_state_variance);
  if (rc) return rc;
  e->ssg_template_ar = e->ssg.nblocks - 1;
  return BA_OK;
}

// block `block` of one chain: its variance parameters, the state model's sufficient
// statistics of the last sweep, and for an autoregression block its coefficients and ArModel
// sufficient statistics
int ba_ss_get_state_model(ba_engine *e, int64_t chain, int32_t block, double *variances, double *suf_n,
                          double *suf_ss, double *phi, double *ar_xtx, double *ar_xty, double *ar_yty,
                          double *ar_n) {
  ENGINE_ACCESSOR_SERVED(e);
  if (!ss_kind(e->data_kind) || !e->ssm_set || e->dssm_work.count == 0)
    return fail(BA_E_STATE, "no structural state-space run yet");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  if (block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  const SsgBlock &k = e->ssg.blk[block];
  const bool is_sl = k.kind == SSG_SEMILOCAL;
  const bool is_ar = k.kind == SSG_AR || is_sl;   // (both keep coefficients and statistics in an autoregression slot)
  const bool is_student = block == e->ssg.student_block - 1;   // (phi: nu_level, nu_slope)
  if (!is_ar && ((phi && !is_student) || ar_xtx || ar_xty || ar_yty || ar_n))
    return fail(BA_E_INVALID, "not an autoregression state model");
  if (is_sl && (ar_xty || ar_yty))
    return fail(BA_E_INVALID, "a semilocal linear trend's Ar1Suf comes back through ar_xtx (six doubles) and ar_n");
  if (ss_la_serving(e)) {
    if (!suf_n && !suf_ss && !ar_xtx && !ar_xty && !ar_yty && !ar_n) {
      // the draw ba_ss_draw_next is serving, from the record
      const ba_engine::SsLa::Rows *r = nullptr;
      int rcr = ss_la_rows(e, chain, false, &r);
      if (rcr) return rcr;
      const size_t row = (size_t)e->ssla.served - 1;
      if (variances)
        for (int v = 0; v < k.nvar; ++v) variances[v] = r->var[row * e->ssla.nvar + k.var0 + v];
      if (phi)
        for (int i = 0; i < (is_sl ? 2 : k.lags); ++i) phi[i] = r->phi[row * e->ssla.nphi + (size_t)k.ar_index * AR_MAX + i];
      return BA_OK;
    }
    int rcs = ss_la_settle(e);   // (sufficient statistics are not in the record)
    if (rcs) return rcs;
  }
  int rc = ba_sync(e);
  if (rc) return rc;
  HIP_TRY(pinned_reserve(e, (6 + AR_MAX + AR_SUF_STRIDE) * 8));
  double *hv = (double *)e->pinned, *hphi = hv + 6, *hsuf = hphi + AR_MAX;
  const size_t at = (size_t)chain * SSG_MAX_VAR + k.var0;
  HIP_TRY(hipMemcpyAsync(hv, e->dssm_sigsq.ptr + at, (size_t)k.nvar * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(hv + 2, e->dssm_n.ptr + at, (size_t)k.nvar * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(hv + 4, e->dssm_ss.ptr + at, (size_t)k.nvar * 8, hipMemcpyDeviceToHost, e->stream));
  if (is_ar) {
    const size_t slot = (size_t)chain * SSG_MAX_AR + k.ar_index;
    HIP_TRY(hipMemcpyAsync(hphi, e->dar_phi.ptr + slot * AR_MAX, AR_MAX * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(hsuf, e->dar_suf.ptr + slot * AR_SUF_STRIDE, AR_SUF_STRIDE * 8, hipMemcpyDeviceToHost,
                           e->stream));
  }
  if (is_student && phi)
    HIP_TRY(hipMemcpyAsync(hphi, e->dslt_nu.ptr + (size_t)chain * 2, 2 * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (is_student && phi) { phi[0] = hphi[0]; phi[1] = hphi[1]; }
  for (int v = 0; v < k.nvar; ++v) {
    if (variances) variances[v] = hv[v];
    if (suf_n) suf_n[v] = hv[2 + v];
    if (suf_ss) suf_ss[v] = hv[4 + v];
  }
  if (k.kind == SSG_SEMILOCAL) {
    // (phi, mu) of the slope's NonzeroMeanAr1Model; its Ar1Suf -- sumsq, sum, cross, n, first,
    // last value -- through ar_xtx (six doubles)
    if (phi) { phi[0] = hphi[0]; phi[1] = hphi[1]; }
    if (ar_xtx) std::memcpy(ar_xtx, hsuf, 6 * 8);
    if (ar_n) *ar_n = hsuf[3];
  } else if (is_ar) {
    const int L = k.lags;
    if (phi) std::memcpy(phi, hphi, (size_t)L * 8);
    if (ar_xtx)
      for (int i = 0; i < L; ++i)
        for (int j = 0; j < L; ++j) ar_xtx[(size_t)j * L + i] = hsuf[(size_t)i * AR_MAX + j];
    if (ar_xty) std::memcpy(ar_xty, hsuf + AR_SUF_XTY, (size_t)L * 8);
    if (ar_yty) *ar_yty = hsuf[AR_SUF_YTY];
    if (ar_n) *ar_n = hsuf[AR_SUF_N];
  }
  return BA_OK;
}

int ba_ss_get_ar(ba_engine *e, int64_t chain, double *phi, double *sigsq, double *suf_xtx,
                 double *suf_xty, double *suf_yty, double *suf_n) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!ss_kind(e->data_kind) || !e->ssm_set || e->ssg_template_ar < 0 || e->dar_phi.count == 0)
    return fail(BA_E_STATE, "no structural run with an autoregression block yet");
  return ba_ss_get_state_model(e, chain, e->ssg_template_ar, sigsq, nullptr, nullptr, phi, suf_xtx, suf_xty,
                               suf_yty, suf_n);
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

// ---- the Student local linear trend's own state (slt_kernel.hip)
static int slt_ready(ba_engine *e) {
  if (e->data_kind != DATA_STATE_SPACE) return fail(BA_E_STATE, set_data_first(DATA_STATE_SPACE));
  if (!e->ssm_set || !e->ssg.student_block)
    return fail(BA_E_STATE, "the list of state models holds no Student local linear trend");
  return ss_prepare(e);
}

int ba_ss_trend_get_weights(ba_engine *e, int64_t chain, double *level_w, double *slope_w) {
  ENGINE_PROLOGUE(e);
  if (!level_w || !slope_w) return fail(BA_E_INVALID, "null argument");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = slt_ready(e);
  if (rc) return rc;
  const size_t T = (size_t)e->T;
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(level_w, e->dslt_w.ptr + (size_t)chain * 2 * T, T * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(slope_w, e->dslt_w.ptr + (size_t)chain * 2 * T + T, T * 8, hipMemcpyDeviceToHost));
  return BA_OK;
}

int ba_ss_trend_set_weights(ba_engine *e, int64_t chain, const double *level_w, const double *slope_w) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!level_w || !slope_w) return fail(BA_E_INVALID, "null argument");
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = slt_ready(e);
  if (rc) return rc;
  const size_t T = (size_t)e->T, C = (size_t)e->cfg.chains;
  for (size_t t = 0; t < T; ++t)
    if (!(level_w[t] > 0.0) || !std::isfinite(level_w[t]) || !(slope_w[t] > 0.0) || !std::isfinite(slope_w[t]))
      return fail(BA_E_INVALID, "Weights must be finite and positive.");
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t c = chain < 0 ? 0 : (size_t)chain; c < (chain < 0 ? C : (size_t)chain + 1); ++c) {
    HIP_TRY(hipMemcpy(e->dslt_w.ptr + c * 2 * T, level_w, T * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->dslt_w.ptr + c * 2 * T + T, slope_w, T * 8, hipMemcpyHostToDevice));
  }
  return BA_OK;
}

// the GammaSuf of the weights the last observe_state drew: (n, sum, sum of logs) of the level, then of the slope
int ba_ss_trend_get_weight_suf(ba_engine *e, int64_t chain, double *out) {
  ENGINE_PROLOGUE(e);
  if (!out) return fail(BA_E_INVALID, "null argument");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = slt_ready(e);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, e->dslt_wsuf.ptr + (size_t)chain * 6, 6 * 8, hipMemcpyDeviceToHost));
  return BA_OK;
}

// the ArSpikeSlabSampler::draw() of every spike-and-slab autoregression alone
int ba_ss_autoar_draw_parameters(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  e->table_ok = false;
  if (e->data_kind != DATA_STATE_SPACE) return fail(BA_E_STATE, set_data_first(DATA_STATE_SPACE));
  ArSpikeParams V;
  if (!fill_ar_spike_params(e, V)) return fail(BA_E_STATE, "the list of state models holds no spike-and-slab autoregression");
  int rc = ss_prepare(e);
  if (rc) return rc;
  SsParams S;
  fill_ss_params(e, S);
  fill_ar_spike_params(e, V);
  HIP_TRY(launch_ar_spike(e->stream, S, V));
  return BA_OK;
}

int ba_ss_get_ar_inclusion(ba_engine *e, int64_t chain, int32_t block, uint8_t *gamma) {
  ENGINE_PROLOGUE(e);   // (under a look-ahead: the chains back at the draw being served)
  if (!gamma) return fail(BA_E_INVALID, "null argument");
  if (!ss_kind(e->data_kind) || !e->ssm_set || e->dssm_work.count == 0)
    return fail(BA_E_STATE, "no structural state-space run yet");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  if (block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  const SsgBlock &k = e->ssg.blk[block];
  if (!k.ar_spike || e->dar_gamma.count == 0) return fail(BA_E_INVALID, "not a spike-and-slab autoregression state model");
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(gamma, reinterpret_cast<const uint8_t *>(e->dar_gamma.ptr) + ((size_t)chain * SSG_MAX_AR + k.ar_index) * AR_MAX,
                    (size_t)k.lags, hipMemcpyDeviceToHost));
  return BA_OK;
}

// the block's sample_posterior() alone: sigma_level^2, nu_level, sigma_slope^2, nu_slope
int ba_ss_trend_draw_parameters(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  e->table_ok = false;
  int rc = slt_ready(e);
  if (rc) return rc;
  SsParams S;
  fill_ss_params(e, S);
  SltParams U;
  fill_slt_params(e, U);
  HIP_TRY(launch_slt_params(e->stream, S, U));
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
static int ss_sweep_impl(ba_engine *e, int32_t nsweeps, int rec_slot) {
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

// The callers' loop on the bsts path -- for (i in niter) { model.sample_posterior(); record }
// (Interfaces/R/bsts/src/bsts.cc:82-119) -- at the device's rate: rounds are enqueued
// `lookahead` at a time, every round's draw recorded on the device, and ba_ss_draw_next
// hands them out one per call; the accessors below see the draw being served.
int ba_ss_set_lookahead(ba_engine *e, int32_t lookahead) {
  ENGINE_PROLOGUE(e);
  if (lookahead < 1) return fail(BA_E_INVALID, "lookahead must be at least 1");
  if (lookahead > 1 && e->ssm_set && e->ssg.student_block)
    return fail(BA_E_STATE, "the look-ahead does not carry a Student local linear trend's weights: use a look-ahead of 1");
  MUTATE(e);
  {
    // the record: two halves x chains x rounds x (gamma + beta [+ variances, coefficients]);
    // a look-ahead it has no room for (p = 4096 with 1024 chains: 75 MB a round) is cut
    // down to what 2 GiB hold rather than failing in hipMalloc
    const double per_round = 2.0 * (double)e->cfg.chains * ((double)std::max(e->p, 1) * 9.0 + 8.0 * (SSG_MAX_VAR + SSG_MAX_AR * AR_MAX + 1));
    const double budget = 2147483648.0;
    if ((double)lookahead * per_round > budget) lookahead = std::max<int32_t>(1, (int32_t)(budget / per_round));
  }
  e->ssla.len = lookahead;
  e->ssla.cur = 0;
  e->ssla.calm = 0;
  e->ssla.probe_wait = 16;
  ss_la_reset(e);
  return BA_OK;
}

// the chains whose STATE PATH the look-ahead records (default: chain 0); the other chains'
// state is read by going back to the draw being served (correct, and slow)
int ba_ss_lookahead_chains(ba_engine *e, int32_t nchains, const int64_t *chains) {
  ENGINE_PROLOGUE(e);
  if (nchains < 0 || (nchains > 0 && !chains)) return fail(BA_E_INVALID, "bad argument");
  for (int i = 0; i < nchains; ++i)
    if (chains[i] < 0 || chains[i] >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  MUTATE(e);
  e->ssla.reg.clear();
  e->ssla.want.clear();
  for (int i = 0; i < nchains; ++i) e->ssla.reg.push_back((int32_t)chains[i]);
  ss_la_reset(e);
  return BA_OK;
}

int ba_ss_draw_next(ba_engine *e) {
  ENGINE_PROLOGUE_NOJOIN(e);
  {
    int rcj = pipe_join(e);
    if (rcj) return rcj;
  }
  ba_engine::SsLa &A = e->ssla;
  if (A.len > 1 && e->ssm_set && e->ssg.student_block)
    return fail(BA_E_STATE, "the look-ahead does not carry a Student local linear trend's weights: use a look-ahead of 1");
  if (A.len <= 1) return ss_sweep_impl(e, 1, -1);
  if (A.cur <= 1) {
    // (every draw of late was followed by something the record could not serve: one round
    // per call, and another try with a batch of two after a while)
    if (A.cur < 1) A.cur = A.len;   // (first call after ba_ss_set_lookahead)
    else {
      if (++A.calm >= A.probe_wait) { A.cur = 2; A.calm = 0; }
      return ss_sweep_impl(e, 1, -1);
    }
  }
  if (A.served == A.avail) {
    if (A.avail > 0 && A.clean) {   // a batch served to its end in peace
      A.cur = std::min(A.len, A.cur * 2);
      A.probe_wait = 16;
    }
    A.clean = true;
    if (A.ahead) {
      // the record is used up: on to the batch that is already running (or done)
      A.slot ^= 1;
      A.ahead = false;
      A.avail = A.ahead_len;
    } else {
      // ... or from the chains' current state
      int rc = ss_la_settle(e);
      if (!rc) rc = la_rewind(e);
      if (!rc) rc = ss_prepare(e);
      if (!rc) rc = ss_la_alloc(e);
      // (the first impute_state of a run, if it is still to come, is not part of a batch:
      // a batch's snapshot is a point between two rounds)
      if (!rc) rc = ss_sweep_impl(e, 0, -1);
      if (rc) return rc;
      A.slot = 0;
      rc = ss_la_launch(e, 0);
      if (rc) return rc;
      A.avail = A.cur;
    }
    A.served = 0;
    A.synced = false;
    A.cache.clear();
    // the batch after this one goes out now, into the other half
    A.ahead_len = A.cur;
    int rc = ss_la_launch(e, A.slot ^ 1);
    if (rc) return rc;
    A.ahead = true;
  }
  ++A.served;
  return BA_OK;
}

int ba_ss_forecast(ba_engine *e, int32_t horizon, const double *newX, double *out) {
  ENGINE_PROLOGUE(e);
  if (e->data_kind == DATA_SS_STUDENT)
    return fail(BA_E_STATE, "forecasts with Student-t observation noise are not implemented");
  if (e->data_kind == DATA_SS_POISSON)
    return fail(BA_E_STATE, "forecasts with Poisson observation noise are not implemented");
  if (e->data_kind == DATA_SS_LOGIT)
    return fail(BA_E_STATE, "forecasts with binomial observation noise are not implemented");
  if (e->ssm_set && e->ssg.student_block)
    return fail(BA_E_STATE, "forecasts with a Student local linear trend are not implemented");
  if (!newX || !out || horizon <= 0) return fail(BA_E_INVALID, "bad argument");
  if (e->data_kind != DATA_STATE_SPACE || e->dss_scratch.count == 0 || !e->ss_initialized)
    return fail(BA_E_STATE, "no state draw yet: run ba_ss_sweep or ba_ss_impute_state first");
  int rc = hol_prepare(e, horizon);   // (a random-walk holiday: the calendar's entries T .. T + horizon - 1)
  if (rc) return rc;
  rc = ba_sync(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, h = (size_t)horizon;
  DevBuf<double> dnx, dout;
  HIP_TRY(dnx.resize(h * p));
  HIP_TRY(dout.resize(C * h));
  HIP_TRY(hipMemcpyAsync(dnx.ptr, newX, h * p * 8, hipMemcpyHostToDevice, e->stream));
  SsParams S;
  fill_ss_params(e, S);
  if (e->ssm_set)
    HIP_TRY(launch_ssm_forecast(e->stream, S, horizon, dnx.ptr, e->dpos_forecast.ptr, dout.ptr));
  else
    HIP_TRY(launch_ss_forecast(e->stream, S, horizon, dnx.ptr, e->dpos_forecast.ptr, dout.ptr));
  HIP_TRY(hipMemcpyAsync(out, dout.ptr, C * h * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BA_OK;
}

// One-step prediction errors, forecast variances and the log likelihood of the chains' current
// draw (ss_filter_kernel.hip).  An observer: it enqueues its own kernel and copies, and changes
// no stream position, state path, sufficient statistic or snapshot.  While ba_ss_draw_next
// serves a batch the parameters are the served row of the record, and the filter runs on a
// stream of its own behind the batch's event -- beside the batch that is running ahead.
int ba_ss_prediction_errors(ba_engine *e, int64_t chain_first, int64_t chain_count, int32_t standardize,
                            double *errors, double *variances, double *log_likelihood) {
  ENGINE_PROLOGUE_NOJOIN(e);
  {
    int rcj = pipe_join(e);
    if (rcj) return rcj;
  }
  if (e->data_kind == DATA_SS_STUDENT || e->data_kind == DATA_SS_POISSON || e->data_kind == DATA_SS_LOGIT)
    return fail(BA_E_STATE, "one-step prediction errors are built for the Gaussian observation model only");
  if (e->data_kind != DATA_STATE_SPACE) return fail(BA_E_STATE, set_data_first(DATA_STATE_SPACE));
  if (!errors && !variances && !log_likelihood) return fail(BA_E_INVALID, "null argument");
  if (chain_first < 0 || chain_count <= 0 || chain_first >= e->cfg.chains || chain_count > e->cfg.chains - chain_first)
    return fail(BA_E_INVALID, "chain range out of bounds");
  const bool served = ss_la_serving(e);
  int rc = BA_OK;
  if (served) {
    rc = ss_la_wait(e);
  } else {
    rc = ss_prepare(e);
    if (!rc) rc = ba_sync(e);   // (a stopped chain: its error, as ba_ss_forecast)
  }
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, T = (size_t)e->T, n = (size_t)chain_count;
  hipStream_t s = e->stream;
  if (served) {
    if (!e->ssf_stream) HIP_TRY(hipStreamCreateWithFlags(&e->ssf_stream, hipStreamNonBlocking));
    s = e->ssf_stream;   // (ss_la_wait has waited for the batch's event on the host)
  }
  if (e->dssf_err.count < n * T) HIP_TRY(e->dssf_err.resize(n * T));
  if (variances && e->dssf_var.count < n * T) HIP_TRY(e->dssf_var.resize(n * T));
  if (e->dssf_ll.count < n) HIP_TRY(e->dssf_ll.resize(n));
  if (e->dssf_flag.count == 0) HIP_TRY(e->dssf_flag.resize(1));
  SsFilterParams F{};
  F.T = e->T;
  F.p = e->p;
  F.chain_first = (int32_t)chain_first;
  F.chain_count = (int32_t)chain_count;
  F.standardize = standardize ? 1 : 0;
  F.y = e->dss_y.ptr;
  F.X = e->dss_X.ptr;
  F.observed = e->dss_obs.ptr;
  if (e->ssm_set) {
    F.spec = reinterpret_cast<const SsgSpec *>(e->dssg_spec.ptr);
    F.m = e->ssg.m;
    F.nblocks = e->ssg.nblocks;
    F.nvar = e->ssg.nvar;
    F.nar = e->ssg.nar;
    if (e->ssg.student_block) {
      F.qw = e->dslt_w.ptr;   // (a look-ahead above 1 is refused with such a block: always live)
      F.qw_stride = 2 * (int64_t)T;
    }
    if (ssg_has_calendar(e->ssg)) F.cal = e->dhol_cal.ptr;   // (one table for every draw: the record needs none)
  } else {
    // the local-level path: the same kernel on a one-block list
    SsgSpec one{};
    one.m = one.nblocks = one.nvar = 1;
    one.blk[0].kind = SSG_LOCAL_LEVEL;
    one.blk[0].dim = 1;
    one.blk[0].nvar = 1;
    one.blk[0].duration = 1;
    one.blk[0].ar_index = -1;
    one.a0[0] = e->ss_a0;
    one.P0[0] = e->ss_P0;
    if (e->dssf_spec.count == 0) HIP_TRY(e->dssf_spec.resize(sizeof(SsgSpec)));
    HIP_TRY(hipMemcpy(e->dssf_spec.ptr, &one, sizeof(SsgSpec), hipMemcpyHostToDevice));
    F.spec = reinterpret_cast<const SsgSpec *>(e->dssf_spec.ptr);
    F.m = F.nblocks = F.nvar = 1;
    F.nar = 0;
  }
  F.ld = (F.m + 1) | 1;
  if (served) {
    // the draw being served: row served - 1 of every chain, [slot][chain][round][...]
    const ba_engine::SsLa &A = e->ssla;
    const size_t L = (size_t)A.len, at0 = (size_t)A.slot * C * L + (size_t)A.served - 1;
    F.src.gamma = A.rgamma.ptr + at0 * p;
    F.src.beta = A.rbeta.ptr + at0 * p;
    F.src.sigsq = A.rsig.ptr + at0;
    F.src.var = A.rvar.ptr + at0 * A.nvar;
    F.src.phi = A.nphi ? A.rphi.ptr + at0 * A.nphi : nullptr;
    F.src.gamma_stride = F.src.beta_stride = (int64_t)(L * p);
    F.src.sigsq_stride = (int64_t)L;
    F.src.var_stride = (int64_t)(L * A.nvar);
    F.src.phi_stride = (int64_t)(L * A.nphi);
  } else {
    F.src.gamma = e->dgamma.ptr;
    F.src.beta = e->dbeta.ptr;
    F.src.sigsq = e->dsigsq.ptr;
    F.src.gamma_stride = F.src.beta_stride = (int64_t)p;
    F.src.sigsq_stride = 1;
    if (e->ssm_set) {
      F.src.var = e->dssm_sigsq.ptr;
      F.src.var_stride = SSG_MAX_VAR;
      F.src.phi = e->ssg.nar > 0 ? e->dar_phi.ptr : nullptr;
      F.src.phi_stride = SSG_MAX_AR * AR_MAX;
    } else {
      F.src.var = e->dlev_sigsq.ptr;   // (between calls the live value is the one the last state draw used)
      F.src.var_stride = 1;
    }
  }
  F.errors = e->dssf_err.ptr;
  F.variances = variances ? e->dssf_var.ptr : nullptr;
  F.loglik = e->dssf_ll.ptr;
  F.flag = e->dssf_flag.ptr;
  int32_t flag = 0;
  HIP_TRY(hipMemsetAsync(e->dssf_flag.ptr, 0x7f, 4, s));
  HIP_TRY(launch_ss_filter(s, F));
  if (errors) HIP_TRY(hipMemcpyAsync(errors, e->dssf_err.ptr, n * T * 8, hipMemcpyDeviceToHost, s));
  if (variances) HIP_TRY(hipMemcpyAsync(variances, e->dssf_var.ptr, n * T * 8, hipMemcpyDeviceToHost, s));
  if (log_likelihood) HIP_TRY(hipMemcpyAsync(log_likelihood, e->dssf_ll.ptr, n * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&flag, e->dssf_flag.ptr, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (flag >= 0 && flag < e->cfg.chains) {
    char buf[64];
    std::snprintf(buf, sizeof buf, " (chain %lld)", (long long)(e->cfg.chain_offset + (int64_t)flag));
    return fail(BA_E_FORECAST_VARIANCE, std::string("Found a zero (or negative) forecast variance!") + buf);
  }
  return BA_OK;
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

// ---- bsts family = "student": StateSpaceStudentRegressionModel + StateSpaceStudentPosteriorSampler
// (Models/StateSpace/StateSpaceStudentRegressionModel.cpp, PosteriorSamplers/
// StateSpaceStudentPosteriorSampler.cpp:56-126, StateSpacePosteriorSampler.cpp:41-63).  The
// observation model is the Student path's (student_kernel.hip: weights, sigma^2, nu; the
// SpikeSlabSampler sweep on every chain's own V = slab precision + X'WX through the column
// service), the state draw the general structural kernel with H_t = sigma^2 / w_t.
namespace boom_amd {

// the buffers of the kind beyond ss_prepare's and the Student path's: H_t; new weights are 1
// (the first impute_state of StateSpacePosteriorSampler::draw runs before any weight is drawn)
static int sst_buffers(ba_engine *e) {
  int rc = student_prepare(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, T = (size_t)e->T;
  const bool fresh = e->lat.w.count != C * T || e->dsst_h.count != C * T;
  rc = column_buffers(e);
  if (rc) return rc;
  if (e->dstu_u.count != C * T) HIP_TRY(e->dstu_u.resize(C * T));
  if (fresh) {
    HIP_TRY(e->dsst_h.resize(C * T));
    std::vector<double> one(C * T, 1.0);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->lat.w.ptr, one.data(), C * T * 8, hipMemcpyHostToDevice));
    e->sst_ready = false;
  }
  return BA_OK;
}

static int sst_prepare(ba_engine *e) {
  int rc = sweep_refusal(e, DATA_SS_STUDENT);
  if (rc) return rc;
  if (!e->ssm_set)
    return fail(BA_E_STATE, e->ss_level_set
                                ? "the Student-t state-space family takes a list of state models: call ba_ss_add_state_model "
                                  "(a local level is the one-block list), not ba_ss_set_local_level"
                                : "call ba_ss_add_state_model first");
  if (!e->have_slab) return fail(BA_E_STATE, "call ba_sss_set_slab first");
  if (!e->sss_slab_scales)
    return fail(BA_E_INVALID, "the Student-t state-space sampler takes a slab whose precision scales with sigma^2 (scales_with_sigsq = 1)");
  rc = switch_mode(e, 1, 1.0);
  if (rc) return rc;
  rc = ss_prepare(e, DATA_SS_STUDENT);
  if (rc) return rc;
  if (!e->ss_initialized) e->sst_ready = false;
  return sst_buffers(e);
}

static void fill_sst_params(ba_engine *e, SsParams &S, StudentParams &U) {
  fill_ss_params(e, S);
  S.ssm.tpl_trend = S.ssm.tpl_nseasons = S.ssm.tpl_ar_lags = 0;   // always the general kernel
  S.h = e->dsst_h.ptr;
  S.h_stride = e->T;
  fill_student_params(e, U);
  U.offset = S.scratch + S.T;   // (array 1 of a chain's scratch block: the kernel's last pass leaves Z_t'alpha_t there)
  U.offset_stride = S.scratch_stride;
  U.observed = e->dss_obs.ptr;
  U.h = e->dsst_h.ptr;
}

// Base::impute_state with the weights in hand: H_t, the state draw (the state models' parameters
// as they stand when draw == 0), then the offsets' consequences -- z, X'Wz, the diagonal of V
static int sst_impute_state(ba_engine *e, const SsParams &S, const StudentParams &U, int draw) {
  HIP_TRY(launch_student_ss_weights(e->stream, U, 0));
  HIP_TRY(launch_ssm_simsmooth(e->stream, S, draw));
  HIP_TRY(launch_student_ss_suf(e->stream, U, e->lat.Xsq.ptr, e->dA.ptr, e->dxty_c.ptr, e->cols.vdiag.ptr,
                                e->cols.planes.ptr));
  e->ss_initialized = true;
  e->sst_ready = true;
  return BA_OK;
}

}  // namespace boom_amd

extern "C" {

int ba_ss_student_set_data(ba_engine *e, int32_t T, int32_t p, const double *y, const double *X,
                           const uint8_t *observed) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!y || !X) return fail(BA_E_INVALID, "null argument");
  if (T <= 0 || p <= 0) return fail(BA_E_INVALID, "T and p must be positive");
  for (int32_t t = 0; t < T; ++t)
    if ((!observed || observed[t]) && !std::isfinite(y[t])) return fail(BA_E_INVALID, "observed responses must be finite");
  int rc = ba_ss_set_data(e, T, p, y, X, observed);
  if (rc) return rc;
  // the Student path's view of the same data (n = T): X, y, X squared
  std::vector<double> yo((size_t)T);
  for (int32_t t = 0; t < T; ++t) yo[(size_t)t] = (!observed || observed[t]) ? y[t] : 0.0;
  rc = upload_latent_data(e, T, p, X, yo.data(), nullptr, /*squared=*/true, 0);
  if (rc) return rc;
  // a new TRegressionModel and a sampler whose latent data are not initialised
  e->dstu_u.release();
  e->dstu_nu.release();
  e->dstu_dx.release();
  e->dstu_margin.release();
  e->lat.w.release();
  e->dsst_h.release();
  e->sst_round = 0;
  e->sst_ready = false;
  e->data_kind = DATA_SS_STUDENT;
  return BA_OK;
}

int ba_ss_student_get_weights(ba_engine *e, int64_t chain, double *w) {
  ENGINE_PROLOGUE(e);
  if (!w) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != DATA_SS_STUDENT) return fail(BA_E_STATE, set_data_first(DATA_SS_STUDENT));
  return read_chain_row(e, chain, e->lat.w, (size_t)e->T, w, [&] { return sst_buffers(e); });
}

int ba_ss_student_set_weights(ba_engine *e, int64_t chain, const double *w) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!w) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != DATA_SS_STUDENT) return fail(BA_E_STATE, set_data_first(DATA_SS_STUDENT));
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  const size_t T = (size_t)e->T, C = (size_t)e->cfg.chains;
  for (size_t t = 0; t < T; ++t)
    if (!(w[t] >= 0.0) || !std::isfinite(w[t])) return fail(BA_E_INVALID, "Weights must be finite and non-negative.");
  int rc = sst_buffers(e);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t c = chain < 0 ? 0 : (size_t)chain; c < (chain < 0 ? C : (size_t)chain + 1); ++c)
    HIP_TRY(hipMemcpy(e->lat.w.ptr + c * T, w, T * 8, hipMemcpyHostToDevice));
  e->sst_ready = false;   // (the statistics in hand are not these weights': the next call draws the state first)
  return BA_OK;
}

int ba_ss_student_impute_state(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  int rc = sst_prepare(e);
  if (rc) return rc;
  SsParams S;
  StudentParams U;
  fill_sst_params(e, S, U);
  rc = sst_impute_state(e, S, U, 0);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return check_chain_status(e);
}

// nsweeps x StateSpacePosteriorSampler::draw (StateSpacePosteriorSampler.cpp:41-63) with the
// Student observation model, every chain
int ba_ss_student_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = sst_prepare(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p;
  if (e->trace_stride > 0 && nsweeps > e->trace_stride)
    return fail(BA_E_INVALID, "nsweeps exceeds the enabled trace length");
  if (e->trace_stride > 0 && e->dstu_nu_rec.count != C * e->trace_stride) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(e->dstu_nu_rec.resize(C * e->trace_stride));
  }
  SsvsParams P;
  fill_params(e, P);
  SsParams S;
  StudentParams U;
  fill_sst_params(e, S, U);
  if (e->trace_stride > 0) HIP_TRY(hipMemsetAsync(e->dtrace_idx.ptr, 0, C * 4, e->stream));
  if (nsweeps == 0) return BA_OK;
  if (!e->sst_ready) {
    // the sampler's first draw(): impute_state with the weights as they stand (1 unless the
    // caller set them), then -- latent data not initialised yet -- impute_nonstate_latent_data.
    // Those weights are replaced by the round's own before any statistic reads them (the
    // statistics are taken at impute_state): they go to the z buffer, which the X'Wz GEMM has
    // finished with, and w stays what the statistics in hand were built from.
    const bool first = !e->ss_initialized;
    rc = sst_impute_state(e, S, U, 0);
    if (rc) return rc;
    if (first) {
      StudentParams W = U;
      W.w = e->lat.z.ptr;
      W.sweep = e->lat.draws++;
      HIP_TRY(launch_student_ss_weights(e->stream, W, 1));
    }
  }
  for (int i = 0; i < nsweeps; ++i) {
    // 1. the observation model's sampler with fix_latent_data(true)
    // (TRegressionSpikeSlabSampler::draw, TRegressionSpikeSlabSampler.cpp:41-47): indicators and
    // beta on the statistics of the last impute_state ...
    HIP_TRY(launch_xtwx_cols_start(e->stream, e->dgamma.ptr, (int)C, (int)p, e->cols.req.ptr, e->cols.count.ptr,
                                   e->cols.valid.ptr, e->cols.words));
    int32_t R = 0;
    HIP_TRY(hipMemcpyAsync(&R, e->cols.count.ptr, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = build_columns(e, R);
    if (rc) return rc;
    HIP_TRY(launch_sweeps(e, P, 1));
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = check_chain_status(e);   // (park-and-replay for vectors of V asked for mid-sweep)
    if (rc) return rc;
    // 2. ... sigma^2, nu
    U.sweep = e->sst_round++;
    HIP_TRY(launch_student_sigma_nu(e->stream, U));
    // 3. - 5. impute_nonstate_latent_data, then the state models' samplers and impute_state (one
    // kernel: the samplers read their own streams and the statistics of the last state draw, so
    // their place before or after the weights does not show)
    U.sweep = e->lat.draws++;
    HIP_TRY(launch_student_ss_weights(e->stream, U, 1));
    HIP_TRY(launch_ssm_simsmooth(e->stream, S, 1));
    // 6. the complete-data statistics of the next round's observation draw
    HIP_TRY(launch_student_ss_suf(e->stream, U, e->lat.Xsq.ptr, e->dA.ptr, e->dxty_c.ptr, e->cols.vdiag.ptr,
                                  e->cols.planes.ptr));
    fill_params(e, P);
  }
  e->table_ok = false;
  e->model_ok = false;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return check_chain_status(e);
}

}  // extern "C"

// ---- bsts family = "poisson" and family = "logit": StateSpacePoissonModel + StateSpacePoissonPosteriorSampler
// (Models/StateSpace/StateSpacePoissonModel.cpp, PosteriorSamplers/StateSpacePoissonPosteriorSampler.cpp:
// 79-147), StateSpaceLogitModel + StateSpaceLogitPosteriorSampler (StateSpaceLogitModel.cpp,
// StateSpaceLogitPosteriorSampler.cpp:49-123), both under StateSpacePosteriorSampler.cpp:42-64.  The
// observation model is the family's regression path's (probit_kernel.hip: the auxiliary-mixture
// imputation; the SpikeSlabSampler sweep at sigma^2 = 1 on every chain's own V = slab precision +
// X'QX through the column service), the state draw the general structural kernel on every chain's
// own series v_t with H_t = 1 / q_t.  One set of helpers serves both kinds; what differs is here:
namespace boom_amd {

// the kind's family number for the launchers (probit_kernel.hip), its name in a refusal, and the
// precision a new model gives an observed step: 1 (AugmentedPoissonRegressionData::add_data), or
// 4 / n_t (AugmentedBinomialRegressionData::add_data, StateSpaceLogitModel.cpp:67-74)
static int ssp_family(const ba_engine *e) { return e->data_kind == DATA_SS_LOGIT ? 1 : 0; }
static double ssp_initial_precision(const ba_engine *e, size_t t) {
  return e->data_kind == DATA_SS_LOGIT ? 4.0 / e->ssp_trials[t] : 1.0;
}

// the buffers of the kind beyond ss_prepare's and the column service's: v_t and H_t; new latent
// data are v = 0, q = the family's initial precision (0 where the step is missing)
static int ssp_buffers(ba_engine *e) {
  int rc = alloc_chain_state(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, T = (size_t)e->T;
  const bool fresh = e->lat.w.count != C * T || e->dssp_value.count != C * T || e->dssp_h.count != C * T;
  rc = column_buffers(e);
  if (rc) return rc;
  if (fresh) {
    HIP_TRY(e->dssp_value.resize(C * T));
    HIP_TRY(e->dssp_h.resize(C * T));
    std::vector<double> q(C * T);
    for (size_t c = 0; c < C; ++c)
      for (size_t t = 0; t < T; ++t) q[c * T + t] = e->ssp_observed[t] ? ssp_initial_precision(e, t) : 0.0;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->lat.w.ptr, q.data(), C * T * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(e->dssp_value.ptr, 0, C * T * 8));
    e->ssp_ready = false;
  }
  return BA_OK;
}

static int ssp_prepare(ba_engine *e, DataKind kind) {
  int rc = sweep_refusal(e, kind);
  if (rc) return rc;
  const bool logit = kind == DATA_SS_LOGIT;
  if (!logit && !e->poisson_mix_set) return fail(BA_E_STATE, "call ba_poisson_set_mixtures first");
  if (!e->ssm_set) {
    if (!e->ss_level_set) return fail(BA_E_STATE, "call ba_ss_add_state_model first");
    return fail(BA_E_STATE, logit ? "the logit state-space family takes a list of state models: call ba_ss_add_state_model "
                                    "(a local level is the one-block list), not ba_ss_set_local_level"
                                  : "the Poisson state-space family takes a list of state models: call ba_ss_add_state_model "
                                    "(a local level is the one-block list), not ba_ss_set_local_level");
  }
  if (!e->have_slab) return fail(BA_E_STATE, "call ba_sss_set_slab first");
  if (e->sss_slab_scales)
    return fail(BA_E_INVALID, logit ? "the logit state-space sampler takes a fixed-precision slab (scales_with_sigsq = 0)"
                                    : "the Poisson state-space sampler takes a fixed-precision slab (scales_with_sigsq = 0)");
  rc = switch_mode(e, 1, 1.0);
  if (rc) return rc;
  rc = ss_prepare(e, kind);
  if (rc) return rc;
  rc = set_unit_sigsq(e);   // (the latent data have unit variance, as in logit_family_sweep)
  if (rc) return rc;
  if (!e->ss_initialized) e->ssp_ready = false;
  return ssp_buffers(e);
}

static void fill_ssp_params(ba_engine *e, SsParams &S, ProbitParams &Q) {
  fill_ss_params(e, S);
  S.ssm.tpl_trend = S.ssm.tpl_nseasons = S.ssm.tpl_ar_lags = 0;   // always the general kernel
  S.h = e->dssp_h.ptr;
  S.h_stride = e->T;
  S.y = e->dssp_value.ptr;   // (v itself: the kernel subtracts x'beta)
  S.y_stride = e->T;
  fill_probit_params(e, Q);
  Q.offset = S.scratch + S.T;   // (array 1 of a chain's scratch block: the kernel's last pass leaves Z_t'alpha_t there)
  Q.offset_stride = S.scratch_stride;
  Q.observed = e->dss_obs.ptr;
  Q.value = e->dssp_value.ptr;
  Q.h = e->dssp_h.ptr;
}

// Base::impute_state with the latent data in hand: H_t, the state draw (the state models'
// parameters as they stand when draw == 0), then the offsets' consequences -- z, X'Qz, the diagonal of V
static int ssp_impute_state(ba_engine *e, const SsParams &S, const ProbitParams &Q, int draw) {
  const int family = ssp_family(e);
  HIP_TRY(launch_latent_ss_h(e->stream, Q, family, 0));
  HIP_TRY(launch_ssm_simsmooth(e->stream, S, draw));
  HIP_TRY(launch_latent_ss_suf(e->stream, Q, family, e->lat.Xsq.ptr, e->dA.ptr, e->cols.vdiag.ptr, e->cols.planes.ptr));
  e->ss_initialized = true;
  e->ssp_ready = true;
  return BA_OK;
}

// ba_ss_poisson_get_latent / ba_ss_logit_get_latent
static int ssp_get_latent(ba_engine *e, DataKind kind, int64_t chain, double *value, double *precision) {
  if (!value || !precision) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != kind) return fail(BA_E_STATE, set_data_first(kind));
  int rc = read_chain_row(e, chain, e->dssp_value, (size_t)e->T, value, [&] { return ssp_buffers(e); });
  if (rc) return rc;
  return read_chain_row(e, chain, e->lat.w, (size_t)e->T, precision, [&] { return BA_OK; });
}

// ba_ss_poisson_set_latent / ba_ss_logit_set_latent
static int ssp_set_latent(ba_engine *e, DataKind kind, int64_t chain, const double *value, const double *precision) {
  if (!value || !precision) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != kind) return fail(BA_E_STATE, set_data_first(kind));
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  const size_t T = (size_t)e->T, C = (size_t)e->cfg.chains;
  std::vector<double> v(T, 0.0), q(T, 0.0);   // (a missing step's entries are not read)
  for (size_t t = 0; t < T; ++t) {
    if (!e->ssp_observed[t]) continue;
    if (precision[t] < 0) return fail(BA_E_INVALID, "precision must be non-negative.");
    // (the reference takes these and then filters with a variance of -infinity)
    if (!(precision[t] > 0) || !std::isfinite(precision[t]))
      return fail(BA_E_INVALID, "the precision of an observed step must be positive and finite");
    if (!std::isfinite(value[t])) return fail(BA_E_INVALID, "the latent value of an observed step must be finite");
    v[t] = value[t];
    q[t] = precision[t];
  }
  int rc = ssp_buffers(e);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t c = chain < 0 ? 0 : (size_t)chain; c < (chain < 0 ? C : (size_t)chain + 1); ++c) {
    HIP_TRY(hipMemcpy(e->dssp_value.ptr + c * T, v.data(), T * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->lat.w.ptr + c * T, q.data(), T * 8, hipMemcpyHostToDevice));
  }
  e->ssp_ready = false;   // (the statistics in hand are not these data's: the next call draws the state first)
  return BA_OK;
}

// ba_ss_poisson_impute_state / ba_ss_logit_impute_state
static int ssp_impute_state_entry(ba_engine *e, DataKind kind) {
  int rc = ssp_prepare(e, kind);
  if (rc) return rc;
  SsParams S;
  ProbitParams Q;
  fill_ssp_params(e, S, Q);
  rc = ssp_impute_state(e, S, Q, 0);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return check_chain_status(e);
}

// ba_ss_poisson_sweep / ba_ss_logit_sweep: nsweeps x StateSpacePosteriorSampler::draw
// (StateSpacePosteriorSampler.cpp:42-64) with the kind's observation model, every chain
static int ssp_sweep(ba_engine *e, DataKind kind, int32_t nsweeps) {
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = ssp_prepare(e, kind);
  if (rc) return rc;
  const int family = ssp_family(e);
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p;
  if (e->trace_stride > 0 && nsweeps > e->trace_stride)
    return fail(BA_E_INVALID, "nsweeps exceeds the enabled trace length");
  SsvsParams P;
  fill_params(e, P);
  SsParams S;
  ProbitParams Q;
  fill_ssp_params(e, S, Q);
  if (e->trace_stride > 0) HIP_TRY(hipMemsetAsync(e->dtrace_idx.ptr, 0, C * 4, e->stream));
  if (nsweeps == 0) return BA_OK;
  if (!e->ssp_ready) {
    // the sampler's first draw(): impute_state with the latent data as they stand (v = 0, q = the
    // family's initial precision unless the caller set them), then -- latent data not initialised
    // yet -- impute_nonstate_latent_data.  Every value that imputation writes is overwritten by the
    // round's own (step 3 below) before anything reads it -- the statistics are taken at
    // impute_state -- so it is not launched; only its slots of the imputation stream (11 Poisson,
    // 9 logit) are used up: the counter moves on, and round r of a fresh sampler imputes with
    // s = r + 1.
    const bool first = !e->ss_initialized;
    rc = ssp_impute_state(e, S, Q, 0);
    if (rc) return rc;
    if (first) ++e->lat.draws;
  }
  for (int i = 0; i < nsweeps; ++i) {
    // 1. the observation model's sampler with fix_latent_data(true)
    // (PoissonRegressionSpikeSlabSampler::draw, PoissonRegressionSpikeSlabSampler.cpp:55-59;
    // BinomialLogitSpikeSlabSampler::draw): indicators and beta at sigma^2 = 1 on the statistics
    // of the last impute_state
    HIP_TRY(launch_xtwx_cols_start(e->stream, e->dgamma.ptr, (int)C, (int)p, e->cols.req.ptr, e->cols.count.ptr,
                                   e->cols.valid.ptr, e->cols.words));
    int32_t R = 0;
    HIP_TRY(hipMemcpyAsync(&R, e->cols.count.ptr, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = build_columns(e, R);
    if (rc) return rc;
    HIP_TRY(launch_sweeps(e, P, 1));
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = check_chain_status(e);   // (park-and-replay for vectors of V asked for mid-sweep)
    if (rc) return rc;
    // 2. - 4. impute_nonstate_latent_data at the new beta and the last state draw, then the state
    // models' samplers and impute_state (one kernel: the samplers read their own streams and the
    // statistics of the last state draw, so their place before or after the imputation does not show)
    Q.sweep = e->lat.draws++;
    HIP_TRY(launch_latent_ss_h(e->stream, Q, family, 1));
    HIP_TRY(launch_ssm_simsmooth(e->stream, S, 1));
    // 5. the complete-data statistics of the next round's observation draw
    HIP_TRY(launch_latent_ss_suf(e->stream, Q, family, e->lat.Xsq.ptr, e->dA.ptr, e->cols.vdiag.ptr, e->cols.planes.ptr));
    fill_params(e, P);
  }
  e->table_ok = false;
  e->model_ok = false;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return check_chain_status(e);
}

}  // namespace boom_amd

extern "C" {

int ba_ss_poisson_set_data(ba_engine *e, int32_t T, int32_t p, const double *counts, const double *exposure,
                           const double *X, const uint8_t *observed) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!counts || !exposure || !X) return fail(BA_E_INVALID, "null argument");
  if (T <= 0 || p <= 0) return fail(BA_E_INVALID, "T and p must be positive");
  // (a missing step's count and exposure are never read: 0 and 1 stand in for them on the device)
  std::vector<double> yo((size_t)T, 0.0), ex((size_t)T, 1.0);
  std::vector<uint8_t> obs((size_t)T, 1);
  for (int32_t t = 0; t < T; ++t) {
    if (observed && !observed[t]) { obs[(size_t)t] = 0; continue; }
    if (!(counts[t] >= 0) || counts[t] != std::floor(counts[t])) return fail(BA_E_INVALID, "counts must be non-negative integers");
    if (!(exposure[t] > 0)) return fail(BA_E_INVALID, "exposures must be positive");
    yo[(size_t)t] = counts[t];
    ex[(size_t)t] = exposure[t];
  }
  int rc = ba_ss_set_data(e, T, p, yo.data(), X, observed);
  if (rc) return rc;
  // the Poisson path's view of the same data (n = T): X, counts, exposures, X squared
  rc = upload_latent_data(e, T, p, X, yo.data(), ex.data(), /*squared=*/true, 0);
  if (rc) return rc;
  e->poisson_y.resize((size_t)T);
  for (int32_t t = 0; t < T; ++t) e->poisson_y[(size_t)t] = (int64_t)std::llround(yo[(size_t)t]);   // (missing: 0, "unused")
  e->poisson_mix_set = false;
  // a new model (v = 0, q = 1) and a sampler whose latent data are not initialised
  e->ssp_observed = obs;
  e->lat.w.release();
  e->dssp_value.release();
  e->dssp_h.release();
  e->ssp_ready = false;
  e->data_kind = DATA_SS_POISSON;
  return BA_OK;
}

int ba_ss_poisson_get_latent(ba_engine *e, int64_t chain, double *value, double *precision) {
  ENGINE_PROLOGUE(e);
  return ssp_get_latent(e, DATA_SS_POISSON, chain, value, precision);
}

int ba_ss_poisson_set_latent(ba_engine *e, int64_t chain, const double *value, const double *precision) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_set_latent(e, DATA_SS_POISSON, chain, value, precision);
}

int ba_ss_poisson_impute_state(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_impute_state_entry(e, DATA_SS_POISSON);
}

int ba_ss_poisson_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_sweep(e, DATA_SS_POISSON, nsweeps);
}

// ---- bsts family = "logit"
int ba_ss_logit_set_data(ba_engine *e, int32_t T, int32_t p, const double *successes, const double *trials,
                         const double *X, const uint8_t *observed, int32_t clt_threshold) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!successes || !trials || !X) return fail(BA_E_INVALID, "null argument");
  if (T <= 0 || p <= 0) return fail(BA_E_INVALID, "T and p must be positive");
  // (as in ba_logit_set_data: two uniforms per trial of the step's substream of LOGIT_STRIDE)
  if (clt_threshold < 1 || 4 * clt_threshold > LOGIT_STRIDE)
    return fail(BA_E_INVALID, "clt_threshold must be between 1 and 64");
  // (a missing step's successes and trials are never read: 0 and 1 stand in for them on the device)
  std::vector<double> yo((size_t)T, 0.0), nt((size_t)T, 1.0);
  std::vector<uint8_t> obs((size_t)T, 1);
  for (int32_t t = 0; t < T; ++t) {
    if (observed && !observed[t]) { obs[(size_t)t] = 0; continue; }
    // (the reference takes n_t = 0 and then filters with a latent value that is not a number)
    if (!(trials[t] >= 1) || trials[t] != std::floor(trials[t]) || !(trials[t] <= 2147483647.0))
      return fail(BA_E_INVALID, "trials must be integers of at least 1 at the observed steps");
    if (!(successes[t] >= 0) || successes[t] != std::floor(successes[t]))
      return fail(BA_E_INVALID, "successes must be non-negative integers");
    if (successes[t] > trials[t]) return fail(BA_E_INVALID, "The number of successes must not exceed the number of trials.");
    yo[(size_t)t] = successes[t];
    nt[(size_t)t] = trials[t];
  }
  int rc = ba_ss_set_data(e, T, p, yo.data(), X, observed);
  if (rc) return rc;
  // the logit path's view of the same data (n = T): X, successes, trials, X squared
  rc = upload_latent_data(e, T, p, X, yo.data(), nt.data(), /*squared=*/true, clt_threshold);
  if (rc) return rc;
  // a new model (v = 0, q = 4 / n_t) and a sampler whose latent data are not initialised
  e->ssp_observed = obs;
  e->ssp_trials = nt;
  e->lat.w.release();
  e->dssp_value.release();
  e->dssp_h.release();
  e->ssp_ready = false;
  e->data_kind = DATA_SS_LOGIT;
  return BA_OK;
}

int ba_ss_logit_get_latent(ba_engine *e, int64_t chain, double *value, double *precision) {
  ENGINE_PROLOGUE(e);
  return ssp_get_latent(e, DATA_SS_LOGIT, chain, value, precision);
}

int ba_ss_logit_set_latent(ba_engine *e, int64_t chain, const double *value, const double *precision) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_set_latent(e, DATA_SS_LOGIT, chain, value, precision);
}

int ba_ss_logit_impute_state(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_impute_state_entry(e, DATA_SS_LOGIT);
}

int ba_ss_logit_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_sweep(e, DATA_SS_LOGIT, nsweeps);
}

}  // extern "C"

// ---- forecasts of the three families: simulate_forecast of StateSpaceStudentRegressionModel,
// StateSpacePoissonModel and StateSpaceLogitModel for every chain's current draw
// (ss_family_forecast_kernel.hip)
namespace boom_amd {

// scale: the horizon's exposures (Poisson) or trial counts (logit), validated; nullptr: ones
// (and for the Student-t family, which has none)
static int ss_family_forecast(ba_engine *e, DataKind kind, int32_t horizon, const double *newX, const double *scale,
                              double *out) {
  if (e->data_kind != kind) return fail(BA_E_STATE, set_data_first(kind));
  if (!newX || !out || horizon <= 0) return fail(BA_E_INVALID, "bad argument");
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, h = (size_t)horizon;
  const bool student = kind == DATA_SS_STUDENT, logit = kind == DATA_SS_LOGIT;
  std::vector<double> sc(h, 1.0);
  for (size_t i = 0; scale && i < h; ++i) {
    if (!(scale[i] >= 0.0) || !std::isfinite(scale[i]))
      return fail(BA_E_INVALID, logit ? "trial counts of a forecast must be non-negative and finite"
                                      : "exposures of a forecast must be non-negative and finite");
    sc[i] = logit ? std::round(scale[i]) : scale[i];   // (lround(trials[i]), StateSpaceLogitModel.cpp:245)
  }
  if (!e->ssm_set || e->dssm_work.count == 0 || !e->ss_initialized || (student && e->dstu_nu.count != C))
    return fail(BA_E_STATE, student ? "no state draw yet: run ba_ss_student_sweep or ba_ss_student_impute_state first"
                            : logit ? "no state draw yet: run ba_ss_logit_sweep or ba_ss_logit_impute_state first"
                                    : "no state draw yet: run ba_ss_poisson_sweep or ba_ss_poisson_impute_state first");
  int rc = ba_sync(e);
  if (rc) return rc;
  DevBuf<double> dnx, dsc, dout;
  HIP_TRY(dnx.resize(h * p));
  HIP_TRY(dsc.resize(h));
  HIP_TRY(dout.resize(C * h));
  HIP_TRY(hipMemcpyAsync(dnx.ptr, newX, h * p * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(dsc.ptr, sc.data(), h * 8, hipMemcpyHostToDevice, e->stream));
  SsParams S;
  fill_ss_params(e, S);
  const int family = student ? SS_FORECAST_STUDENT : logit ? SS_FORECAST_LOGIT : SS_FORECAST_POISSON;
  HIP_TRY(launch_ss_family_forecast(e->stream, S, family, horizon, dnx.ptr, dsc.ptr, e->dstu_nu.ptr,
                                    e->dpos_forecast.ptr, dout.ptr));
  HIP_TRY(hipMemcpyAsync(out, dout.ptr, C * h * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));   // (sc and the pageable copies are done with)
  return BA_OK;
}

}  // namespace boom_amd

extern "C" {

int ba_ss_student_forecast(ba_engine *e, int32_t horizon, const double *newX, double *out) {
  ENGINE_PROLOGUE(e);
  return ss_family_forecast(e, DATA_SS_STUDENT, horizon, newX, nullptr, out);
}

int ba_ss_poisson_forecast(ba_engine *e, int32_t horizon, const double *newX, const double *exposure, double *out) {
  ENGINE_PROLOGUE(e);
  return ss_family_forecast(e, DATA_SS_POISSON, horizon, newX, exposure, out);
}

int ba_ss_logit_forecast(ba_engine *e, int32_t horizon, const double *newX, const double *trials, double *out) {
  ENGINE_PROLOGUE(e);
  return ss_family_forecast(e, DATA_SS_LOGIT, horizon, newX, trials, out);
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
