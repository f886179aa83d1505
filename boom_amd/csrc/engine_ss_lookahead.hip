// The look-ahead on the bsts path: ba_ss_set_lookahead / ba_ss_draw_next, the record of every
// round's draw and the snapshots a rewind restores.
#include "engine_internal.h"

namespace boom_amd {

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

hipError_t ss_la_record(ba_engine *e, int slot, int round) {
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
// (a dynamic regression adds nothing: its d variances, statistics and positions sit in the state
// models' slots, and its predictors are one table for all chains and all draws)
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
  if (e->ssm_set) field(e->dar_gamma.ptr, ssg_has(e->ssg, SSG_HAS_AR_SPIKE) ? C * SSG_MAX_AR * AR_MAX / 8 : 0);
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
bool ss_la_registered(const ba_engine *e, int64_t c) {
  for (int32_t r : e->ssla.reg)
    if (r == c) return true;
  return false;
}
// A chain whose state path was asked for and is not in the record: this read goes back to the
// draw being served (ss_la_settle), the batches from here on record the chain too -- a caller
// that reads chain c after every draw pays for it once, not every time.
// (the list the device buffers are sized by, `reg`, changes in ss_la_alloc only; the state
// record is bounded there)
void ss_la_want_state(ba_engine *e, int64_t c) {
  ba_engine::SsLa &A = e->ssla;
  if (ss_la_registered(e, c)) return;
  for (int32_t w : A.want)
    if (w == c) return;
  if (A.reg.size() + A.want.size() < 32) A.want.push_back((int32_t)c);
}

}  // namespace boom_amd

extern "C" {

// The callers' loop on the bsts path -- for (i in niter) { model.sample_posterior(); record }
// (Interfaces/R/bsts/src/bsts.cc:82-119) -- at the device's rate: rounds are enqueued
// `lookahead` at a time, every round's draw recorded on the device, and ba_ss_draw_next
// hands them out one per call; the accessors below see the draw being served.
int ba_ss_set_lookahead(ba_engine *e, int32_t lookahead) {
  ENGINE_PROLOGUE(e);
  if (lookahead < 1) return fail(BA_E_INVALID, "lookahead must be at least 1");
  if (lookahead > 1 && ss_refused(e, e->data_kind, SSG_USE_LOOKAHEAD)) return BA_E_STATE;
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
  if (A.len > 1 && ss_refused(e, e->data_kind, SSG_USE_LOOKAHEAD)) return BA_E_STATE;
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

}  // extern "C"
