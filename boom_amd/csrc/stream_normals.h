// The standard normals of one simulate_forward (StateSpaceModelBase.cpp:771-790), N of
// them, by all threads of a workgroup.
//
// The reference reads ONE sequential stream: normal i starts where normal i - 1
// stopped, and Kinderman-Ramage (Bmath/snorm.cpp:287-340) consumes a data-dependent
// number of uniforms (two in 88 % of the draws, more in the tail regions), so a
// parallel reader of that stream first has to find where every draw starts.  Rounds 1
// and 2 did exactly that (windows of uniforms in LDS, the draw starting at every
// offset, jump tables, a binary-lifting walk): parity-exact, and 55 % of the Kalman
// kernel.  A counter-based generator does not need it: normal number s of the chain's state
// stream OWNS the positions [s * STATE_SLOT_STRIDE, (s + 1) * STATE_SLOT_STRIDE) (the way the
// probit / logit imputers give every observation its own substream, probit_kernel.hip), so
// every draw is independent of every other.  Rounds 2-5 made each draw a Kinderman-Ramage
// transform of its own slot's uniforms: one Philox block (twenty 32 x 32 -> 64 multiplies at
// 32 cycles a wave instruction) per normal, plus the rejection branches of 12 % of the draws
// worked off from lists in LDS -- 79 wave-microseconds of a 109 us bsts round.
//
// Round 6 (VERDICT r5 task 2 (i)): TWO draws per Philox block.  Draws 2 j and 2 j + 1 (global
// draw numbers: the stream position / STATE_SLOT_STRIDE) are the Box-Muller pair of the two
// uniforms at the start of slot 2 j:
//     R = sqrt(-2 log(1 - u1)),  z_{2j} = R cos(2 pi u2),  z_{2j+1} = R sin(2 pi u2)
// -- exact standard normals from full 53-bit uniforms, half the multiplies per normal, no
// rejection branch, no lists, no second phase.  The oracle's Philox mode draws the same way
// (bo_rnorm on stream 2); its MT mode -- the one pinned on the compiled reference -- reads in
// sequence through norm_rand, as the reference does.  The link between the two has been
// distributional since round 2 and is checked as such (tests/test_substream_bridge.py).
#pragma once
#include <hip/hip_runtime.h>

#include "device_rng.h"
#include "ssvs_params.h"
#include "wave_lanes.h"   // (wave_lds_sync: the one-wave team's hand-off)

namespace boom_amd {

// positions reserved per normal of the state stream (counters, not memory).  A slot's first two
// uniforms are all a Box-Muller pair reads; the imputers' slots (probit_kernel.hip) are the
// ones that can overrun into their spill streams (device_rng.h).
enum : int { STATE_SLOT_STRIDE = 256 };
// (ba_set_slot_limit, for the tests of the imputers' spill streams; the state stream ignores it)
template <class Params>
__host__ __device__ inline int ss_slot_serve(const Params &P) {
  return (P.slot_limit >= 2 && P.slot_limit < STATE_SLOT_STRIDE) ? (P.slot_limit & ~1) : STATE_SLOT_STRIDE;
}

// (the generator needs no LDS any more; kept so that the kernels' LDS layouts keep their names)
struct NormalsLds {
  int unused;
};

// Which draw lands in which slot of the output array, a PAIR of slots at a time (the two slots
// one thread fills from one Philox block where the layout allows).  npairs(par): slot pairs,
// given the parity of the sweep's first global draw number; pair(q, par, &sa, &sb): the output
// slots of pair q (-1: none); draw(s): the index of the sweep's draw that belongs in slot s, or
// -1.  Threads walk the slot pairs, so the stores are coalesced whatever the layout.
struct NormalsInOrder {   // szz[i] = draw i; pair q = the draws of global pair (first >> 1) + q
  int N;
  __device__ __forceinline__ int npairs(int par) const { return (N + par + 1) >> 1; }
  __device__ __forceinline__ void pair(int q, int par, int *sa, int *sb) const {
    const int a = 2 * q - par;
    *sa = (a >= 0 && a < N) ? a : -1;
    *sb = (a + 1 < N) ? a + 1 : -1;
  }
  __device__ __forceinline__ int draw(int s) const { return s; }
};
// ONE_WAVE: the calling wavefront alone makes the draws (the round kernel of
// ss_round_kernel.hip: the chain's other wavefront is in the regression sweep meanwhile);
// the team is then the wave's 64 lanes and the hand-offs are wave-level.
template <bool ONE_WAVE>
struct NormalsTeam {
  static __device__ __forceinline__ int tid() {
    int t = (int)threadIdx.x;
    BA_OPAQUE_V(t);
    return ONE_WAVE ? (t & 63) : t;
  }
  static __device__ __forceinline__ int nth() { return ONE_WAVE ? 64 : (int)blockDim.x; }
  static __device__ __forceinline__ void sync() {
    if (ONE_WAVE) wave_lds_sync(); else __syncthreads();
  }
};

// the Box-Muller pair of Philox block `block` of the chain's state stream
__device__ __forceinline__ void normal_pair(const PhiloxKey &key, uint64_t block, double *zc, double *zs) {
  double u1, u2;
  philox_pair(key, block, &u1, &u2);
  const double R = sqrt(-2.0 * log(1.0 - u1));
  double sn, cs;
  sincos(6.283185307179586 * u2, &sn, &cs);
  *zc = R * cs;
  *zs = R * sn;
}

// Slot pairs [q0, q0 + nq) of the output array, by one team.  bslot0 = the global number of the
// sweep's first draw (stream position / STATE_SLOT_STRIDE).  A pair's two slots take their
// draws from one block when the draws are the two halves of one global pair (the usual case:
// the layouts put a time step's state-error and observation normals side by side, and a sweep
// of the local-level model makes an even number of draws); otherwise the second slot costs a
// block of its own.
template <class Team, class Slots>
__device__ __forceinline__ void normals_pairs(const PhiloxKey &key, uint64_t bslot0, double *szz, const Slots slots,
                                              const int q0, const int nq) {
  const int tid = Team::tid(), nth = Team::nth();
  const int par = (int)(bslot0 & 1ull);
  // (two pairs per thread and round: two independent Philox blocks in flight -- a block is a
  // chain of ten dependent rounds)
  for (int i0 = tid; i0 < nq; i0 += 2 * nth) {
    int sa[2], sb[2];
    uint64_t ga[2], gb[2];
    double zc[2], zs[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = i0 + u * nth;
      sa[u] = sb[u] = -1;
      if (i < nq) slots.pair(q0 + i, par, &sa[u], &sb[u]);
      const int da = sa[u] >= 0 ? slots.draw(sa[u]) : -1, db = sb[u] >= 0 ? slots.draw(sb[u]) : -1;
      if (da < 0) sa[u] = -1;
      if (db < 0) sb[u] = -1;
      ga[u] = bslot0 + (uint64_t)(da < 0 ? 0 : da);
      gb[u] = bslot0 + (uint64_t)(db < 0 ? 0 : db);
      // the block of the first slot's draw (of the second's, where the first holds none)
      const uint64_t g = sa[u] >= 0 ? ga[u] : gb[u];
      normal_pair(key, ((g & ~1ull) * STATE_SLOT_STRIDE) >> 1, &zc[u], &zs[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (sa[u] >= 0) szz[sa[u]] = (ga[u] & 1ull) ? zs[u] : zc[u];
      const bool same = sa[u] < 0 || (gb[u] >> 1) == (ga[u] >> 1);
      if (sb[u] >= 0 && same) szz[sb[u]] = (gb[u] & 1ull) ? zs[u] : zc[u];
      // (a second slot whose draw is half of ANOTHER global pair: rare -- a sweep that starts on
      // an odd draw number in a layout that pairs by time step)
      if (__ballot(sb[u] >= 0 && !same) != 0ull) {
        double c2, s2;
        normal_pair(key, ((gb[u] & ~1ull) * STATE_SLOT_STRIDE) >> 1, &c2, &s2);
        if (sb[u] >= 0 && !same) szz[sb[u]] = (gb[u] & 1ull) ? s2 : c2;
      }
    }
  }
}

// szz[slot] = the sweep's normals in the slots' layout; the stream position moves on by N slots.
// Every thread of the team calls it (it contains the team's barrier); returns the chain status
// (CHAIN_OK: a Box-Muller draw cannot overrun its slot), the same in every thread.
template <bool ONE_WAVE = false, class Slots>
__device__ __forceinline__ int stream_normals(NormalsLds &, const PhiloxKey &key, uint64_t bpos0, int N,
                                              double *szz, uint64_t *pos_out, const Slots slots,
                                              int = STATE_SLOT_STRIDE) {
  typedef NormalsTeam<ONE_WAVE> Team;
  const uint64_t bslot0 = bpos0 / STATE_SLOT_STRIDE;   // (the stream position is a whole number of slots)
  normals_pairs<Team>(key, bslot0, szz, slots, 0, slots.npairs((int)(bslot0 & 1ull)));
  Team::sync();
  if (Team::tid() == 0) *pos_out = bpos0 + (uint64_t)N * STATE_SLOT_STRIDE;
  return CHAIN_OK;
}
__device__ __forceinline__ int stream_normals(NormalsLds &L, const PhiloxKey &key, uint64_t bpos0, int N,
                                              double *szz, uint64_t *pos_out, int serve = STATE_SLOT_STRIDE) {
  return stream_normals<false>(L, key, bpos0, N, szz, pos_out, NormalsInOrder{N}, serve);
}

}  // namespace boom_amd
