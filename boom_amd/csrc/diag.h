// The diagnostic builds' cycle stamps, all in one place (never in the product: every macro here
// is empty unless its -D flag is given; the Makefile's tools/build/libboomamd_*stamps*.so targets make the builds, tools/
// ss_phase_profile.py and tools/phase_profile.py read them).
//
//   flag                      macro            what the 8 slots time                    clock
//   -DBA_STAMPS               STAMP(i)         phases of one SSVS sweep (ssvs_sweep_body.h)   core
//   -DBA_STAMPS -DBA_STAMPS2  SUBSTAMP(c, i)   the inside of a proposal batch: 0 uniform +
//                                              log, 1 classify, 2 V gather, 3 V solve, 4 A
//                                              gather, 5 A solve, 6 epilogue, 7 outside       core
//   -DBA_STAMPS -DBA_STAMPS3  TSTAMP(c, i)     the master's pieces of a forked sweep: 0
//                                              commit, 1 sweep-start copy, 2 fork, 3 swap
//                                              proposal, 4 sigma, 5 normals, 6 back
//                                              substitution, 7 everything else                core
//   -DBA_STAMPS -DBA_STAMPS4  HSTAMP(c, i)     helper wave 1: 0 shuffle uniforms, 1 matching
//                                              rounds, 2 links, 3 walks, 4 table walk, 5
//                                              waiting for commands, 6 its share of proposal
//                                              rounds, 7 other                                core
//   -DBA_STAMPS -DBA_STAMPS5  FSTAMP(c, i)     a model rebuild (refactor and its site): 0
//                                              gathers, prior sum, row shift, r and c, 1 the
//                                              inserted row, 2 the column loop and the log
//                                              determinants, 3 w and the model's value, 4
//                                              publish / restore; 5 and 6 are COUNTS (rebuilds,
//                                              columns kept); 7 everything else               core
//   -DBA_STAMPS -DBA_STAMPS6  MSTAMP(c, i)     the master's "everything else" of TSTAMP, split: 0
//                                              waiting for a table walk it did not fork, 1
//                                              waiting at the join, 2 its share of the fill
//                                              rounds, 3 events (rebuild or slot switch); 4, 5
//                                              and 6 are COUNTS (sweeps with a stop, walks
//                                              forked other than a sweep's first, those rolled
//                                              back); 7 everything else                       core
//   -DBA_STAMPS -DBA_STAMPS7  XSTAMP(c, i)     the master's "everything else" of MSTAMP, itemised:
//                                              0 a join's bookkeeping (behind the barrier), 1 the
//                                              loop top (a phase's end to the next phase's first
//                                              line: the loop's condition, the event test, the
//                                              phase dispatch), 2 PH_FLIPS bookkeeping around a
//                                              walk or a stop, 3 batch-mode rounds, 4 PH_BEGIN's
//                                              decisions ahead of the sweep-start copy, 5 a sweep
//                                              start that does not fork (the all-threads shuffle);
//                                              6 is a COUNT (passes of the loop); 7 what the other
//                                              sets name (TSTAMP's pieces, waits, fills, events)   core
//   -DBA_PSTAMPS              PSTAMP(i)        the sweep kernel's prologue (absolute stamps)  core
//   -DBA_KSTAMPS              KSTAMP(i)        the local-level Kalman kernel's phases, and
//                             SSTAMP(i)        the structural kernels' (chain 0 prints)       core
//   -DBA_RSTAMPS              RSTAMP(i)        the bsts round kernel's phases per chain and
//                                              wave, summed over the launch's rounds          100 MHz
//
// The sites declare their own accumulators (`ph[8]` + `last`, under the same flag); the macros
// only add "now - last" to slot i and move `last` on.
#pragma once

#define BA_STAMP_ADD(ph, last, i, now, T) do { const long long t_ = (long long)(now); (ph)[i] += (T)(t_ - (last)); (last) = t_; } while (0)
#define BA_STAMP_OFF do { } while (0)
#define BA_CORE_CLOCK __builtin_readcyclecounter()

struct StampCtx { long long last; double ph[8]; };

#ifdef BA_STAMPS
#define STAMP_DECL long long st_last = (long long)BA_CORE_CLOCK; double st_ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define STAMP(i) BA_STAMP_ADD(st_ph, st_last, i, BA_CORE_CLOCK, double)
#else
#define STAMP_DECL BA_STAMP_OFF
#define STAMP(i) BA_STAMP_OFF
#endif
#if defined(BA_STAMPS) && defined(BA_STAMPS2)
#define SUBSTAMP(c, i) BA_STAMP_ADD((c).ph, (c).last, i, BA_CORE_CLOCK, double)
#else
#define SUBSTAMP(c, i) BA_STAMP_OFF
#endif
#if defined(BA_STAMPS) && defined(BA_STAMPS3)
#define TSTAMP(c, i) BA_STAMP_ADD((c).ph, (c).last, i, BA_CORE_CLOCK, double)
#else
#define TSTAMP(c, i) BA_STAMP_OFF
#endif
#if defined(BA_STAMPS) && defined(BA_STAMPS4)
#define HSTAMP(c, i) BA_STAMP_ADD((c).ph, (c).last, i, BA_CORE_CLOCK, double)
#else
#define HSTAMP(c, i) BA_STAMP_OFF
#endif
#if defined(BA_STAMPS) && defined(BA_STAMPS5)
#define FSTAMP(c, i) BA_STAMP_ADD((c).ph, (c).last, i, BA_CORE_CLOCK, double)
#define FCOUNT(c, i, x) do { (c).ph[i] += (double)(x); } while (0)
#else
#define FSTAMP(c, i) BA_STAMP_OFF
#define FCOUNT(c, i, x) BA_STAMP_OFF
#endif
#if defined(BA_STAMPS) && defined(BA_STAMPS6)
#define MSTAMP(c, i) BA_STAMP_ADD((c).ph, (c).last, i, BA_CORE_CLOCK, double)
#define MCOUNT(c, i, x) do { (c).ph[i] += (double)(x); } while (0)
#else
#define MSTAMP(c, i) BA_STAMP_OFF
#define MCOUNT(c, i, x) BA_STAMP_OFF
#endif
#if defined(BA_STAMPS) && defined(BA_STAMPS7)
#define XSTAMP(c, i) BA_STAMP_ADD((c).ph, (c).last, i, BA_CORE_CLOCK, double)
#define XCOUNT(c, i, x) do { (c).ph[i] += (double)(x); } while (0)
#else
#define XSTAMP(c, i) BA_STAMP_OFF
#define XCOUNT(c, i, x) BA_STAMP_OFF
#endif
#ifdef BA_PSTAMPS
#define PSTAMP(i) pst[i] = (long long)BA_CORE_CLOCK
#else
#define PSTAMP(i) BA_STAMP_OFF
#endif
#ifdef BA_KSTAMPS
#define KSTAMP(i) BA_STAMP_ADD(kph, klast, i, BA_CORE_CLOCK, long long)
#define SSTAMP(i) BA_STAMP_ADD(kph, klast, i, BA_CORE_CLOCK, long long)
#else
#define KSTAMP(i) BA_STAMP_OFF
#define SSTAMP(i) BA_STAMP_OFF
#endif
#ifdef BA_RSTAMPS
#define RSTAMP(i) BA_STAMP_ADD(rph, rlast, i, wall_clock64(), long long)
#else
#define RSTAMP(i) BA_STAMP_OFF
#endif
