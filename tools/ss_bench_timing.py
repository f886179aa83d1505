"""The timing loop the state space family benchmarks (ss_student_bench.py, ss_poisson_bench.py) share."""
import time


def timed(eng, sweep, nsw):
    """nsw rounds by the wall clock, then nsw more under the engine's kernel timers"""
    sweep(max(2, nsw // 2))   # burn-in: the models grow to their size
    t0 = time.perf_counter()
    sweep(nsw)
    dt = time.perf_counter() - t0
    eng.set_kernel_timing(True)
    eng.kernel_times(reset=True)
    sweep(nsw)
    kt = eng.kernel_times(reset=True)
    eng.set_kernel_timing(False)
    return dict(ms_per_round=dt / nsw * 1e3, kernel_ms_per_round={k: round(v[0] / nsw, 4) for k, v in kt.items()},
                launches_per_round={k: v[1] / nsw for k, v in kt.items()},
                kbar=float(eng.get_states()[0].sum(1).mean()))
