"""Propagation with events AND the state-transition matrix in one call (csrc/propagate_event_stm_kernels.h,
asset_hip_propagate_events_stm) against what a caller did before it existed: asset_hip_propagate_events, then asset_hip_propagate_stm to
the end times that call returned -- two propagations.  Kepler arcs of twobody_lt with zero thrust, one revolution each from periapsis,
m = 10^3 .. 10^6 problems ordered by size and hence by step count (the arcs of tools/bench_propagate.py).

    python tools/bench_event_stm.py [--problems 1000 10000 100000 1000000] [--repeats 5] [--configs never stop0 stop1]

Configurations: `stop0`, the apsis event r . v (direction 0) with stop = 0 -- every problem locates its apoapsis and runs on to tf;
`stop1`, the same event with stop = 1 -- every problem stops in the step that holds its apoapsis, about half the arc; `never`, the event
r . r, which never fires (stop = 0, no occurrences).  Each with and without ev_jac.  MaxEventLocs is 2.  Per (size, configuration) one
JSON line with, all in ms and all wall-clock times of the host-pointer C entry points (allocation, copies, kernels; no Python lists),
one warm-up call and then the median of `--repeats`:
    one_call, one_call_ev_jac   asset_hip_propagate_events_stm without and with ev_jac;
    two_calls                   asset_hip_propagate_events, then asset_hip_propagate_stm to its t_end (`events` and `stm_to_t_end` apart);
    stm_alone                   asset_hip_propagate_stm to tf;
    ratio_one_to_two, ratio_one_ev_jac_to_two, ratio_one_to_stm_alone.
The end states of the one call and of the events call are compared bit for bit on the way (`state_bits_equal`), and the largest
difference between the one call's Jacobian and the second propagation's is reported (`jac_max_diff`: two different step sequences)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asset_asrl_amd import vf  # noqa: E402
from asset_asrl_amd.ode import TwoBody  # noqa: E402
from bench_propagate import kepler_rows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, nargs="+", default=[1000, 10000, 100000, 1000000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", nargs="+", default=["never", "stop0", "stop1"], choices=["never", "stop0", "stop1"])
    args = ap.parse_args()
    g = TwoBody().integrator("DOPRI87", 0.1)
    g.MaxEventLocs = 2
    a = vf.Arguments(10)
    rr, rv = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], a[0] * a[3] + a[1] * a[4] + a[2] * a[5]
    events = {"never": [(rr, 0, 0)], "stop0": [(rv, 0, 0)], "stop1": [(rv, 0, 1)]}

    def timed(f):
        out = f()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            out = f()
            ts.append(time.perf_counter() - t0)
        return out, 1e3 * float(np.median(ts))

    def stm_to(Y, T):
        m, n, N = Y.shape[0], g.xv, Y.shape[1]
        xf, jac = np.empty((m, 1, n)), np.empty((m, n, N + 1))
        steps, status = np.empty((m, 2), dtype=np.int32), np.empty(m, dtype=np.int32)
        g._call("asset_hip_propagate_stm", g._device_name, Y, T, None, xf, jac, steps, status)
        return jac

    for m in args.problems:
        rows, tfs = kepler_rows(m)
        Y, T = g._rows(rows, tfs)
        _, stm_alone = timed(lambda: stm_to(Y, T))
        for cfg in args.configs:
            parsed = g._events(events[cfg])
            one, t_one = timed(lambda: g._call_events(Y, T, *parsed, stm=True))
            _, t_one_ej = timed(lambda: g._call_events(Y, T, *parsed, stm=True, event_jacs=True))
            ev, t_ev = timed(lambda: g._call_events(Y, T, *parsed))
            t_end = np.ascontiguousarray(ev["t_end"])
            jac2, t_stm = timed(lambda: stm_to(Y, t_end))
            print(json.dumps(dict(workload="twobody_lt-kepler-revolution", problems=m, config=cfg, one_call=t_one, one_call_ev_jac=t_one_ej,
                                  two_calls=t_ev + t_stm, events=t_ev, stm_to_t_end=t_stm, stm_alone=stm_alone,
                                  ratio_one_to_two=t_one / (t_ev + t_stm), ratio_one_ev_jac_to_two=t_one_ej / (t_ev + t_stm),
                                  ratio_one_to_stm_alone=t_one / stm_alone,
                                  state_bits_equal=bool(np.array_equal(one["xf"].view(np.uint64), ev["xf"].view(np.uint64))
                                                        and np.array_equal(one["t_end"], ev["t_end"])),
                                  jac_max_diff=float(np.abs(one["jac"] - jac2).max()),
                                  occurrences=int(one["ev_count"].sum()), stopped=int((one["stopped"] >= 0).sum()),
                                  accepted=int(one["steps"][:, 0].sum()), rejected=int(one["steps"][:, 1].sum()),
                                  status_counts=[int((one["status"] == k).sum()) for k in range(3)])), flush=True)


if __name__ == "__main__":
    main()
