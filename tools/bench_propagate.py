"""Batched propagation (csrc/propagate_kernels.h) of Kepler arcs: twobody_lt with zero thrust, one revolution each, m = 10^3 .. 10^6
problems, without and with the state-transition matrix.

    python tools/bench_propagate.py [--problems 1000 10000 100000 1000000] [--repeats 3] [--stm-max 100000]

The problems are the same orbit family at slightly different sizes (semi-major axes spread by 10 %), sorted, so neighbouring lanes take
similar step counts.  Times are wall-clock times of the host-pointer entry points (asset_hip_propagate / asset_hip_propagate_stm): they
include the allocation, the copies and the Python lists of rows -- what a caller of Integrator.integrate_parallel waits for; the STM
is run up to `--stm-max` problems (10^6 of them are about 1 GB of matrices on the host).  One warm-up call, then the median
of `--repeats`.  One JSON line per (size, kind) with problems/s and accepted steps/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asset_asrl_amd.ode import TwoBody  # noqa: E402


def kepler_rows(m):
    scale = np.linspace(1.0, 1.1, m)
    rows = np.zeros((m, 10))
    rows[:, 0] = 0.5 * scale
    rows[:, 4], rows[:, 5] = 1.5 / np.sqrt(scale), 0.2 / np.sqrt(scale)
    a = 1.0 / (2.0 / rows[:, 0] - (rows[:, 4] ** 2 + rows[:, 5] ** 2))
    return rows, rows[:, 6] + 2.0 * np.pi * a ** 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, nargs="+", default=[1000, 10000, 100000, 1000000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stm-max", type=int, default=100000, help="largest batch that is also run with the STM")
    args = ap.parse_args()
    g = TwoBody().integrator("DOPRI87", 0.1)
    for m in args.problems:
        rows, tfs = kepler_rows(m)
        for kind in ("states", "stm"):
            if kind == "stm" and m > args.stm_max:
                continue
            fn = (lambda: g.integrate_parallel(rows, tfs, details=True)) if kind == "states" else \
                (lambda: g.integrate_stm_parallel(rows, tfs, details=True))
            fn()
            ts = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                out = fn()
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            steps, status = out[1], out[2]
            xf = np.array([r[:6] for r in out[0]]) if kind == "states" else np.array([r[0][:6] for r in out[0]])
            print(json.dumps(dict(workload="twobody_lt-kepler-revolution", problems=m, kind=kind, ms=1e3 * t, ms_min=1e3 * float(np.min(ts)),
                                  problems_per_s=m / t, accepted_steps_per_s=float(steps[:, 0].sum()) / t,
                                  accepted=int(steps[:, 0].sum()), rejected=int(steps[:, 1].sum()),
                                  status_counts=[int((status == k).sum()) for k in range(3)],
                                  closure_max=float(np.abs(xf - rows[:, :6]).max()))), flush=True)


if __name__ == "__main__":
    main()
