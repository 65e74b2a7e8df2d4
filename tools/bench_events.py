"""Batched propagation with events (csrc/propagate_event_kernels.h) against the plain propagation of the same arcs: Kepler arcs of
twobody_lt with zero thrust, one revolution each from periapsis, m = 10^3 .. 10^6 problems (the arcs of tools/bench_propagate.py).

    python tools/bench_events.py [--problems 1000 10000 100000 1000000] [--repeats 3] [--kinds plain never stop] [--parent FILE]

Three timings per size:
    plain   integrate_parallel without events;
    never   with the event r . r, which never fires (direction 0, stop 0): what detection costs -- one evaluation of the event
            functions per step, the state machine's registers;
    stop    with the apsis event r . v (direction 0, stop 1): every problem locates its apoapsis after half a revolution and stops in
            the step that holds it, so it integrates about half the arc.
MaxEventLocs is 1: an occurrence is 8 doubles per problem to copy back, not 64.  Times are wall-clock times of the host-pointer entry
points (allocation, copies and the Python lists of rows included), one warm-up call, then the median of `--repeats`.  One JSON line per
(size, kind).  `ms` is what a caller of integrate_parallel waits for; `ms_c` is the C entry point alone (asset_hip_propagate /
asset_hip_propagate_events: allocation, copies, the kernel), without the Python lists.  `ratio_to_plain` and `ratio_to_plain_c` are
against this run's plain times of the same size.
The plain propagation of the PARENT commit: the arcs and the plain call are those of tools/bench_propagate.py, which the parent has, so
run `python tools/bench_propagate.py --stm-max 0 > parent.jsonl` in a checkout of the parent on the same machine and pass
`--parent parent.jsonl`: every line then carries `ratio_to_parent_plain` (its `ms` against the parent's "states" `ms`)."""
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kinds", nargs="+", default=["plain", "never", "stop"], choices=["plain", "never", "stop"])
    ap.add_argument("--parent", help="output of tools/bench_propagate.py --stm-max 0 at the parent commit (JSON lines)")
    args = ap.parse_args()
    parent = {}
    if args.parent:
        for ln in open(args.parent):
            if ln.lstrip().startswith("{"):
                d = json.loads(ln)
                if d.get("kind") == "states":
                    parent[d["problems"]] = d["ms"]
    g = TwoBody().integrator("DOPRI87", 0.1)
    g.MaxEventLocs = 1
    a = vf.Arguments(10)
    never = [(a[0] * a[0] + a[1] * a[1] + a[2] * a[2], 0, 0)]
    apsis = [(a[0] * a[3] + a[1] * a[4] + a[2] * a[5], 0, 1)]
    for m in args.problems:
        rows, tfs = kepler_rows(m)
        Y, T = g._rows(rows, tfs)
        plain_ms = plain_c = None
        for kind in args.kinds:
            ev = {"plain": None, "never": never, "stop": apsis}[kind]
            if ev is None:
                fn, fc = (lambda: g.integrate_parallel(rows, tfs, details=True)), (lambda: g._propagate(Y, T, 1))
            else:
                parsed = g._events(ev)
                fn, fc = (lambda: g.integrate_parallel(rows, tfs, ev, details=True)), (lambda: g._call_events(Y, T, *parsed))

            def timed(f):
                out = f()
                ts = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    out = f()
                    ts.append(time.perf_counter() - t0)
                return out, float(np.median(ts)), float(np.min(ts))
            out, t, tmin = timed(fn)
            _, tc, _ = timed(fc)
            if kind == "plain":
                steps, status, extra = out[1], out[2], {}
                plain_ms, plain_c = 1e3 * t, 1e3 * tc
            else:
                info = out[1]
                steps, status = info["steps"], info["status"]
                extra = dict(occurrences=int(info["ev_count"].sum()), located=int(info["ev_conv"].sum()), stopped=int((info["stopped"] >= 0).sum()))
            print(json.dumps(dict(workload="twobody_lt-kepler-revolution", problems=m, kind=kind, ms=1e3 * t, ms_min=1e3 * tmin, ms_c=1e3 * tc,
                                  ratio_to_plain=(1e3 * t / plain_ms) if plain_ms else None,
                                  ratio_to_plain_c=(1e3 * tc / plain_c) if plain_c else None,
                                  ratio_to_parent_plain=(1e3 * t / parent[m]) if m in parent else None, problems_per_s=m / t,
                                  accepted=int(steps[:, 0].sum()), rejected=int(steps[:, 1].sum()),
                                  status_counts=[int((status == k).sum()) for k in range(3)], **extra)), flush=True)


if __name__ == "__main__":
    main()
