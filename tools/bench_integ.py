"""Integrator-based mesh-error estimator (csrc/integ_kernels.h) on Reentry-LGL7 meshes of 10 000 / 100 000 / 1 000 000 segments, with
the de Boor estimator on the same mesh beside it.

    python tools/bench_integ.py [--segments 10000 100000 1000000] [--repeats 5] [--width 0.1]

Every segment is `--width` wide in Reentry's units (random node rows, asset_asrl_amd.synth), so the work per node interval does not
depend on the mesh size.  Times are wall-clock times of the host-pointer entry points (asset_hip_mesh_error_integrator /
asset_hip_mesh_error_deboor): they include the allocation, the copy of the trajectory to the device and of the results back -- what a
caller of Phase.checkMesh waits for.  One warm-up call, then the median of `--repeats`.  One JSON line per size."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asset_asrl_amd import mesh, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=float, default=0.1)
    args = ap.parse_args()
    for nseg in args.segments:
        traj = synth.make_traj("reentry", "LGL7", nseg, seed=11, T=args.width * nseg)

        def timed(fn):
            fn()
            ts = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                out = fn()
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts)), float(np.min(ts)), out
        t_int, t_int_min, out = timed(lambda: mesh.mesh_error_integrator("reentry", "LGL7", traj, details=True))
        t_db, t_db_min, _ = timed(lambda: mesh.mesh_error_deboor("reentry", "LGL7", traj))
        steps, status = out[6], out[7]
        acc, rej = int(steps[:, 0].sum()), int(steps[:, 1].sum())
        print(json.dumps(dict(workload="reentry-LGL7", segments=nseg, intervals=int(steps.shape[0]), segment_width=args.width,
                              integrator_ms=1e3 * t_int, integrator_ms_min=1e3 * t_int_min, deboor_ms=1e3 * t_db, deboor_ms_min=1e3 * t_db_min,
                              accepted=acc, rejected=rej, max_steps_of_an_interval=int(steps.sum(axis=1).max()),
                              status_counts=[int((status == k).sum()) for k in range(3)],
                              rhs_evals_per_s=13.0 * (acc + rej) / t_int)), flush=True)


if __name__ == "__main__":
    main()
