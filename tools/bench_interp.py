"""Times the hand-over of a trajectory between two meshes: the device trajectory table (asset_asrl_amd/interp.py) against the
host path ``Phase.refineTrajManual`` takes with ``setTrajInterpolation("linear")`` (np.interp column by column).

    python tools/bench_interp.py [--sizes 10000,100000,1000000] [--timeout 600]

Workload: `reentry`, LGL7, nb segments re-distributed onto 1.3 nb equal segments (3.9 nb + 1 query times).  One child process does
the GPU work, under a time limit of its own; it prints one JSON line per size:
  create_ms        asset_hip_traj_table_create, wall clock (host trajectory in: H2D copy, right-hand side at every node, sync)
  interp_us        stage 2 alone, device-resident, HIP events around `iters` launches on one stream
  gbytes_s, hbm    algorithmic bytes of stage 2 (trajectory + right-hand sides read once, times read, rows written) per second,
                   and that as a fraction of 8 TB/s
  host_ptr_ms      the same hand-over through host pointers (LGLInterpTable.NDdistribute: H2D times, kernel, D2H rows), wall clock
  linear_ms        Phase.refineTrajManual with "linear" on the same meshes (host only)"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(sizes, iters):
    import numpy as np
    import torch

    from asset_asrl_amd import _lib, synth
    from asset_asrl_amd.interp import LGLInterpTable, distribute_times
    from asset_asrl_amd.ode import ShuttleReentry

    torch.zeros(1, device="cuda:0")
    L = _lib.lib()
    legacy = C.c_void_p(1)                       # ASSET_HIP_STREAM_LEGACY: the stream torch's events are recorded on
    for nb in sizes:
        nn = int(1.3 * nb)
        traj = synth.make_traj("reentry", "LGL7", nb)
        N, n = traj.shape[1], 5
        t0 = time.perf_counter()
        table = LGLInterpTable("reentry", traj, "LGL7")
        create_cold = time.perf_counter() - t0
        table.close()
        t0 = time.perf_counter()
        table = LGLInterpTable("reentry", traj, "LGL7")
        create = time.perf_counter() - t0
        times = distribute_times("LGL7", [0.0, 1.0], [nn], table.T0, table.TF)
        d_t = torch.from_numpy(times).cuda()
        d_out = torch.empty((times.size, N), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def launch():
            _lib.check(L.asset_hip_traj_table_interp_device(table.handle, C.c_void_p(d_t.data_ptr()), times.size, 0,
                                                            C.c_void_p(d_out.data_ptr()), None, None, legacy), "interp_device")
        for _ in range(3):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            launch()
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / iters
        table.WarnOutOfBounds = False
        table.NDdistribute([0.0, 1.0], [nn])
        t0 = time.perf_counter()
        out = table.NDdistribute([0.0, 1.0], [nn])
        host_ptr = time.perf_counter() - t0
        assert np.array_equal(out, d_out.cpu().numpy())
        table.close()
        ph = ShuttleReentry().phase("LGL7", traj, nb)
        t0 = time.perf_counter()
        ph.refineTrajManual([0.0, 1.0], [nn])
        linear = time.perf_counter() - t0
        nbytes = 8 * (traj.shape[0] * (N + n) + times.size * (1 + N))
        print(json.dumps({"segments": nb, "new_segments": nn, "queries": int(times.size), "create_ms": round(1e3 * create, 3),
                          "create_first_ms": round(1e3 * create_cold, 3), "interp_us": round(us, 2), "algorithmic_bytes": nbytes,
                          "gbytes_s": round(nbytes / us / 1e3, 1), "hbm_fraction_of_8TBs": round(nbytes / us / 1e3 / 8000.0, 4),
                          "host_ptr_ms": round(1e3 * host_ptr, 3), "linear_ms": round(1e3 * linear, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.child:
        return child(sizes, a.iters)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--sizes", a.sizes, "--iters", str(a.iters)],
                       timeout=a.timeout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
