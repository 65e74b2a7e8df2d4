"""``astro.KeplerPropagator`` on the device, and what a root costs inside a transcription.

  * value + Jacobian of the propagator as a plain function, 10^3 .. 10^6 Kepler arcs of tools/bench_propagate.py's family (one
    revolution each), device-resident (the library's time_device: device events around `iters` launches after a warm-up), median of
    5 rounds (of 3 at 10^6); beside it ``integrate_stm_parallel`` of twobody_lt on the same arcs -- the wall-clock time of the call a
    caller has to make without the propagator to get the same numbers (end state and STM) -- the ratio, and the mean number of passes
    of the root's loop per arc (the host's iteration on a sample of the arcs: the device runs the same rule);
  * ``--transcription``: the twin pair of tests/root_cases.py (an ODE written with ``ScalarRootFinder(s^2 - q, 30, 1e-15)`` against the
    same ODE written with ``sqrt(q)``) at LGL7 x 10 000 segments, value + Jacobian + adjoint gradient + adjoint Hessian, the two forms
    alternating, with OPS_FJGH of both and the launch form each got;
  * ``--resources``: registers and private-segment (scratch) bytes of every kernel of the cached modules of the pair and of the
    propagator, as the compiler wrote them into the code objects (llvm-readelf --notes; no device needed).

  python tools/bench_kepler.py [--problems 1000 10000 100000 1000000] [--stm-max 1000000] [--fraction 1.0]    # one JSON line per size
  python tools/bench_kepler.py --transcription
  python tools/bench_kepler.py --resources
  python tools/bench_kepler.py --prebuild      # without a device: compile every module into the cache
"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FN_NAME = "bench_kepler_prop"


def kepler_inputs(m, fraction=1.0):
    """rows, end times and propagator inputs of the family; `fraction` of a revolution (after exactly one the guess sqrt(mu) dt alpha
    IS the root and the loop leaves at its first test, so a part of a revolution is what shows the loop's cost)"""
    from bench_propagate import kepler_rows
    rows, tfs = kepler_rows(m)
    tfs = rows[:, 6] + fraction * (tfs - rows[:, 6])
    return rows, tfs, np.column_stack([rows[:, :6], tfs - rows[:, 6]])


def mean_passes(kp, Y, sample=200):
    from asset_asrl_amd.vf.ir import ROOTS, evaluate, topo_order
    node = [n for n in topo_order(kp.outs) if n.op == "root"][0]
    total = 0
    idx = np.linspace(0, len(Y) - 1, min(sample, len(Y))).astype(int)
    for i in idx:
        a = evaluate(list(node.args), Y[i])
        total += ROOTS[node.value].iterate(a[0], a[1:])[1]
    return total / len(idx)


def propagator_rounds(args):
    import torch
    from asset_asrl_amd import astro
    from asset_asrl_amd.evaluator import JAC
    from asset_asrl_amd.ode import TwoBody
    from asset_asrl_amd.pathfuncs import FunctionEvaluator
    dev = torch.device("cuda:0")
    kp = astro.KeplerPropagator(1.0)
    g = TwoBody().integrator("DOPRI87", 0.1)
    for m in args.problems:
        rows, tfs, Y = kepler_inputs(m, args.fraction)
        vindex = np.arange(m * 7, dtype=np.int32).reshape(m, 7)
        cindex = np.arange(m * 6, dtype=np.int32).reshape(m, 6)
        ev = FunctionEvaluator(kp, FN_NAME, vindex, cindex, m * 7, m * 6)
        fx, _, kkt = ev.eval(JAC, Y.ravel().copy(), None)
        closure = float(np.abs(np.asarray(fx).reshape(m, 6) - rows[:, :6]).max()) if args.fraction == 1.0 else None   # one revolution: back at the start
        Xd, Ld = torch.from_numpy(Y.ravel().copy()).to(dev), torch.zeros(m * 6, dtype=torch.float64, device=dev)
        bufs = (torch.empty(m * ev.OR, dtype=torch.float64, device=dev), torch.empty(m * ev.IR, dtype=torch.float64, device=dev),
                torch.empty(m * ev.KSTRIDE, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        rounds = 3 if m >= 1000000 else 5
        ms = [ev.time_device(JAC, Xd, Ld, *bufs, warmup=3, iters=args.iters) for _ in range(rounds)]
        out = dict(workload="kepler-revolution", fraction=args.fraction, problems=m, propagator_ms=float(np.median(ms)), propagator_ms_min=min(ms), propagator_ms_max=max(ms),
                   closure_max=closure, mean_passes=mean_passes(kp, Y))
        ev.close()
        if m <= args.stm_max:
            g.integrate_stm_parallel(rows, tfs, details=True)
            ts = []
            for _ in range(rounds):
                t0 = time.perf_counter()
                res = g.integrate_stm_parallel(rows, tfs, details=True)
                ts.append(1e3 * (time.perf_counter() - t0))
            xf = np.array([r[0][:6] for r in res[0][:1000]])
            out.update(integrate_stm_ms=float(np.median(ts)), integrate_stm_ms_min=min(ts), integrate_stm_ms_max=max(ts),
                       ratio=float(np.median(ts) / np.median(ms)), agreement_max=float(np.abs(xf - np.asarray(fx).reshape(m, 6)[:1000]).max()))
        print(json.dumps(out), flush=True)


def transcription(args):
    import torch
    import root_cases as cases
    from asset_asrl_amd import jit
    from asset_asrl_amd.evaluator import JAC_ADJGRAD_HESS, DefectEvaluator
    from helpers import Workload, rel_err
    dev = torch.device("cuda:0")
    w = Workload("root_ode", "LGL7", args.nseg, False, sizes=(2, 1, 0))
    forms = [("root", cases.make_ode(False)), ("closed form", cases.make_ode(True))]
    evs = [(k, DefectEvaluator(jit.ensure_kernel(o, "LGL7", False), "LGL7", False, w.vindex, w.cindex, w.n_primal, w.n_equal)) for k, o in forms]
    a, b = (ev.eval(JAC_ADJGRAD_HESS, w.X, w.L) for _, ev in evs)
    out = {"segments": args.nseg, "mode": "LGL7", "rel_err_root_against_closed_form": max(rel_err(x, y) for x, y in zip(a, b))}
    Xd, Ld = torch.from_numpy(w.X).to(dev), torch.from_numpy(w.L).to(dev)
    ms = {k: [] for k, _ in evs}
    bufs = {k: (torch.empty(ev.nseg * ev.OR, dtype=torch.float64, device=dev), torch.empty(ev.nseg * ev.IR, dtype=torch.float64, device=dev),
                torch.empty(ev.nseg * ev.KSTRIDE, dtype=torch.float64, device=dev)) for k, ev in evs}
    torch.cuda.synchronize()
    for _ in range(5):
        for k, ev in evs:
            ms[k].append(ev.time_device(JAC_ADJGRAD_HESS, Xd, Ld, *bufs[k], warmup=5, iters=args.iters))
    for (k, ev), (_, ode) in zip(evs, forms):
        out[k] = dict(us_median=1e3 * float(np.median(ms[k])), us_min=1e3 * min(ms[k]), us_max=1e3 * max(ms[k]),
                      ops_fjgh=ode.derivatives().stats()["ops_fjgh"], launch_plan=ev.launch_plan(JAC_ADJGRAD_HESS))
        ev.close()
    out["ratio"] = out["root"]["us_median"] / out["closed form"]["us_median"]
    print(json.dumps(out, default=str))


def module_resources(path):
    """[(kernel, vgprs, agprs, sgprs, private segment bytes)] of one cached module, from the notes of its code object"""
    from isa_dpp_hazard import LLVM, RTC_MAGIC
    data = open(path, "rb").read()
    pos = len(RTC_MAGIC)
    nl = data.index(b"\n", pos)
    for _ in range(int(data[pos:nl]) + 1):
        pos = nl + 1
        nl = data.index(b"\n", pos)
    size = int(data[pos:nl])
    with tempfile.TemporaryDirectory() as td:
        co = os.path.join(td, "co")
        open(co, "wb").write(data[nl + 1:nl + 1 + size])
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    out = []
    for blk in notes.split("- .agpr_count:")[1:]:
        get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out.append((name[:60], get("vgpr_count"), int(blk.split()[0]), get("sgpr_count"), get("private_segment_fixed_size")))
    return out


def resources():
    import root_cases as cases
    from asset_asrl_amd import astro, jit
    jit.compile_only_mode(True)
    dirs = {"root ODE, LGL7": jit.ensure_kernel(cases.make_ode(False), "LGL7", False), "closed form, LGL7": jit.ensure_kernel(cases.make_ode(True), "LGL7", False),
            "propagator, function": jit.ensure_function(astro.KeplerPropagator(1.0), FN_NAME)}
    for label, name in dirs.items():
        for mod in sorted(glob.glob(os.path.join(jit.JIT_DIR, name, "module_*.rtc"))):
            if label.endswith("LGL7") and "lgl7_0" not in os.path.basename(mod):
                continue
            rows = module_resources(mod)
            worst = max(rows, key=lambda r: (r[4], r[1] + r[2]))
            print(json.dumps(dict(module=label, kernels=len(rows), max_vgprs=max(r[1] for r in rows), max_agprs=max(r[2] for r in rows),
                                  max_private_segment_bytes=max(r[4] for r in rows), largest=worst)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, nargs="+", default=[1000, 10000, 100000, 1000000])
    ap.add_argument("--stm-max", type=int, default=1000000, help="largest batch that is also integrated with the STM")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fraction", type=float, default=1.0, help="part of a revolution each arc covers")
    ap.add_argument("--nseg", type=int, default=10000)
    ap.add_argument("--transcription", action="store_true")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--prebuild", action="store_true")
    a = ap.parse_args(argv)
    if a.resources:
        return resources()
    if a.prebuild:
        import root_cases as cases
        from asset_asrl_amd import astro, jit
        from asset_asrl_amd.ode import TwoBody
        jit.compile_only_mode(True)
        jit.ensure_function(astro.KeplerPropagator(1.0), FN_NAME)
        for twin in (False, True):
            jit.ensure_kernel(cases.make_ode(twin), "LGL7", False)
        jit.ensure_kernel(TwoBody(), "LGL3", False)
        print("bench_kepler: modules compiled")
        return 0
    import torch  # noqa: F401   (before the project's library: the process then has one HIP runtime, torch's)
    from asset_asrl_amd import _lib
    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise RuntimeError("bench_kepler: no HIP device visible")
    torch.cuda.set_device(0)
    return transcription(a) if a.transcription else propagator_rounds(a)


if __name__ == "__main__":
    sys.exit(main())
