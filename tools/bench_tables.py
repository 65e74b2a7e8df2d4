"""Device time of tabulated data in generated code (``vf.InterpTable2D`` / ``vf.InterpTable3D``) against the
polynomial the table was sampled from -- the same function without a look-up and without loads:

  * the function kernel, 10^6 applications at random points of the table's range: a 2-D cubic table (64 x 64) and a 3-D cubic table
    (16 x 16 x 16), value + Jacobian + adjoint gradient + adjoint Hessian;
  * the defect evaluation of the table ODE of tests/interp_nd_cases.py (a 2-D cubic and a 3-D linear table) at LGL7 x 10 000 segments;
  * each table form in both layouts of a cubic table (vf.functions.TABLE_LAYOUT: "record" / "planes").

Device events around `iters` launches after a warm-up (the library's time_device), the forms of a pair alternating, `rounds` times;
reported: the median per form, the spread over the rounds, time per application / per evaluation, the ratio table / twin.  The outputs
of every form of a pair are compared at the timed size before anything is timed.

  python tools/bench_tables.py                 # on the GPU box; prints one JSON line
  python tools/bench_tables.py --prebuild      # without a device: compile every module into the cache
"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # noqa: F401   (before the project's library, as tools/time_phase_functions.py: the process then has one HIP runtime, torch's)

ROOT =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import interp_nd_cases as cases  # noqa: E402
from helpers import Workload, rel_err  # noqa: E402

from asset_asrl_amd import jit, vf  # noqa: E402
from asset_asrl_amd.evaluator import JAC_ADJGRAD_HESS, DefectEvaluator  # noqa: E402

NAPP, NSEG = 1000000, 10000
LAYOUTS = ("record", "planes")


class layout:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.old, vf.functions.TABLE_LAYOUT = vf.functions.TABLE_LAYOUT, self.name

    def __exit__(self, *exc):
        vf.functions.TABLE_LAYOUT = self.old


def bench_table(poly, sizes):
    """A cubic table of the polynomial `poly` on evenly spaced axes of the given sizes over the range of its test grid."""
    axes = [np.linspace(a[0], a[-1], n) for a, n in zip(cases.GRID[poly], sizes)]
    if len(axes) == 2:
        data = np.array([[cases.poly_np(poly, (x, y)) for x in axes[0]] for y in axes[1]])
        return vf.InterpTable2D(*axes, data)
    data = np.array([[[cases.poly_np(poly, (x, y, z)) for z in axes[2]] for y in axes[1]] for x in axes[0]])
    return vf.InterpTable3D(*axes, data)


def function_forms(poly, sizes):
    """[(label, vf function, device name)]: the table in both layouts, then the polynomial twin."""
    tab = bench_table(poly, sizes)
    d = len(sizes)
    forms = []
    for lay in LAYOUTS:
        with layout(lay):
            forms.append((f"table, {lay}", tab.vf(), f"tables_bench_{poly}_{lay}"))
    a = vf.Arguments(d)
    forms.append(("polynomial twin", vf.stack([cases.poly_vf(poly, a.tolist())]), f"tables_bench_{poly}_twin"))
    return tab, forms


def ode_forms():
    forms = []
    for lay in LAYOUTS:
        with layout(lay):
            cases.make_ode.cache_clear()
            ode = cases.make_ode(False)
            ode.derivatives()                     # (the expression is built under the layout; the module is named by its body)
            forms.append((f"table, {lay}", ode))
    cases.make_ode.cache_clear()
    forms.append(("polynomial twin", cases.make_ode(True)))
    return forms


def time_pair(evs, X, L, rounds, iters):
    """evs: [(label, evaluator)] -> {label: {...}}; the forms alternate inside every round."""
    dev = torch.device("cuda:0")
    Xd, Ld = torch.from_numpy(X).to(dev), torch.from_numpy(L).to(dev)
    bufs, ms = {}, {k: [] for k, _ in evs}
    for k, ev in evs:
        bufs[k] = (torch.empty(ev.nseg * ev.OR, dtype=torch.float64, device=dev), torch.empty(ev.nseg * ev.IR, dtype=torch.float64, device=dev),
                   torch.empty(ev.nseg * ev.KSTRIDE, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, ev in evs:
            ms[k].append(ev.time_device(JAC_ADJGRAD_HESS, Xd, Ld, *bufs[k], warmup=5, iters=iters))
    n = evs[0][1].nseg
    out = {k: {"ms_median": round(float(np.median(v)), 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5),
               "ns_per_application": round(float(np.median(v)) * 1e6 / n, 3)} for k, v in ms.items()}
    twin = out["polynomial twin"]["ms_median"]
    for k in out:
        out[k]["ratio_to_twin"] = round(out[k]["ms_median"] / twin, 3)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--prebuild", action="store_true", help="compile every module into the cache (no device needed)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--napp", type=int, default=NAPP)
    ap.add_argument("--nseg", type=int, default=NSEG)
    a = ap.parse_args(argv)
    funcs = [("2-D cubic 64x64", "cubic2", (64, 64)), ("3-D cubic 16x16x16", "cubic3", (16, 16, 16))]
    if a.prebuild:
        jit.compile_only_mode(True)
        for _, poly, sizes in funcs:
            for _, f, name in function_forms(poly, sizes)[1]:
                jit.ensure_function(f, name)
        for _, ode in ode_forms():
            jit.ensure_kernel(ode, "LGL7", False)
        jit.compile_only_mode(False)
        print("bench_tables: modules compiled")
        return 0
    from asset_asrl_amd import _lib
    from asset_asrl_amd.pathfuncs import FunctionEvaluator
    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise RuntimeError("bench_tables: no HIP device visible")
    torch.cuda.set_device(0)
    out = {"applications": a.napp, "segments": a.nseg, "rounds": a.rounds, "iters": a.iters, "kind": "JAC_ADJGRAD_HESS"}
    rng = np.random.default_rng(0)
    for label, poly, sizes in funcs:
        tab, forms = function_forms(poly, sizes)
        d = len(sizes)
        X = np.column_stack([rng.uniform(ax[0], ax[-1], a.napp) for ax in (t.ts for t in tab._axes)]).ravel()
        L = rng.uniform(-1, 1, a.napp)
        vindex = np.arange(a.napp * d, dtype=np.int32).reshape(a.napp, d)
        cindex = np.arange(a.napp, dtype=np.int32).reshape(a.napp, 1)
        evs = [(k, FunctionEvaluator(f, name, vindex, cindex, a.napp * d, a.napp)) for k, f, name in forms]
        ref = evs[-1][1].eval(JAC_ADJGRAD_HESS, X, L)
        agree = {k: max(rel_err(x, y) for x, y in zip(ev.eval(JAC_ADJGRAD_HESS, X, L), ref)) for k, ev in evs[:-1]}
        out[label] = dict(time_pair(evs, X, L, a.rounds, a.iters), entries=tab.entries, rel_err_against_twin=agree)
        for _, ev in evs:
            ev.close()
    w = Workload("interp_nd", "LGL7", a.nseg, False, sizes=(2, 1, 0))
    evs = [(k, DefectEvaluator(jit.ensure_kernel(ode, "LGL7", False), "LGL7", False, w.vindex, w.cindex, w.n_primal, w.n_equal)) for k, ode in ode_forms()]
    ref = evs[-1][1].eval(JAC_ADJGRAD_HESS, w.X, w.L)
    agree = {k: max(rel_err(x, y) for x, y in zip(ev.eval(JAC_ADJGRAD_HESS, w.X, w.L), ref)) for k, ev in evs[:-1]}
    res = time_pair(evs, w.X, w.L, a.rounds, a.iters)
    for k in res:
        res[k]["us_per_evaluation"] = round(res[k].pop("ns_per_application") * a.nseg / 1e3, 2)
    out[f"table ODE, LGL7 x {a.nseg} segments"] = dict(res, rel_err_against_twin=agree)
    for _, ev in evs:
        ev.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
