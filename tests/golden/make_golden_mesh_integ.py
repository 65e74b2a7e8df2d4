"""Generate tests/golden/mesh_integ/mesh_error_integ.npz (run once, here; commit the file): the end state of every node interval's initial-value
problem in 50-digit arithmetic, for the integrator-based mesh-error estimate (csrc/integ_kernels.h; tests/integ_checker.py).

`x_exact[i]` solves  x' = f(x, t, u(t), p),  x(t_i) = row i,  to t_(i+1): u(t) the block's degree cs - 1 polynomial through its nodes' controls
(Cardinal_UPolyPower_Weights of tests/golden/lgl_tables.json, evaluated in mpf), or the start row's controls held (no controls,
BlockConstant); p the start row's.  The right-hand sides are make_golden_mesh.ODES in mpf.  Method: Gragg's modified midpoint rule with
2, 4, .., 2 k substeps over the whole interval, extrapolated in h^2 (Bulirsch-Stoer; k = DEPTH) -- not the tableau under test, and not
mpmath.odefun, which took over ten minutes for six Reentry intervals.  The reference's own convergence is ASSERTED: the extrapolation to
depth k and the one to depth k - 2 (the same rule at a lower resolution and order) agree to < 1e-25 (relative to max(1, |x|)) on every
interval of every case.  Nothing of asset_asrl_amd/csrc is used.

Per case the file also holds what tests/integ_checker.py's bounds need: `steps64` (accepted, rejected of the float64 restatement, right-hand
side = the oracle's float64 ``OdeStruct.f``), `err64` = |restatement - x_exact|, the longdouble restatement `xld` (as a float64 pair) and
`d64` = |float64 restatement - longdouble restatement|.  Asserted here: every interval |H| <= 0.2, every restatement status 0, and for the
adaptive cases the quarter-of-the-bound condition err64 <= accepted64 AbsTol.

Usage:  python tests/golden/make_golden_mesh_integ.py
"""
from __future__ import annotations

import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import integ_checker as gck  # noqa: E402
import interp_checker as ick  # noqa: E402
from make_golden_mesh import ODES, M  # noqa: E402

mp.mp.dps = 50
DEPTH = 26
MODE_CS = ick.MODE_CS
_TABLES = json.load(open(os.path.join(HERE, "lgl_tables.json")))["tables"]
CONVERGED = mp.mpf(10) ** -25


def _specs():
    out = []

    def add(ode, mode, blocked, nb, dt, tag="", reverse=False, **opts):
        name = f"{ode}_{mode}{'_blocked' if blocked else ''}_{nb}{tag}"
        out.append(dict(name=name, ode=ode, mode=mode, blocked=bool(blocked), nb=nb, dt=dt, reverse=reverse, seed=900 + len(out),
                        sizes=list(ODES[ode][1]), options=opts))
    add("reentry", "Trapezoidal", False, 24, 0.08)
    add("reentry", "LGL3", False, 20, 0.08)
    add("reentry", "LGL5", False, 12, 0.16)
    add("reentry", "LGL7", False, 10, 0.2)
    add("reentry", "LGL5", True, 10, 0.16)
    add("vanderpol", "LGL7", False, 6, 0.2)
    add("shape_1_0_0", "LGL5", False, 8, 0.16)
    add("shape_5_3_2", "LGL3", False, 12, 0.08)
    add("twobody_lt", "LGL5", False, 10, 0.16)
    add("twobody_lt", "Trapezoidal", True, 10, 0.08)
    add("reentry", "LGL7", False, 6, 0.2, tag="_reversed", reverse=True)
    # fixed steps: def_step 0.1 gives numsteps = 1 or 2, so the count numsteps + 1 holds (h = 0.9 H / numsteps needs ceil(numsteps / 0.9)
    # steps, which is numsteps + 1 up to numsteps = 8)
    add("reentry", "LGL5", False, 8, 0.16, tag="_fixed", adaptive=False, def_step=0.1, min_step=1e-5, max_step=1000.0)
    return out


SPECS = _specs()


def make_traj(spec):
    ode, mode, nb = spec["ode"], spec["mode"], spec["nb"]
    named = ode in ("reentry", "twobody_lt")
    traj = ick.ragged_traj(ode, mode, nb, seed=spec["seed"], T=spec["dt"] * nb, sizes=None if named else tuple(spec["sizes"]), spread=2.0)
    return traj[::-1].copy() if spec["reverse"] else traj


def control_mp(traj, mode, xv, uv, blk, t):
    cs = MODE_CS[mode]
    K = cs - 1
    Uw = _TABLES[str(cs)]["Cardinal_UPolyPower_Weights"]
    rows = traj[blk * K:blk * K + cs]
    tb0 = mp.mpf(float(rows[0, xv]))
    s = (t - tb0) / (mp.mpf(float(rows[-1, xv])) - tb0)
    ups = [sum((mp.mpf(float(w)) * s ** (cs - 1 - k) for k, w in enumerate(Uw[i])), mp.mpf(0)) for i in range(cs)]
    return [sum((mp.mpf(float(rows[i, xv + 1 + j])) * ups[i] for i in range(cs)), mp.mpf(0)) for j in range(uv)]


def solve_interval(spec, traj, i):
    """(x(t_(i+1)) to depth DEPTH, the same to depth DEPTH - 2), lists of mpf."""
    ode, mode = spec["ode"], spec["mode"]
    xv, uv, pv = spec["sizes"]
    f_ode = ODES[ode][0]
    K = MODE_CS[mode] - 1
    held = uv == 0 or spec["blocked"]
    row = [mp.mpf(float(v)) for v in traj[i]]
    t0, tf = row[xv], mp.mpf(float(traj[i + 1, xv]))

    def f(x, t):
        u = row[xv + 1:xv + 1 + uv] if held else control_mp(traj, mode, xv, uv, i // K, t)
        return f_ode(list(x) + [t] + list(u) + row[xv + 1 + uv:], M)

    x0, H = row[:xv], tf - t0
    T = []
    for j in range(DEPTH):
        n = 2 * (j + 1)
        h = H / n
        z0, z1 = x0, [a + h * b for a, b in zip(x0, f(x0, t0))]
        for m in range(1, n):
            fz = f(z1, t0 + m * h)
            z0, z1 = z1, [a + 2 * h * b for a, b in zip(z0, fz)]
        fz = f(z1, tf)
        row_j = [[(a + b + h * c) / 2 for a, b, c in zip(z1, z0, fz)]]
        for k in range(1, j + 1):
            r = (mp.mpf(n) / (2 * (j - k + 1))) ** 2
            row_j.append([a + (a - b) / (r - 1) for a, b in zip(row_j[k - 1], T[j - 1][k - 1])])
        T.append(row_j)
    return T[-1][-1], T[-3][-1]


def main():
    from oracle import bindings as oracle
    oracle.build()
    out, cases = {}, []
    for spec in SPECS:
        traj = make_traj(spec)
        xv, uv, pv = spec["sizes"]
        nint = traj.shape[0] - 1
        assert np.abs(np.diff(traj[:, xv])).max() <= 0.2, (spec["name"], np.abs(np.diff(traj[:, xv])).max())
        xe, worst = [], mp.mpf(0)
        for i in range(nint):
            a, b = solve_interval(spec, traj, i)
            worst = max(worst, max(abs(p - q) / max(1, abs(p)) for p, q in zip(a, b)))
            xe.append(a)
        assert worst < CONVERGED, (spec["name"], mp.nstr(worst, 5))
        x_exact = np.array([[float(v) for v in r] for r in xe]).reshape(nint, xv)
        rhs = ick.oracle_rhs(oracle, spec["ode"])
        opt = gck.options(**spec["options"])
        x64, steps64, st64 = gck.reintegrate(rhs, traj, spec["mode"], spec["blocked"], xv, uv, opt, float)
        xld, stepsld, stld = gck.reintegrate(rhs, traj, spec["mode"], spec["blocked"], xv, uv, opt, gck.LD)
        assert (st64 == 0).all() and (stld == 0).all(), spec["name"]
        err64 = np.array([[float(abs(mp.mpf(float(x64[i, k])) - xe[i][k])) for k in range(xv)] for i in range(nint)]).reshape(nint, xv)
        d64 = np.abs(x64.astype(gck.LD) - xld).astype(float)
        quarter = steps64[:, :1] * np.broadcast_to(np.asarray(opt["abs_tol"], dtype=float), (xv,))[None, :]
        if opt["adaptive"]:
            assert (err64 <= quarter).all(), (spec["name"], float((err64 / quarter).max()))
        hi = xld.astype(float)
        for k, v in dict(traj=traj, x_exact=x_exact, steps64=steps64.astype(np.int32), err64=err64, d64=d64, xld_hi=hi,
                         xld_lo=(xld - hi.astype(gck.LD)).astype(float)).items():
            out[f"{spec['name']}.{k}"] = v
        cases.append(dict(spec, convergence=float(worst), quarter_used=float((err64 / quarter).max()), d64_max=float(d64.max()),
                          steps64_total=[int(v) for v in steps64.sum(axis=0)]))
        print(f"{spec['name']}: {nint} intervals, convergence {mp.nstr(worst, 3)}, err64 / quarter bound {(err64 / quarter).max():.3g}, "
              f"steps {steps64.sum(axis=0)}, d64 {d64.max():.2e}", flush=True)
    meta = dict(dps=mp.mp.dps, mpmath=mp.__version__, method=f"modified midpoint, h^2 extrapolation to depth {DEPTH}; checked against depth "
                f"{DEPTH - 2} to 1e-25", eps_f_factor=gck.EPS_F_FACTOR, cases=cases)
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.join(HERE, "mesh_integ"), exist_ok=True)
    path = os.path.join(HERE, "mesh_integ", "mesh_error_integ.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main()
