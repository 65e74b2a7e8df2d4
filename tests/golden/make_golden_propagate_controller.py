"""Generate tests/golden/propagate_controller/controller.npz (run once, here; commit the file): states at every output time, the
state-transition matrix at tf and the two time columns of the closed loop of three small propagation cases with a controller, in
50-digit arithmetic (csrc/propagate_ctrl_kernels.h; tests/controller_checker.py).

Per problem the augmented system  x' = f_c(x, t, p),  S' = J_x S + [0 | J_p],  S(t0) = [I | 0]  of the CLOSED loop f_c(x, t, p) = f(x, t, K(.), p)
is integrated by mpmath's Taylor-series integrator (``mpmath.odefun``) to every sample time -- the float64 times of
propagate_checker.sample_times, promoted exactly; an arc backward in time is integrated in tau = t0 - t.  The right-hand sides, the
laws and their derivatives are written here in mpf by hand, independent of tests/controller_checker.py (numpy) and of
tests/controller_cases.py (the DSL).  ASSERTED: the integration at 50 and at 65 digits agree to 1e-40 (relative to max(1, |y|)), and for
``pd`` -- a damped oscillator, x(t) = e^(-a s) (x0 cos w s + (x1 + a x0) / w sin w s), a = 0.2, w = sqrt(p0 - a^2) -- the integrated states and
x0 columns agree with the closed form to 1e-40 and the p0 column with its numerical derivative to 1e-20.

Cases (the ODE input row is [x0, x1, t, u, p0]; the rows' u entries hold 7.0, which nothing may read):
    pd        x0' = x1, x1' = u with u = -p0 x0 - 0.4 x1, varlocs [0, 1, 4]; m = 5, ns = 4, both time directions
    vdp_fb    vanderpol with u = -0.5 tanh(x1) cos t, varlocs [1, 2]; m = 3, ns = 3
    pd_fixed  pd with Adaptive = False, ns = 1, m = 3: held to the longdouble restatement, 8 d64 + 16 u |x|, equal step counts
The file holds the arrays of propagate_checker.ARRAYS (S of width N - 1 with exactly zero u columns), so the bound functions of
propagate_checker apply as they are.  ASSERTED here (controller_checker.check_restatement): the float64 restatement uses at most a
quarter of every bound; a case that fails gets shorter arcs, the bound is not widened.

Usage:  python tests/golden/make_golden_propagate_controller.py
"""
from __future__ import annotations

import json
import multiprocessing as mproc
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import controller_checker as cck  # noqa: E402
import propagate_checker as pck  # noqa: E402

DPS, DPS_CHECK = 50, 65
AGREE = mp.mpf(10) ** -40
C04, C01 = mp.mpf(0.4), mp.mpf(0.1)      # the doubles the laws and the ODE are written with, promoted exactly


# ---- the closed loops in mpf: value, J_x [2][2], J_p [2]; y = (x0, x1), p = p0 (pd) or mu (vanderpol)
def pd_loop(x, t, p):
    return [x[1], -p * x[0] - C04 * x[1]], [[0, 1], [-p, -C04]], [0, -x[0]]


def vdp_loop(x, t, p):
    e = mp.exp(-C01 * t)
    K = -mp.mpf("0.5") * mp.tanh(x[1]) * mp.cos(t)
    dK = -mp.mpf("0.5") * mp.cos(t) / mp.cosh(x[1]) ** 2
    f = [x[1], p * (1 - x[0] ** 2) * x[1] - x[0] + K * e]
    Jx = [[0, 1], [-2 * p * x[0] * x[1] - 1, p * (1 - x[0] ** 2) + dK * e]]
    return f, Jx, [0, (1 - x[0] ** 2) * x[1]]


LOOPS = {"pd": pd_loop, "vdp_fb": vdp_loop}


def _specs():
    out = []

    def add(name, law, ode, rows, tfs, ns, **opts):
        out.append(dict(name=name, law=law, ode=ode, sizes=[2, 1, 1], ns=ns, options=opts, rows=np.asarray(rows, dtype=float),
                        tfs=np.asarray(tfs, dtype=float)))

    rows = np.array([[1.0, 0.0, 0.0, 7.0, 1.0], [0.5, -0.8, 0.25, 7.0, 2.5], [-0.7, 0.6, 1.0, 7.0, 0.6], [0.2, 1.1, -0.5, 7.0, 4.0],
                     [-1.2, -0.3, 0.125, 7.0, 1.5]])
    add("pd", "pd", "pd", rows, rows[:, 2] + np.array([0.5, -0.4, 0.3, -0.5, 0.45]), 4, def_step=0.05, min_step=1e-6, max_step=100.0)
    rows = np.array([[1.2, -0.4, 0.0, 7.0, 0.8], [-0.6, 0.9, 0.5, 7.0, 1.3], [0.3, 0.2, 1.0, 7.0, 0.5]])
    add("vdp_fb", "vdp_fb", "vanderpol", rows, rows[:, 2] + np.array([0.5, -0.45, 0.4]), 3, def_step=0.05, min_step=1e-6, max_step=100.0)
    rows = np.array([[1.0, 0.0, 0.0, 7.0, 1.0], [0.5, -0.8, 0.25, 7.0, 2.5], [-0.7, 0.6, 1.0, 7.0, 0.6]])
    # (arcs that are no multiple of the step: the number of steps does not hang on the rounding of H / DefStepSize)
    add("pd_fixed", "pd", "pd", rows, rows[:, 2] + np.array([0.47, -0.38, 0.31]), 1, adaptive=False, def_step=0.05, min_step=1e-5, max_step=1000.0)
    return out


def _integrate(loop, row, times, dps):
    """[y(t) for t in times], y = (x0, x1, S row-major [2][3], columns x0, x1, p)"""
    mp.mp.dps = dps
    t0, p = mp.mpf(float(row[2])), mp.mpf(float(row[4]))
    s = 1 if float(times[-1]) >= float(row[2]) else -1

    def G(tau, y):
        f, Jx, Jp = loop(y[:2], t0 + s * tau, p)
        S = [y[2:5], y[5:8]]
        dS = [[Jx[k][0] * S[0][c] + Jx[k][1] * S[1][c] + (Jp[k] if c == 2 else 0) for c in range(3)] for k in range(2)]
        return [s * v for v in f + dS[0] + dS[1]]
    y0 = [mp.mpf(float(row[0])), mp.mpf(float(row[1])), 1, 0, 0, 0, 1, 0]
    sol = mp.odefun(G, 0, [mp.mpf(v) for v in y0])
    return [[+v for v in sol(s * (mp.mpf(float(t)) - t0))] for t in times]


def _pd_closed_form(row, t, p=None):
    t0 = mp.mpf(float(row[2]))
    p = mp.mpf(float(row[4])) if p is None else p
    a = C04 / 2
    w, s = mp.sqrt(p - a * a), mp.mpf(float(t)) - t0

    def x(x0, x1):
        c, sn, e = mp.cos(w * s), mp.sin(w * s), mp.exp(-a * s)
        A, Bc = x0, (x1 + a * x0) / w
        pos = e * (A * c + Bc * sn)
        vel = e * ((Bc * w - a * A) * c - (A * w + a * Bc) * sn)
        return [pos, vel]
    return x


def solve_problem(task):
    spec, i = task
    row, tf, ns = spec["rows"][i], float(spec["tfs"][i]), spec["ns"]
    loop = LOOPS[spec["law"]]
    times = list(pck.sample_times(row[2], tf, ns)) if ns > 1 else [row[2], tf]
    ys = _integrate(loop, row, times, DPS)
    yc = _integrate(loop, row, times, DPS_CHECK)
    mp.mp.dps = DPS
    worst = max(abs(a - b) / max(1, abs(a)) for ya, yb in zip(ys, yc) for a, b in zip(ya, yb))
    assert worst < AGREE, (spec["name"], i, worst)
    if spec["law"] == "pd":
        x0, x1 = mp.mpf(float(row[0])), mp.mpf(float(row[1]))
        for t, y in zip(times, ys):
            cf = _pd_closed_form(row, t)
            ref = cf(x0, x1) + [cf(1, 0)[0], cf(0, 1)[0], cf(1, 0)[1], cf(0, 1)[1]]
            got = y[:2] + [y[2], y[3], y[5], y[6]]
            assert max(abs(a - b) for a, b in zip(got, ref)) < AGREE, (spec["name"], i, "closed form")
            for k in range(2):
                dp = mp.diff(lambda q: _pd_closed_form(row, t, q)(x0, x1)[k], mp.mpf(float(row[4])))
                assert abs(dp - y[4 + 3 * k]) < mp.mpf(10) ** -20, (spec["name"], i, "closed form, p0 column")
    t0m, tfm, p = mp.mpf(float(row[2])), mp.mpf(tf), mp.mpf(float(row[4]))
    yf = ys[-1]
    f0 = loop(ys[0][:2], t0m, p)[0]
    ff, Jxf, _ = loop(yf[:2], tfm, p)
    Sx = [[yf[2], yf[3]], [yf[5], yf[6]]]
    # S of width N - 1 = 4: columns [x0, x1, u (exactly zero: the closed loop does not read it), p0]
    S = [[yf[2], yf[3], 0, yf[4]], [yf[5], yf[6], 0, yf[7]]]
    smax = np.abs(np.eye(2))
    for y in ys:
        smax = np.maximum(smax, np.array([[float(abs(y[2])), float(abs(y[3]))], [float(abs(y[5])), float(abs(y[6]))]]))
    fl = lambda rows: np.array([[float(v) for v in r] for r in rows])
    xs = [y[:2] for y in (ys if ns > 1 else ys[-1:])]
    return dict(x_exact=fl(xs), S_exact=fl(S), S_max=smax, dt0_exact=np.array([float(-(Sx[k][0] * f0[0] + Sx[k][1] * f0[1])) for k in range(2)]),
                dtf_exact=np.array([float(v) for v in ff]), f0=np.array([float(v) for v in f0]),
                Jxf_abs=np.array([[float(abs(mp.mpf(v))) for v in r] for r in Jxf]), convergence=float(worst))


def main():
    from oracle import bindings as oracle
    oracle.build()
    out, cases, k = {}, [], 0
    specs = _specs()
    tasks = [(s, i) for s in specs for i in range(len(s["tfs"]))]
    with mproc.get_context("fork").Pool(min(len(tasks), os.cpu_count() or 1)) as pool:
        solved = pool.map(solve_problem, tasks, chunksize=1)
    for s in specs:
        m = len(s["tfs"])
        res, k = solved[k:k + m], k + m
        case = dict(s)
        for a in ("x_exact", "S_exact", "S_max", "dt0_exact", "dtf_exact", "f0", "Jxf_abs"):
            case[a] = np.array([r[a] for r in res])
        r = cck.restate_case(oracle, case)
        used = cck.check_restatement(case, r, cck.closed_loop_of(oracle, s["law"])[0])
        n, Cc = 2, 4
        zero = dict(xld=np.zeros((m, n), dtype=pck.LD), Sld=np.zeros((m, n, Cc), dtype=pck.LD), d64=np.zeros((m, n)), dS64=np.zeros((m, n, Cc)))
        zero.update(r)
        case.update(zero)
        for a in pck.ARRAYS:
            out[f"{s['name']}.{a}"] = np.asarray(case[a], dtype=np.int32 if a.startswith("steps") else float)
        for a in ("xld", "Sld"):
            hi = case[a].astype(float)
            out[f"{s['name']}.{a}_hi"], out[f"{s['name']}.{a}_lo"] = hi, (case[a] - hi.astype(pck.LD)).astype(float)
        meta = {k: v for k, v in s.items() if k not in ("rows", "tfs")}
        conv = max(x["convergence"] for x in res)
        meta.update(m=m, convergence=conv, quarter_used=used, eS=[float(v) for v in r["eS"]],
                    steps64_total=[int(v) for v in r["steps64"].sum(axis=0)], steps64_end_total=[int(v) for v in r["steps64_end"].sum(axis=0)])
        cases.append(meta)
        print(f"{s['name']}: m {m}, ns {s['ns']}, 50 / 65 digits agree to {conv:.2e}, quarter of the bounds used {used}, eS {r['eS'].max():.3e}, "
              f"steps (dense) {r['steps64'].sum(axis=0)}, (ns = 1) {r['steps64_end'].sum(axis=0)}", flush=True)
    meta = dict(dps=DPS, mpmath=mp.__version__, method=f"mpmath.odefun (Taylor series) on the closed loop and its variational equations; "
                f"{DPS} and {DPS_CHECK} digits agree to 1e-40", cases=cases)
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.join(HERE, "propagate_controller"), exist_ok=True)
    path = os.path.join(HERE, "propagate_controller", "controller.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main()
