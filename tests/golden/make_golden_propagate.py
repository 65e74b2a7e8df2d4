"""Generate tests/golden/propagate/propagate.npz (run once, here; commit the file): states at every output time, the state-transition
matrix at tf and the two time columns of a dozen small propagation cases in 50-digit arithmetic, for the batched propagation
(csrc/propagate_kernels.h; tests/propagate_checker.py).

Per problem the augmented system  x' = f(x, t, u, p),  S' = J_x S + [0 | J_u | J_p],  S(t0) = [I | 0]  (S = d x / d [x0, u, p], controls and
parameters held at the row's) is integrated from sample time to sample time -- the float64 times of propagate_checker.sample_times, promoted
exactly -- in pieces of at most HMAX.  Method, that of make_golden_mesh_integ.py: Gragg's modified midpoint rule with 2, 4, .., 2 k substeps
over a piece, extrapolated in h^2 (k = 14, pieces of 0.1; Reentry: k = 24, pieces of 0.05; synthetic32: k = 10, pieces of 0.0125); the extrapolation to depth k and the one to depth k - 2 are ASSERTED to agree: the sum over a problem's
pieces of their difference (relative to max(1, |y|)) stays below 1e-25.  The right-hand sides are make_golden_mesh.ODES (and make_golden's
synthetic32) in mpf; the Jacobian-vector products J w come from make_golden.D2 seeded with one direction (a 1 x 1 Hessian: the full
N x N one costs N^2 per operation).  Nothing of asset_asrl_amd/csrc is used.

Per case the file holds (propagate_checker.fixture): x_exact at every sample, S_exact at tf, S_max = the entry-wise maximum of |S_x| over the
samples (t0 included), the exact time columns -S_x f(x0) and f(xf), f0 and |J_x(xf)| for their bounds, and the float64 / longdouble
restatement's states, STM and step counts (propagate_checker.restate_case: the oracle's ``f`` and ``fj``) with eS = max |S_restated - S_exact|
over AbsTol x {1/2, 1, 2}.  ASSERTED here: the float64 restatement is within B / 4 on every adaptive case (propagate_checker.check_restatement);
a case that fails is replaced, the bound is not widened.  eS per case is printed.

Usage:  python tests/golden/make_golden_propagate.py [case name ...]
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

import propagate_checker as pck  # noqa: E402
from make_golden import D2, MP  # noqa: E402
from make_golden import ODES as GOLDEN_ODES  # noqa: E402
from make_golden_mesh import ODES as MESH_ODES  # noqa: E402
from make_golden_mesh import M  # noqa: E402

mp.mp.dps = 50
HMAX = 0.1
CONVERGED = mp.mpf(10) ** -25
ODES = dict(MESH_ODES)
ODES["synthetic32"] = (GOLDEN_ODES["synthetic32"], (32, 0, 0))


def kepler_row(scale=1.0):
    """A bound two-body state (mu = 1) and its period: r = (0.5, 0, 0) scale, v = (0, 1.5, 0.2) / sqrt(scale)."""
    r = np.array([0.5, 0.0, 0.0]) * scale
    v = np.array([0.0, 1.5, 0.2]) / np.sqrt(scale)
    row = np.concatenate([r, v, [0.25], [0.0, 0.0, 0.0]])
    rm, vm = [mp.mpf(float(a)) for a in r], [mp.mpf(float(a)) for a in v]
    a = 1 / (2 / mp.sqrt(sum(c * c for c in rm)) - sum(c * c for c in vm))
    return row, 2 * mp.pi * a ** mp.mpf(1.5)


def _specs():
    out = []

    def add(name, ode, rows, tfs, ns, **opts):
        rows = np.atleast_2d(np.asarray(rows, dtype=float))
        # (random Reentry states move fast: shorter pieces and a deeper extrapolation, as make_golden_mesh_integ.py needs for them)
        # (synthetic32, dense: every sample interval is one short piece, where depth 10 converges; its augmented system has 1056 entries)
        hmax, depth = (0.05, 24) if ode == "reentry" else ((0.0125, 10) if ode == "synthetic32" else (HMAX, 14))
        out.append(dict(name=name, ode=ode, sizes=list(ODES[ode][1]), ns=ns, options=opts, rows=rows, tfs=np.asarray(tfs, dtype=float).ravel(),
                        hmax=hmax, depth=depth))

    def random_rows(ode, m, seed, t0=0.0):
        from asset_asrl_amd import synth
        named = ode in ("reentry", "twobody_lt", "synthetic32")
        tr = synth.make_traj(ode, "LGL3", m, seed=seed, T=1.0, sizes=None if named else tuple(ODES[ode][1]))
        rows = tr[:m].copy()
        rows[:, ODES[ode][1][0]] = t0 + 0.125 * np.arange(m)
        return rows

    krow, period = kepler_row()
    T = float(period)
    kep = dict(def_step=0.1, min_step=1e-5, max_step=1000.0)
    add("kepler_quarter", "twobody_lt", krow, [krow[6] + T / 4], 1, **kep)
    add("kepler_full", "twobody_lt", krow, [krow[6] + T], 9, **kep)
    add("kepler_back", "twobody_lt", krow, [krow[6] - T / 4], 1, **kep)
    r = random_rows("reentry", 3, 41)
    add("reentry_short", "reentry", r, r[:, 5] + np.array([0.3, 0.45, -0.35]), 1)
    r = random_rows("reentry", 2, 42)
    add("reentry_dense", "reentry", r, r[:, 5] + np.array([0.5, 0.4]), 9)
    r = random_rows("vanderpol", 2, 43)
    add("vanderpol_dense", "vanderpol", r, r[:, 2] + np.array([0.8, -0.6]), 9, def_step=0.05, min_step=1e-6, max_step=100.0)
    r = random_rows("shape_5_3_2", 2, 44)
    add("shape_5_3_2_dense", "shape_5_3_2", r, r[:, 5] + np.array([0.6, 0.5]), 9, def_step=0.05, min_step=1e-6, max_step=100.0)
    r = random_rows("shape_1_0_0", 2, 45)
    add("shape_1_0_0", "shape_1_0_0", r, r[:, 1] + np.array([0.7, -0.4]), 1)
    r = random_rows("synthetic32", 2, 46, t0=0.3)
    add("synthetic32_dense", "synthetic32", r, r[:, 32] + np.array([0.08, 0.064]), 9)
    r = random_rows("reentry", 2, 47)
    add("reentry_fixed", "reentry", r, r[:, 5] + np.array([0.3, 0.24]), 1, adaptive=False, def_step=0.05, min_step=1e-5, max_step=1000.0)
    return out


def _aug_rhs(ode, row_mp):
    f_ode, (n, uv, pv) = ODES[ode]
    N, Cc = n + 1 + uv + pv, n + uv + pv
    tail = row_mp[n + 1:]
    one = np.array([[mp.mpf(0)]], dtype=object)

    def seed(v, g):
        return D2(v, np.array([mp.mpf(g)], dtype=object), one.copy())

    def jvp(x, t, w):
        """J(x, t, u, p) w for a direction w in ODE-input space (list of N mpf)."""
        y = [seed(x[i], w[i]) for i in range(n)] + [seed(t, w[n])] + [seed(tail[k], w[n + 1 + k]) for k in range(uv + pv)]
        out = f_ode(y, MP)
        return [o.g[0] if isinstance(o, D2) else mp.mpf(0) for o in out]

    def value(x, t):
        return [mp.mpf(v) for v in f_ode(list(x) + [t] + list(tail), M)]

    def rhs(y, t):
        x = y[:n]
        dx = value(x, t)
        dS = [None] * (n * Cc)
        for c in range(Cc):
            w = [y[n + k * Cc + c] for k in range(n)] + [mp.mpf(0)] * (N - n)
            if c >= n:
                w[c + 1] = mp.mpf(1)
            col = jvp(x, t, w)
            for k in range(n):
                dS[k * Cc + c] = col[k]
        return dx + dS
    return rhs, value, jvp, n, N, Cc


def _gbs(rhs, y0, t0, t1, depth):
    """(y(t1) to depth `depth`, the same to depth - 2)."""
    H = t1 - t0
    T = []
    for j in range(depth):
        nn = 2 * (j + 1)
        h = H / nn
        z0, z1 = y0, [a + h * b for a, b in zip(y0, rhs(y0, t0))]
        for m in range(1, nn):
            fz = rhs(z1, t0 + m * h)
            z0, z1 = z1, [a + 2 * h * b for a, b in zip(z0, fz)]
        fz = rhs(z1, t1)
        row_j = [[(a + b + h * c) / 2 for a, b, c in zip(z1, z0, fz)]]
        for k in range(1, j + 1):
            r = (mp.mpf(nn) / (2 * (j - k + 1))) ** 2
            row_j.append([a + (a - b) / (r - 1) for a, b in zip(row_j[k - 1], T[j - 1][k - 1])])
        T.append(row_j)
    return T[-1][-1], T[-3][-1]


def solve_problem(task):
    """One problem in mpf -> dict of float64 arrays and the convergence figure."""
    ode, row, tf, ns, hmax, depth = task
    mp.mp.dps = 50
    row_mp = [mp.mpf(float(v)) for v in row]
    rhs, value, jvp, n, N, Cc = _aug_rhs(ode, row_mp)
    y = row_mp[:n] + [mp.mpf(1 if (k == c) else 0) for k in range(n) for c in range(Cc)]
    t0 = row_mp[n]
    bounds = [t0] + [mp.mpf(float(t)) for t in (pck.sample_times(row[n], tf, ns)[1:] if ns > 1 else [tf])]
    xs, smax, worst = [y[:n]], np.abs(np.eye(n)), mp.mpf(0)
    for ta, tb in zip(bounds[:-1], bounds[1:]):
        nsub = max(1, int(mp.ceil(abs(tb - ta) / mp.mpf(hmax))))
        for k in range(nsub):
            a, b = ta + (tb - ta) * k / nsub, (ta + (tb - ta) * (k + 1) / nsub) if k + 1 < nsub else tb
            y, ylow = _gbs(rhs, y, a, b, depth)
            worst += max(abs(p - q) / max(1, abs(p)) for p, q in zip(y, ylow))
        xs.append(y[:n])
        smax = np.maximum(smax, np.array([[float(abs(y[n + k * Cc + c])) for c in range(n)] for k in range(n)]))
    S = [[y[n + k * Cc + c] for c in range(Cc)] for k in range(n)]
    f0, ff = value(row_mp[:n], t0), value(y[:n], bounds[-1])
    dt0 = [-sum((S[k][j] * f0[j] for j in range(n)), mp.mpf(0)) for k in range(n)]
    Jx = np.zeros((n, n))
    for j in range(n):
        w = [mp.mpf(0)] * N
        w[j] = mp.mpf(1)
        Jx[:, j] = [float(abs(v)) for v in jvp(y[:n], bounds[-1], w)]
    fl = lambda rows: np.array([[float(v) for v in r] for r in rows])
    return dict(x_exact=fl(xs if ns > 1 else xs[-1:]), S_exact=fl(S), S_max=smax, dt0_exact=np.array([float(v) for v in dt0]),
                dtf_exact=np.array([float(v) for v in ff]), f0=np.array([float(v) for v in f0]), Jxf_abs=Jx, convergence=float(worst))


def main(argv):
    from oracle import bindings as oracle
    oracle.build()
    specs = [s for s in _specs() if not argv or s["name"] in argv]
    tasks = [(s["ode"], s["rows"][i], float(s["tfs"][i]), s["ns"], s["hmax"], s["depth"]) for s in specs for i in range(len(s["tfs"]))]
    with mproc.get_context("fork").Pool(min(len(tasks), os.cpu_count() or 1)) as pool:
        solved = pool.map(solve_problem, tasks, chunksize=1)
    out, cases, k = {}, [], 0
    for s in specs:
        m = len(s["tfs"])
        res, k = solved[k:k + m], k + m
        conv = max(r["convergence"] for r in res)
        assert conv < float(CONVERGED), (s["name"], conv)
        case = dict(s)
        for a in ("x_exact", "S_exact", "S_max", "dt0_exact", "dtf_exact", "f0", "Jxf_abs"):
            case[a] = np.array([r[a] for r in res])
        r = pck.restate_case(oracle, case)
        used = pck.check_restatement(case, r)
        n, Cc = s["sizes"][0], sum(s["sizes"])
        zero = dict(xld=np.zeros((m, n), dtype=pck.LD), Sld=np.zeros((m, n, Cc), dtype=pck.LD), d64=np.zeros((m, n)), dS64=np.zeros((m, n, Cc)))
        zero.update(r)
        case.update(zero)
        for a in pck.ARRAYS:
            out[f"{s['name']}.{a}"] = np.asarray(case[a], dtype=np.int32 if a.startswith("steps") else float)
        for a in ("xld", "Sld"):
            hi = case[a].astype(float)
            out[f"{s['name']}.{a}_hi"], out[f"{s['name']}.{a}_lo"] = hi, (case[a] - hi.astype(pck.LD)).astype(float)
        meta = {k2: v for k2, v in s.items() if k2 not in ("rows", "tfs")}
        meta.update(m=m, convergence=conv, quarter_used=used, eS=[float(v) for v in r["eS"]],
                    steps64_total=[int(v) for v in r["steps64"].sum(axis=0)], steps64_end_total=[int(v) for v in r["steps64_end"].sum(axis=0)])
        cases.append(meta)
        print(f"{s['name']}: m {m}, ns {s['ns']}, convergence {conv:.2e}, B/4 used {used}, eS {r['eS'].max():.3e}, steps (dense) "
              f"{r['steps64'].sum(axis=0)}, (ns = 1) {r['steps64_end'].sum(axis=0)}", flush=True)
    if argv:
        print("(partial run: nothing written)")
        return
    meta = dict(dps=mp.mp.dps, mpmath=mp.__version__, method=f"modified midpoint, h^2 extrapolation, pieces of at most {HMAX}; two depths "
                "agree to 1e-25", cases=cases)
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.join(HERE, "propagate"), exist_ok=True)
    path = os.path.join(HERE, "propagate", "propagate.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main(sys.argv[1:])
