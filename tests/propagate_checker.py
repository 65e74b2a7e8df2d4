"""Independent restatement of the batched propagation (csrc/propagate_kernels.h behind asset_hip_propagate / asset_hip_propagate_stm and
asset_asrl_amd/integrator.py), its error bounds, and the loader of the 50-digit fixture tests/golden/propagate/propagate.npz
(tests/golden/make_golden_propagate.py).  Pure numpy; nothing here touches the code under test.

What is restated: the step rule of tests/integ_checker.py (its tableau, options and defaults are used as they are) for ONE initial-value
problem with held controls and parameters, with output times -- sample j at t0 + (j H) / (ns - 1), each reached by shortening the step
that would reach or pass it (an output time that rounds to the current time copies the state without a step); after an accepted
shortened step the next step is the controller's new h or the unshortened one, whichever is larger in size -- and with the state-transition matrix: every column of S = d x(tf) / d [x0, u, p] carried through the same stages of
the same steps, KC_s = h J(X_s) W_s.  The right-hand side and its Jacobian are callbacks on float64 rows (the oracle's ``OdeStruct.f`` and
``OdeStruct.fj``: oracle_f, oracle_fj); `dtype` is the arithmetic of everything else (float64 or longdouble).

Bounds (u = 2^-53).  None is measured against the code under test.
    states, adaptive     |x - x_exact|_k <= B_k = sum_j S_max[k][j] AbsTol_j accepted64: a local error of at most the tolerance per accepted
                         step, carried to the end by the flow's own sensitivity (S_max: the entry-wise maximum of |d x(t_j) / d x0| over
                         the case's samples, t0 included).  Condition (generator, CPU test): the float64 restatement uses at most B / 4.
    fixed steps          no accept / reject decisions: |x - longdouble restatement| <= 8 d64 + 16 u |x|, d64 = |float64 restatement -
                         longdouble restatement|; the same for S with dS64; step counts equal.
    STM, adaptive        a flipped decision changes the step sequence and with it the discretisation error of S: eS = max |S_restated -
                         S_exact| over the float64 restatement at AbsTol x {1/2, 1, 2}; |S - S_exact| <= 4 eS + 16 u |S_exact| (4: the
                         quarter-of-the-bound convention of the states).
    time columns         through their closed forms: d xf / d tf = f(xf): sum_j |J_x(xf)|_kj B_j + 16 u |f|;  d xf / d t0 = -S_x f(x0):
                         sum_j (4 eS + 16 u |S_kj|) |f0_j| + 16 u sum_j |S_kj f0_j|.
    controller           totals of accepted and rejected steps within max(2, 10 %) of the restatement's (integ_checker.compare_step_totals)."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

import integ_checker as gck

_HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(_HERE, "golden", "propagate", "propagate.npz")   # (a directory of its own: tests/test_oracle.py takes every
                                                                        # tests/golden/*.npz for a defect vector)
U = gck.U
LD = gck.LD
TOL_FACTORS = (0.5, 1.0, 2.0)


def oracle_f(oracle, name: str):
    """y[N] -> f[n] through ``void f(const double* y, double* fx, const void* ctx)`` (oracle/oracle.h)."""
    o = oracle.get_ode(name, 0)
    fn = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)(o.f)
    dp = C.POINTER(C.c_double)

    def f(y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        out = np.zeros(o.xv)
        fn(y.ctypes.data_as(dp), out.ctypes.data_as(dp), o.ctx)
        return out
    f.keep = (o, fn)
    return f


def oracle_fj(oracle, name: str):
    """y[N] -> (f[n], J[n, N]) through ``void fj(const double* y, double* fx, double* J, const void* ctx)``."""
    o = oracle.get_ode(name, 0)
    fn = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)(o.fj)
    dp = C.POINTER(C.c_double)
    N = o.xv + 1 + o.uv + o.pv

    def fj(y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        out, J = np.zeros(o.xv), np.zeros((o.xv, N))
        fn(y.ctypes.data_as(dp), out.ctypes.data_as(dp), J.ctypes.data_as(dp), o.ctx)
        return out, J
    fj.keep = (o, fn)
    return fj


def sample_times(t0, tf, ns, dtype=float):
    """The output times of a dense call (float64 arithmetic, as the kernel and integrator.py form them), as `dtype`."""
    t0, tf = float(t0), float(tf)
    if ns == 1:
        return np.array([tf]).astype(dtype)
    H = tf - t0
    t = np.array([t0 + (float(j) * H) / float(ns - 1) for j in range(ns)])
    t[-1] = tf
    return t.astype(dtype)


def propagate(f, fj, row, tf, ns, opt, dtype=float, stm=False):
    """One problem -> dict(xs[ns, n] `dtype` (NaN where not reached), S[n, C] or None, steps (accepted, rejected), status).
    stm needs ns == 1."""
    A, Cc, Bw, Bh = gck.tableau(dtype)
    row = np.asarray(row, dtype=float)
    n = f(row).size
    N = row.size
    Ccols = N - 1
    assert not (stm and ns != 1)
    xs_out = np.full((ns, n), np.nan, dtype=dtype)
    S = None
    if stm:
        S = np.zeros((n, Ccols), dtype=dtype)
        S[:, :n] = np.eye(n, dtype=dtype)
        E = np.zeros((N, Ccols), dtype=dtype)              # unit entries of the control and parameter columns, ODE-input space
        for c in range(n, Ccols):
            E[c + 1, c] = 1
    nanS = None if not stm else np.full((n, Ccols), np.nan, dtype=dtype)
    if not (np.isfinite(row[:n + 1]).all() and np.isfinite(tf)):
        if ns > 1:
            xs_out[0] = row[:n]
        return dict(xs=xs_out, S=nanS, steps=(0, 0), status=2)
    x, tc, tfd = row[:n].astype(dtype), dtype(row[n]), dtype(tf)
    j = 0
    if ns > 1:
        xs_out[0] = x
        j = 1
    H = tfd - tc
    if H == 0:
        xs_out[:] = x
        return dict(xs=xs_out, S=S, steps=(0, 0), status=0)
    atol, rtol = (np.broadcast_to(np.asarray(opt[k], dtype=float), (n,)).astype(dtype) for k in ("abs_tol", "rel_tol"))
    numsteps = int(abs(H / dtype(opt["def_step"]))) + 1
    h = dtype(0.9) * (H / dtype(numsteps))
    acc_n = rej_n = 0
    times = sample_times(row[n], tf, ns, dtype)

    def rhs(xst, ts):
        y = row.copy()
        y[:n], y[n] = xst.astype(float), float(ts)
        if stm:
            fv, J = fj(y)
            return fv.astype(dtype), J.astype(dtype)
        return f(y).astype(dtype), None

    def fail(status):
        return dict(xs=xs_out, S=nanS, steps=(acc_n, rej_n), status=status)

    with np.errstate(all="ignore"):
        while j < ns:
            tt = times[j]
            while tt != tc:
                if acc_n + rej_n >= opt["max_steps"]:
                    return fail(1)
                tnext, last, hfull = tc + h, False, h
                if (tnext - tt >= 0) if H > 0 else (tnext - tt <= 0):
                    h, tnext, last = tt - tc, tt, True
                hs = tnext - tc
                Ks = np.zeros((13, n), dtype=dtype)
                Kc = np.zeros((13, n, Ccols), dtype=dtype) if stm else None
                for s in range(13):
                    xst = x.copy()
                    for q in range(s):
                        xst = xst + A[s - 1][q] * Ks[q]
                    ts = tc if s == 0 else tc + Cc[s - 1] * hs
                    fv, J = rhs(xst, ts)
                    Ks[s] = fv * hs
                    if stm:
                        W = E.copy()
                        Ws = S.copy()
                        for q in range(s):
                            Ws = Ws + A[s - 1][q] * Kc[q]
                        W[:n] = Ws
                        Kc[s] = (J @ W) * hs
                xn, xe = x.copy(), x.copy()
                for s in range(13):
                    xn = xn + Bw[s] * Ks[s]
                    xe = xe + Bh[s] * Ks[s]
                if not (np.isfinite(h) and np.isfinite(xn).all()):
                    return fail(2)
                reject = False
                if opt["adaptive"]:
                    ek, ak = np.abs(xn - xe), atol + np.abs(xn) * rtol
                    w = int(np.argmax(ek / ak))
                    err, acc = ek[w], ak[w]
                    hnext = dtype(0.9) * h * (acc / err) ** (dtype(1) / dtype(8))
                    msc = dtype(opt["max_step_change"])
                    if hnext / h > msc:
                        h = h * msc
                    elif hnext / h < 1 / msc:
                        h = h / msc
                    else:
                        h = hnext
                    if abs(h) > opt["max_step"]:
                        h = dtype(opt["max_step"]) * h / abs(h)
                    hit_min = False
                    if abs(h) < opt["min_step"]:
                        h, hit_min = dtype(opt["min_step"]) * h / abs(h), True
                    reject = (err - acc) > 0 and not hit_min
                if reject:
                    rej_n += 1
                    continue
                acc_n += 1
                if stm:
                    Sn = S.copy()
                    for s in range(13):
                        Sn = Sn + Bw[s] * Kc[s]
                    S = Sn
                x, tc = xn, tnext
                if last:
                    if abs(h) < abs(hfull):
                        h = hfull
                    break
            xs_out[j] = x
            j += 1
    return dict(xs=xs_out, S=S, steps=(acc_n, rej_n), status=0)


def propagate_batch(f, fj, rows, tfs, ns, opt, dtype=float, stm=False):
    """(xs[m, ns, n], S[m, n, C] or None, steps[m, 2], status[m])"""
    res = [propagate(f, fj, r, t, ns, opt, dtype, stm) for r, t in zip(np.atleast_2d(rows), np.ravel(tfs))]
    return (np.array([r["xs"] for r in res], dtype=dtype), np.array([r["S"] for r in res], dtype=dtype) if stm else None,
            np.array([r["steps"] for r in res], dtype=int).reshape(-1, 2), np.array([r["status"] for r in res], dtype=int))


def time_columns(f, rows, tfs, xf, S, dtype=LD):
    """(d xf / d t0 [m, n], d xf / d tf [m, n]) from the closed forms."""
    rows = np.atleast_2d(np.asarray(rows, dtype=float))
    m, n = rows.shape[0], np.asarray(xf).shape[-1]
    d0, df = np.zeros((m, n), dtype=dtype), np.zeros((m, n), dtype=dtype)
    for i in range(m):
        y = rows[i].copy()
        f0 = f(y).astype(dtype)
        y[:n], y[n] = np.asarray(xf[i], dtype=float), float(np.ravel(tfs)[i])
        df[i] = f(y).astype(dtype)
        d0[i] = -(np.asarray(S[i]).astype(dtype)[:, :n] @ f0)
    return d0, df


def jac_from(S, d0, df):
    """J[m, n, N + 1] with columns [x0 | t0 | u | p | tf] from S[m, n, C] and the two time columns."""
    S = np.asarray(S)
    m, n, Cc = S.shape
    J = np.zeros((m, n, Cc + 2), dtype=S.dtype)
    J[:, :, :n], J[:, :, n], J[:, :, n + 1:Cc + 1], J[:, :, Cc + 1] = S[:, :, :n], d0, S[:, :, n:], df
    return J


# ------------------------------------------------------------------------------------------------ bounds
def state_bound(S_max, accepted64, abs_tol):
    """B[m, n] = sum_j S_max[m, k, j] AbsTol_j accepted64[m]."""
    S_max = np.asarray(S_max, dtype=float)
    atol = np.broadcast_to(np.asarray(abs_tol, dtype=float), (S_max.shape[-1],))
    return (S_max * atol[None, None, :]).sum(axis=2) * np.asarray(accepted64, dtype=float)[:, None]


def stm_bound(S_exact, eS):
    """[m, n, C]: 4 eS + 16 u |S_exact|."""
    S_exact = np.asarray(S_exact, dtype=float)
    return 4.0 * np.asarray(eS, dtype=float)[:, None, None] + 16.0 * U * np.abs(S_exact)


def time_column_bounds(S_exact, eS, f0, Jxf_abs, B, dtf_exact):
    """(bound of d xf / d t0 [m, n], bound of d xf / d tf [m, n])."""
    S = np.abs(np.asarray(S_exact, dtype=float))
    n = S.shape[1]
    Sx, af0 = S[:, :, :n], np.abs(np.asarray(f0, dtype=float))
    b0 = ((4.0 * np.asarray(eS, dtype=float)[:, None, None] + 16.0 * U * Sx) * af0[:, None, :]).sum(axis=2) + 16.0 * U * (Sx * af0[:, None, :]).sum(axis=2)
    bf = (np.asarray(Jxf_abs, dtype=float) * np.asarray(B, dtype=float)[:, None, :]).sum(axis=2) + 16.0 * U * np.abs(np.asarray(dtf_exact, dtype=float))
    return b0, bf


def compare(got, ref, bound, what=""):
    """asserts |got - ref| <= bound everywhere (NaN fails); prints and returns the worst ratio."""
    got, ref, bound = np.asarray(got), np.asarray(ref), np.asarray(bound, dtype=float)
    d = np.abs(got.astype(LD) - ref.astype(LD)).astype(float)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    worst = float(np.nanmax(ratio, initial=0.0))
    print(f"{what}: worst |got - ref| / bound = {worst:.3g}")
    bad = np.argwhere(~(d <= bound))
    assert bad.size == 0, (f"{what}: outside the bound at {len(bad)} entries, worst ratio {worst:.3g}; first {tuple(bad[0])}: got "
                           f"{got[tuple(bad[0])]!r} ref {ref[tuple(bad[0])]!r} bound {bound[tuple(bad[0])]:.3e}")
    return worst


# ------------------------------------------------------------------------------------------------ the fixture
_CACHE = None
ARRAYS = ("rows", "tfs", "x_exact", "S_exact", "S_max", "dt0_exact", "dtf_exact", "f0", "Jxf_abs", "x64", "x64_end", "S64", "steps64",
          "steps64_end", "steps64_stm", "eS", "d64", "dS64")


def fixture():
    """(meta, cases): cases[name] = the case's meta data (ode, sizes, ns, options) with the arrays of ARRAYS -- rows [m, N], tfs [m],
    x_exact [m, ns, n] (every sample), S_exact [m, n, C], S_max [m, n, n], the exact time columns [m, n], f0 = f(row), Jxf_abs =
    |J_x(xf)|, the float64 restatement's samples x64, ns = 1 end states x64_end, STM S64 and step counts (dense, ns = 1, STM run), eS [m],
    and for the fixed-step case d64 [m, n], dS64 [m, n, C] with the longdouble restatement 'xld' [m, n], 'Sld' [m, n, C]."""
    global _CACHE
    if _CACHE is None:
        z = np.load(FIXTURE)
        meta = json.loads(str(z["meta"]))
        cases = {}
        for c in meta["cases"]:
            d = dict(c)
            for a in ARRAYS:
                d[a] = z[f"{c['name']}.{a}"]
            for a in ("xld", "Sld"):
                d[a] = z[f"{c['name']}.{a}_hi"].astype(LD) + z[f"{c['name']}.{a}_lo"].astype(LD)
            cases[c["name"]] = d
        _CACHE = (meta, cases)
    return _CACHE


def case_names():
    return list(fixture()[1]) if os.path.exists(FIXTURE) else []


def case_options(case, tol_factor=1.0):
    o = gck.options(**case["options"])
    o["abs_tol"] = np.asarray(o["abs_tol"], dtype=float) * tol_factor
    return o


def restate_case(oracle, case):
    """Everything the generator records of the restatement, computed again: dict of the arrays x64, x64_end, S64, steps64, steps64_end,
    steps64_stm, eS, and for a fixed-step case xld, Sld, d64, dS64."""
    f, fj = oracle_f(oracle, case["ode"]), oracle_fj(oracle, case["ode"])
    rows, tfs, ns = case["rows"], case["tfs"], case["ns"]
    opt = case_options(case)
    out = {}
    x64, _, st, status = propagate_batch(f, fj, rows, tfs, ns, opt)
    assert (status == 0).all()
    out["x64"], out["steps64"] = x64, st
    x1, S64, st1, status = propagate_batch(f, fj, rows, tfs, 1, opt, stm=True)
    assert (status == 0).all()
    out["x64_end"], out["S64"], out["steps64_end"], out["steps64_stm"] = x1[:, 0], S64, st1, st1
    eS = np.abs(S64.astype(LD) - case["S_exact"].astype(LD)).astype(float).max(axis=(1, 2))
    if opt["adaptive"]:
        for fac in TOL_FACTORS:
            if fac == 1.0:
                continue
            _, Sf, _, status = propagate_batch(f, fj, rows, tfs, 1, case_options(case, fac), stm=True)
            assert (status == 0).all()
            eS = np.maximum(eS, np.abs(Sf.astype(LD) - case["S_exact"].astype(LD)).astype(float).max(axis=(1, 2)))
    else:
        xl, Sl, stl, status = propagate_batch(f, fj, rows, tfs, 1, opt, dtype=LD, stm=True)
        assert (status == 0).all() and np.array_equal(stl, st1)
        out["xld"], out["Sld"] = xl[:, 0], Sl
        out["d64"] = np.abs(x1[:, 0].astype(LD) - xl[:, 0]).astype(float)
        out["dS64"] = np.abs(S64.astype(LD) - Sl).astype(float)
    out["eS"] = eS
    return out


def check_restatement(case, r):
    """The conditions the bounds rest on (asserted by the generator and by tests/test_propagate_cpu.py); returns the fractions used."""
    opt = case_options(case)
    used = {}
    if opt["adaptive"]:
        for xs, steps, ref, tag in ((r["x64"], r["steps64"], case["x_exact"], "samples"),
                                    (r["x64_end"][:, None, :], r["steps64_end"], case["x_exact"][:, -1:, :], "end")):
            B = state_bound(case["S_max"], steps[:, 0], opt["abs_tol"])
            err = np.abs(xs.astype(LD) - ref.astype(LD)).astype(float)
            frac = float((err / (B[:, None, :] / 4.0)).max())
            assert frac <= 1.0, (case["name"], tag, frac)
            used[tag] = frac
    else:
        assert (r["d64"] <= 64 * U * np.maximum(1.0, np.abs(case["x_exact"][:, -1])).max()).all(), case["name"]
    return used
