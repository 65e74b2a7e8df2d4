"""Independent restatement of the integrator-based mesh-error estimate (csrc/integ_kernels.h behind asset_hip_mesh_error_integrator),
its error bounds, and the loader of the 50-digit fixture tests/golden/mesh_integ/mesh_error_integ.npz (tests/golden/make_golden_mesh_integ.py).
Pure numpy; nothing here touches the code under test.

What is restated (the reference's Integrator::integrate_impl and stepper, ODEPhase::get_meshinfo_integrator): per node interval i the
initial-value problem from row i to t_(i+1) with the Prince-Dormand 8(7) tableau of tests/golden/rk_tables.json (the reference's header
parsed as data) -- first step 0.9 H / (int(|H / def|) + 1), a step reaching t_(i+1) ends there, the order-8 solution propagated,
h <- 0.9 h (acc / err)^(1/8) from the worst |x8 - x7| / (AbsTol + |x8| RelTol), ratio and size clamped, a step with err > acc retried unless h
was raised to the minimum.  Controls: the block's degree cs - 1 polynomial (power weights of tests/golden/lgl_tables.json), or the start
row's held (no controls / BlockConstant); parameters the start row's.  The right-hand side is a callback on float64 rows
(interp_checker.oracle_rhs); `dtype` is the arithmetic of everything else (float64 or longdouble).

Bounds (u = 2^-53), B[i, k] the bound of interval i's end state:
    adaptive      |xend - x_exact| <= B = 4 accepted64 AbsTol_k + 64 u |x_exact|: every accepted step's local estimate -- the order-7 solution's
                  error, which bounds the propagated order-8 one's -- is at most AbsTol, errors add over the steps; 4 covers their transport
                  along a short interval and another step sequence.  Condition (generator, CPU test): the restatement itself uses at most
                  a quarter, err64 <= accepted64 AbsTol.
    non-adaptive  |xend - longdouble restatement| <= 8 d64 + 16 u |x|, d64 = |float64 restatement - longdouble restatement| (8: the
                  project's margin for generated code's operation order and FMA contraction), step counts exactly numsteps + 1, 0.
    mesh_errors   sum_j B_j |dt_j / h_b| + 8 u |ref|;   mesh_dist inside the interval that bound spans through the monotone power, its effect
                  on max_err included (|max e - max e_ref| <= max B);   tsnd 4 u;   error_max / dist_max bit for bit the column maxima.
    controller    per case the totals of accepted and of rejected steps within max(2, 10 %) of the float64 restatement's."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import interp_checker as ick

_HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(_HERE, "golden", "mesh_integ", "mesh_error_integ.npz")   # (a directory of its own: tests/test_oracle.py takes
                                                                                # every tests/golden/*.npz for a defect vector)
U = 2.0 ** -53
LD = np.longdouble
MODE_CS = ick.MODE_CS
ORDER = {"Trapezoidal": 2, "LGL3": 3, "LGL5": 5, "LGL7": 7}
EPS_F_FACTOR = 8.0
DEFAULTS = dict(def_step=0.01, min_step=0.01 / 10000, max_step=0.01 * 10000, max_step_change=3.0, adaptive=True, max_steps=100000,
                abs_tol=1.0e-12, rel_tol=0.0)


@functools.lru_cache(maxsize=None)
def _uweights(cs):
    return ick.weights(cs)[2]


@functools.lru_cache(maxsize=None)
def tableau(dtype=float):
    t = json.load(open(os.path.join(_HERE, "golden", "rk_tables.json")))["tables"]
    return tuple(np.array(t[k], dtype=float).astype(dtype) for k in ("a", "c", "b", "bhat"))


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def control_at(traj, mode, xv, uv, blk, t, dtype):
    """u(t) of block `blk`: sum_i U_i ups_i(s), s = (t - t_first) / h_block, in `dtype`."""
    cs = MODE_CS[mode]
    K = cs - 1
    Uw = _uweights(cs).astype(dtype)
    rows = traj[blk * K:blk * K + cs]
    tb0 = dtype(rows[0, xv])
    s = (dtype(t) - tb0) / (dtype(rows[-1, xv]) - tb0)
    pw = s ** np.arange(cs - 1, -1, -1).astype(dtype)
    ups = Uw @ pw
    return rows[:, xv + 1:xv + 1 + uv].astype(dtype).T @ ups


def integrate_interval(rhs, traj, mode, blocked, xv, uv, i, opt, dtype=float):
    """-> (xend[xv] in `dtype` (NaN unless status 0), accepted, rejected, status) of node interval i."""
    A, Cc, Bw, Bh = tableau(dtype)
    K = MODE_CS[mode] - 1
    row, nxt = traj[i], traj[i + 1]
    held = uv == 0 or blocked
    x, tc, tf = row[:xv].astype(dtype), dtype(row[xv]), dtype(nxt[xv])
    nan = np.full(xv, np.nan, dtype=dtype)
    if not (np.isfinite(row[:xv + 1]).all() and np.isfinite(nxt[:xv + 1]).all()):
        return nan, 0, 0, 2
    atol, rtol = (np.broadcast_to(np.asarray(opt[k], dtype=float), (xv,)).astype(dtype) for k in ("abs_tol", "rel_tol"))
    H = tf - tc
    numsteps = int(abs(H / dtype(opt["def_step"]))) + 1
    h = dtype(0.9) * (H / dtype(numsteps))
    acc_n = rej_n = 0

    def f(xs, ts):
        y = np.array(row, dtype=float)
        y[:xv], y[xv] = xs.astype(float), float(ts)
        if not held:
            y[xv + 1:xv + 1 + uv] = control_at(traj, mode, xv, uv, i // K, ts, dtype).astype(float)
        return rhs(y[None, :])[0].astype(dtype)

    with np.errstate(all="ignore"):
        while True:
            if acc_n + rej_n >= opt["max_steps"]:
                return nan, acc_n, rej_n, 1
            tnext, last = tc + h, False
            if (tnext - tf >= 0) if H > 0 else (tnext - tf <= 0):
                h, tnext, last = tf - tc, tf, True
            hs = tnext - tc
            Ks = np.zeros((13, xv), dtype=dtype)
            for s in range(13):
                xs = x.copy()
                for j in range(s):
                    xs = xs + A[s - 1][j] * Ks[j]
                ts = tc if s == 0 else tc + Cc[s - 1] * hs
                Ks[s] = f(xs, ts) * hs
            xn, xe = x.copy(), x.copy()
            for s in range(13):
                xn = xn + Bw[s] * Ks[s]
                xe = xe + Bh[s] * Ks[s]
            if not (np.isfinite(h) and np.isfinite(xn).all()):
                return nan, acc_n, rej_n, 2
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
            x, tc = xn, tnext
            if last:
                return x, acc_n, rej_n, 0


def reintegrate(rhs, traj, mode, blocked, xv, uv, opt, dtype=float, intervals=None):
    """(xend[nint, xv] `dtype`, steps[nint, 2], status[nint]) over `intervals` (default: all)."""
    traj = np.asarray(traj, dtype=float)
    ids = range(traj.shape[0] - 1) if intervals is None else intervals
    res = [integrate_interval(rhs, traj, mode, blocked, xv, uv, i, opt, dtype) for i in ids]
    return (np.array([r[0] for r in res], dtype=dtype).reshape(len(res), xv), np.array([[r[1], r[2]] for r in res], dtype=int).reshape(-1, 2),
            np.array([r[3] for r in res], dtype=int))


def estimate(traj, mode, xv, e):
    """(tsnd[nb+1], mesh_errors[xv, nb+1], mesh_dist[xv, nb+1], max_err) in longdouble from e[nint, xv] (ODEPhase.h:630-666)."""
    traj = np.asarray(traj, dtype=float)
    K, p = MODE_CS[mode] - 1, LD(ORDER[mode] + 1)
    nb = (traj.shape[0] - 1) // K
    t = traj[:, xv].astype(LD)
    e = np.asarray(e).astype(LD)
    max_err = e.max() if not np.isnan(e).any() else LD(np.nan)
    me = np.zeros((nb, xv), dtype=LD)
    for b in range(nb):
        t0, tf = t[b * K], t[(b + 1) * K]
        for j in range(K):
            me[b] += e[b * K + j] * abs((t[b * K + j + 1] - t[b * K + j]) / (tf - t0))
    h = np.abs(t[K::K] - t[:-1:K])
    with np.errstate(all="ignore"):
        dist = (me / (h ** p * max_err)[:, None]) ** (1 / p)
    tsnd = np.append((t[:-1:K] - t[0]) / (t[-1] - t[0]), LD(1))
    last = lambda a: np.concatenate([a, a[-1:]], axis=0).T
    return tsnd, last(me), last(dist), max_err


def state_bound(x_exact, accepted64, abs_tol):
    """B[nint, xv] of the adaptive end states."""
    x_exact = np.asarray(x_exact, dtype=float)
    atol = np.broadcast_to(np.asarray(abs_tol, dtype=float), (x_exact.shape[1],))
    return 4.0 * np.asarray(accepted64, dtype=float)[:, None] * atol[None, :] + 64.0 * U * np.abs(x_exact)


def compare_states(xend, ref, bound, what=""):
    """asserts |xend - ref| <= bound everywhere; returns the worst ratio."""
    d = np.abs(np.asarray(xend).astype(LD) - np.asarray(ref).astype(LD)).astype(float)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    bad = np.argwhere(~(d <= bound))
    assert bad.size == 0, (f"{what}: end state outside its bound at {len(bad)} entries, worst ratio {np.nanmax(ratio):.3g}; first (interval, "
                           f"state) {tuple(bad[0])}: got {np.asarray(xend)[tuple(bad[0])]!r} ref {np.asarray(ref)[tuple(bad[0])]!r} "
                           f"bound {bound[tuple(bad[0])]:.3e}")
    return float(ratio.max(initial=0.0))


def compare_estimate(got, traj, mode, xv, x_ref, B, what=""):
    """got = (tsnd, mesh_errors[xv, nb+1], mesh_dist[xv, nb+1], error_max, dist_max); the reference estimate is formed from
    e_ref = |x_ref - next node| and every end state may be off by B[nint, xv].  Returns the worst ratios (tsnd, mesh_errors, mesh_dist)."""
    traj = np.asarray(traj, dtype=float)
    gt, gerr, gdist, gemax, gdmax = (np.asarray(a, dtype=float) for a in got)
    K, p = MODE_CS[mode] - 1, LD(ORDER[mode] + 1)
    nb = (traj.shape[0] - 1) // K
    e_ref = np.abs(np.asarray(x_ref).astype(LD) - traj[1:, :xv].astype(LD))
    rt, rerr, rdist, rmax = estimate(traj, mode, xv, e_ref)
    assert gt.shape == rt.shape and gerr.shape == rerr.shape == gdist.shape, what
    worst_t = float(np.abs(gt - rt.astype(float)).max() / (4.0 * U))
    assert worst_t <= 1.0, f"{what}: tsnd off by {worst_t * 4:.2f} u"
    t = traj[:, xv].astype(LD)
    w = np.abs(np.diff(t)).reshape(nb, K) / np.abs(t[K::K] - t[:-1:K])[:, None]          # |dt_j / h_b|
    Bme = (np.asarray(B).astype(LD).reshape(nb, K, xv) * w[:, :, None]).sum(axis=1)      # [nb, xv]
    Bme = np.concatenate([Bme, Bme[-1:]], axis=0).T
    berr = (Bme + 8.0 * U * np.abs(rerr)).astype(float)
    derr = np.abs(gerr.astype(LD) - rerr).astype(float)
    bad = np.argwhere(~(derr <= berr))
    worst_e = float((derr / berr).max())
    assert bad.size == 0, (f"{what}: mesh_errors outside the bound at {len(bad)} entries, worst ratio {worst_e:.3g}; first (state, block) "
                           f"{tuple(bad[0])}: got {gerr[tuple(bad[0])]!r} ref {float(rerr[tuple(bad[0])])!r} bound {berr[tuple(bad[0])]:.3e}")
    Bmax = np.asarray(B).astype(LD).max()
    h = np.abs(t[K::K] - t[:-1:K])
    hp = np.append(h, h[-1]) ** p
    lo = ((np.maximum(rerr - Bme, 0) / (hp * (rmax + Bmax))[None, :]) ** (1 / p) * (1 - 8 * U)).astype(float)
    hi = (((rerr + Bme) / (hp * np.maximum(rmax - Bmax, np.finfo(float).tiny))[None, :]) ** (1 / p) * (1 + 8 * U)).astype(float)
    rd = rdist.astype(float)
    bad = np.argwhere(~((gdist >= lo) & (gdist <= hi)))
    with np.errstate(invalid="ignore", divide="ignore"):
        up = np.where(gdist > rd, (gdist - rd) / (hi - rd), 0.0)
        dn = np.where(gdist < rd, (rd - gdist) / (rd - lo), 0.0)
    worst_d = float(np.nanmax(np.maximum(up, dn), initial=0.0))
    assert bad.size == 0, (f"{what}: mesh_dist outside its interval at {len(bad)} entries, worst ratio {worst_d:.3g}; first (state, block) "
                           f"{tuple(bad[0])}: got {gdist[tuple(bad[0])]!r} not in [{lo[tuple(bad[0])]!r}, {hi[tuple(bad[0])]!r}]")
    check_column_maxima(gerr, gdist, gemax, gdmax, what)
    return worst_t, worst_e, worst_d


def check_column_maxima(gerr, gdist, gemax, gdmax, what=""):
    """error_max / dist_max: bit for bit the maxima of the device's own columns (numpy's maximum: a NaN entry makes it NaN)."""
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(gemax, np.abs(gerr).max(axis=0), err_msg=f"{what}: error_max")
        np.testing.assert_array_equal(gdmax, np.abs(gdist).max(axis=0), err_msg=f"{what}: dist_max")


def compare_step_totals(steps, steps64, what=""):
    """the controller is the reference's: totals of accepted and of rejected steps within max(2, 10 %) of the restatement's"""
    for col, name in ((0, "accepted"), (1, "rejected")):
        got, ref = int(np.asarray(steps)[:, col].sum()), int(np.asarray(steps64)[:, col].sum())
        assert abs(got - ref) <= max(2, 0.1 * ref), f"{what}: {name} steps {got} against the restatement's {ref}"


# ------------------------------------------------------------------------------------------------ the fixture
_CACHE = None


def fixture():
    """(meta, cases): cases[name] the case's meta data (ode, mode, blocked, sizes, options) with arrays 'traj', 'x_exact' [nint, xv],
    'steps64' [nint, 2], 'err64' [nint, xv], 'xld' [nint, xv] longdouble (the longdouble restatement) and 'd64' [nint, xv]."""
    global _CACHE
    if _CACHE is None:
        z = np.load(FIXTURE)
        meta = json.loads(str(z["meta"]))
        cases = {}
        for c in meta["cases"]:
            d = dict(c)
            for a in ("traj", "x_exact", "steps64", "err64", "d64"):
                d[a] = z[f"{c['name']}.{a}"]
            d["xld"] = z[f"{c['name']}.xld_hi"].astype(LD) + z[f"{c['name']}.xld_lo"].astype(LD)
            cases[c["name"]] = d
        _CACHE = (meta, cases)
    return _CACHE


def case_names():
    return list(fixture()[1]) if os.path.exists(FIXTURE) else []


def case_options(case):
    return options(**case["options"])
