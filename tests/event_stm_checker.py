"""Independent restatement of the batched propagation with events AND the state-transition matrix
(csrc/propagate_event_stm_kernels.h behind asset_hip_propagate_events_stm and ``integrate_events_stm*``), its references and bounds.
Pure numpy; nothing here touches the code under test.

What is restated.  The event state machine of tests/event_checker.py (``propagate_events``: detection after every accepted step, stop
counts, location by ONE step of size theta h from the start of the bracketing step, the root finder PLAIN BISECTION run down to the
contract's termination rule) with the column carry of tests/propagate_checker.py: every column of S = d x / d [x0, u, p] rides through
the same stages of the same trips, KC_s = h J(X_s) W_s -- through the accepted steps, and through a location's theta h step with theta
held, so that every located occurrence has the S of its stored state.  The state's stages evaluate f, not fj.

References.  CLOSED-FORM VARIATIONAL FLOWS, in longdouble, at ANY time -- a stopped propagation ends at the end of an accepted step, so
its end time depends on the step sequence and a stored value at a fixed time cannot serve (the reason event_checker compares stopped
end states "at the end time that was returned"):
    oscillator   S(t) = the rotation by t - t0;
    freefall     tau = t - t0:  S_x = [[1, tau], [0, 1]], gravity column [-tau^2 / 2, -tau].
Cases that do not stop are pinned bit for bit to calls the existing 50-digit fixtures hold (tests/test_gpu_propagate_events_stm.py).
Where there is no closed form (twobody_lt, the shape ODEs) the reference is the float64 restatement, at twice the bounds.

Bounds: propagate_checker.state_bound, stm_bound and time_column_bounds as they are.  eS is the largest |S_restated - S_closed| over
the float64 restatement at AbsTol x {1/2, 1, 2}, each at its own returned time -- the end of the propagation and every located
occurrence (``eS_closed``).  Without a closed form the closed form's place is taken by the variational flow integrated to the item's own
time at a thousandth of the tolerance (``eS_items``), together with the estimate of tests/test_gpu_propagate.py from the restated STM's
own sensitivity to the tolerance on the arc [t0, t_end] (``eS_estimated``); eS is the larger.  None of these is measured against the
device."""
from __future__ import annotations

import numpy as np

import event_checker as eck
import integ_checker as gck
import propagate_checker as pck

U = gck.U
LD = gck.LD
TOL_FACTORS = pck.TOL_FACTORS


# ------------------------------------------------------------------------------------------------ Jacobians of the systems
def _osc_J(y):
    return np.array([[0, 1, 0], [-1, 0, 0]], dtype=y.dtype)


def _fall_J(y):
    return np.array([[0, 1, 0, 0], [0, 0, 0, -1]], dtype=y.dtype)


def complex_step_J(f):
    """y[N] float64 -> J[n, N] of a right-hand side written with numpy operations that take complex arguments"""
    def J(y):
        y = np.asarray(y, dtype=float)
        out = np.zeros((f(y).size, y.size))
        for i in range(y.size):
            z = y.astype(complex)
            z[i] += 1.0e-30j
            out[:, i] = f(z).imag / 1.0e-30
        return out
    return J


def jacobian_of(system):
    """J(y) of a system of event_checker.SYSTEMS: closed form in the dtype of y, or by the complex step in float64"""
    return {"oscillator": _osc_J, "freefall": _fall_J}.get(system) or complex_step_J(eck.SYSTEMS[system]["f"])


# ------------------------------------------------------------------------------------------------ closed-form variational flows
def closed_S(system, row, t, dtype=LD):
    """S[n, C] = d x(t) / d [x0, u, p] of the exact flow from `row`, in `dtype`"""
    row = np.asarray(row).astype(dtype)
    tau = dtype(t) - row[2]
    if system == "oscillator":
        c, s = np.cos(tau), np.sin(tau)
        return np.array([[c, s], [-s, c]], dtype=dtype)
    if system == "freefall":
        one, zero = dtype(1), dtype(0)
        return np.array([[one, tau, -tau * tau / 2], [zero, one, -tau]], dtype=dtype)
    raise KeyError(system)


CLOSED = ("oscillator", "freefall")


# ------------------------------------------------------------------------------------------------ the restatement
def rk_step_stm(f, J, row, x, Sm, E, tc, hs, tab, dtype):
    """(order-8 state, order-7 state, S after the step) of one 13-stage step of size hs from (x, tc) with the columns Sm[n, C]"""
    A, Cc, Bw, Bh = tab
    n = x.size
    y = np.asarray(row).astype(dtype).copy()
    Ks = np.zeros((13, n), dtype=dtype)
    Kc = np.zeros((13,) + Sm.shape, dtype=dtype)
    for s in range(13):
        xst, Ws = x.copy(), Sm.copy()
        for q in range(s):
            xst = xst + A[s - 1][q] * Ks[q]
            Ws = Ws + A[s - 1][q] * Kc[q]
        y[:n], y[n] = xst, (tc if s == 0 else tc + Cc[s - 1] * hs)
        Ks[s] = f(y) * hs
        W = E.copy()
        W[:n] = Ws
        Kc[s] = (np.asarray(J(y)).astype(dtype) @ W) * hs
    xn, xe, Sn = x.copy(), x.copy(), Sm.copy()
    for s in range(13):
        xn = xn + Bw[s] * Ks[s]
        xe = xe + Bh[s] * Ks[s]
        Sn = Sn + Bw[s] * Kc[s]
    return xn, xe, Sn


def propagate_events_stm(f, J, gs, row, tf, direction, stop, opt, event_tol=1.0e-6, max_locs=8, dtype=float):
    """One problem -> the dict of event_checker.propagate_events, with S[n, C] (NaN unless status 0) at the end of the propagation
    and locs[j][k]["S"] at every stored occurrence."""
    tab = gck.tableau(dtype)
    row = np.asarray(row, dtype=float)
    n, ne, N = f(row.astype(dtype)).size, len(gs), row.size
    Cn = N - 1
    out = dict(x=np.full(n, np.nan, dtype=dtype), S=np.full((n, Cn), np.nan, dtype=dtype), t_end=float(tf), stopped=-1, count=[0] * ne,
               locs=[[] for _ in range(ne)], steps=(0, 0), status=0, accepted_steps=[])
    if not (np.isfinite(row[:n + 1]).all() and np.isfinite(tf)):
        out["status"] = 2
        return out
    x, tc, tfd = row[:n].astype(dtype), dtype(row[n]), dtype(tf)
    Sm = np.zeros((n, Cn), dtype=dtype)
    Sm[:, :n] = np.eye(n, dtype=dtype)
    E = np.zeros((N, Cn), dtype=dtype)                 # unit entries of the control and parameter columns, ODE-input space
    for c in range(n, Cn):
        E[c + 1, c] = 1
    H = tfd - tc
    if H == 0:
        out["x"], out["S"] = x, Sm
        return out
    rowd = row.astype(dtype)
    tol = dtype(event_tol)

    def gall(xs, ts):
        y = rowd.copy()
        y[:n], y[n] = xs, ts
        return [g(y) for g in gs]

    atol, rtol = (np.broadcast_to(np.asarray(opt[k], dtype=float), (n,)).astype(dtype) for k in ("abs_tol", "rel_tol"))
    numsteps = int(abs(H / dtype(opt["def_step"]))) + 1
    h = dtype(0.9) * (H / dtype(numsteps))
    acc_n = rej_n = 0
    gp = gall(x, tc)
    with np.errstate(all="ignore"):
        while True:
            if acc_n + rej_n >= opt["max_steps"]:
                out["status"] = 1
                break
            tnext, last = tc + h, False
            if (tnext - tfd >= 0) if H > 0 else (tnext - tfd <= 0):
                h, tnext, last = tfd - tc, tfd, True
            hs = tnext - tc
            xn, xe, Sn = rk_step_stm(f, J, row, x, Sm, E, tc, hs, tab, dtype)
            if not (np.isfinite(h) and np.isfinite(xn).all()):
                out["status"] = 2
                break
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
                if (err - acc) > 0 and not hit_min:
                    rej_n += 1
                    continue
            acc_n += 1
            out["accepted_steps"].append((float(tc), float(tnext)))
            gn = gall(xn, tnext)
            for j in range(ne):
                if gp[j] * gn[j] < 0 and (direction[j] == 0 or (gn[j] > 0 if direction[j] > 0 else gn[j] < 0)):
                    out["count"][j] += 1
                    if out["count"][j] <= max_locs:
                        a, b, Ga = dtype(0), dtype(1), gp[j]
                        for _ in range(eck.BISECT_CAP):
                            final = (b - a) / 2 * abs(hs) < tol
                            th = (a + b) / 2
                            xt, _, St = rk_step_stm(f, J, row, x, Sm, E, tc, th * hs, tab, dtype)
                            G = gall(xt, tc + th * hs)[j]
                            if final or abs(G) < tol:
                                break
                            if (G < 0) == (Ga < 0):
                                a, Ga = th, G
                            else:
                                b = th
                        out["locs"][j].append(dict(x=xt, S=St, t=tc + th * hs, resid=G, conv=bool(final or abs(G) < tol), h=float(hs)))
                    if stop[j] > 0 and out["count"][j] == stop[j] and out["stopped"] < 0:
                        out["stopped"] = j
            x, Sm, tc, gp = xn, Sn, tnext, gn
            if last or out["stopped"] >= 0:
                break
    out["steps"] = (acc_n, rej_n)
    if out["status"] == 0:
        out["x"], out["S"] = x, Sm
    out["t_end"] = float(tc) if out["stopped"] >= 0 else float(tf)
    return out


def restate_case(case, tol_factor=1.0, dtype=float, J=None, sysd=None):
    """The restatement of every problem of a case in the form of event_checker (system, events, direction, stop, rows, tfs, options,
    event_tol, max_locs); tol_factor scales AbsTol.  `sysd`, `J`: a system event_checker.SYSTEMS does not hold, and its Jacobian."""
    sysd = sysd or eck.SYSTEMS[case["system"]]
    gs = [sysd["events"][e][0] for e in case["events"]]
    opt = eck.case_options(case)
    opt["abs_tol"] = np.asarray(opt["abs_tol"], dtype=float) * tol_factor
    J = J or jacobian_of(case["system"])
    return [propagate_events_stm(sysd["f"], J, gs, r, t, case["direction"], case["stop"], opt, case["event_tol"], case["max_locs"], dtype)
            for r, t in zip(case["rows"], case["tfs"])]


# ------------------------------------------------------------------------------------------------ bounds
def items_of(r):
    """[(t, x, S)] of one restated problem: the end of the propagation, then every stored occurrence in the order (event, occurrence)"""
    return [(r["t_end"], r["x"], r["S"])] + [(loc["t"], loc["x"], loc["S"]) for lj in r["locs"] for loc in lj]


def eS_closed(case):
    """eS[m]: the largest |S_restated - S_closed| over the float64 restatement at AbsTol x {1/2, 1, 2}, each item at its own returned
    time.  Returns (eS, the restatement at AbsTol itself)."""
    assert case["system"] in CLOSED
    m = case["rows"].shape[0]
    eS, at_one = np.zeros(m), None
    for fac in TOL_FACTORS:
        res = restate_case(case, fac)
        if fac == 1.0:
            at_one = res
        for i, r in enumerate(res):
            assert r["status"] == 0
            for t, _, Sm in items_of(r):
                ref = closed_S(case["system"], case["rows"][i], LD(float(t)))
                eS[i] = max(eS[i], float(np.abs(np.asarray(Sm).astype(LD) - ref).max()))
    return eS, at_one


def eS_estimated(f, fj, row, t_end, opt):
    """Without a closed form (tests/test_gpu_propagate.py: _Problems.check): the local error is proportional to AbsTol, so
    S(AbsTol) - S(AbsTol / 2) is about half the error of S(AbsTol): eS = 2 max(|S(AbsTol / 2) - S|, |S(2 AbsTol) - S|) on the arc
    [t0, t_end]; dS = |S - longdouble restatement| covers arcs whose step sequence does not depend on the tolerance.  (eS, dS[n, C])"""
    S1 = pck.propagate(f, fj, row, t_end, 1, opt, stm=True)["S"]
    eS = 0.0
    for fac in (0.5, 2.0):
        o = dict(opt, abs_tol=fac * np.asarray(opt["abs_tol"]))
        eS = max(eS, 2.0 * float(np.abs(pck.propagate(f, fj, row, t_end, 1, o, stm=True)["S"] - S1).max()))
    ld = pck.propagate(f, fj, row, t_end, 1, opt, dtype=LD, stm=True)["S"]
    return eS, np.abs(S1.astype(LD) - ld).astype(float)


def tight_options(opt, tight):
    """`tight` times AbsTol, and half the default and the largest step: an arc whose steps are all clamped is refined too (2^-8)"""
    return dict(opt, abs_tol=tight * np.asarray(opt["abs_tol"], dtype=float), def_step=0.5 * opt["def_step"], max_step=0.5 * opt["max_step"])


def eS_items(f, fj, row, items, opt, tight=1.0e-3):
    """What the tolerance's sensitivity does not see: a location's theta h step is not under error control, and an arc whose steps are
    all clamped (MaxStepChange, the first step) has the same step sequence at every tolerance.  The error of every restated item
    (items_of) is therefore also measured directly, against the variational flow integrated to THAT ITEM'S OWN TIME at a tolerance
    `tight` times AbsTol (its own error is that fraction of the measured one): the largest |S_item - S_tight(t_item)|."""
    o = tight_options(opt, tight)
    e = 0.0
    for t, _, Sm in items:
        ref = pck.propagate(f, fj, row, float(t), 1, o, stm=True)
        assert ref["status"] == 0
        e = max(e, float(np.abs(np.asarray(Sm, dtype=float) - ref["S"]).max()))
    return e


def jac_columns(J, n):
    """(S[..., n, C], d / d t0 [..., n], d / d t [..., n]) of J[..., n, N + 1] with columns [x0 | t0 | u | p | t]"""
    J = np.asarray(J)
    N = J.shape[-1] - 1
    return np.concatenate([J[..., :n], J[..., n + 1:N]], axis=-1), J[..., n], J[..., N]


def compare_item_closed(system, row, t, x, Jm, eS, B, what):
    """One item of the device (its returned time t, its state x, its J[n, N + 1]) against the closed forms AT THAT TIME: the S columns
    within stm_bound, the time columns within time_column_bounds.  Returns the worst ratio."""
    sysd = eck.SYSTEMS[system]
    n = sysd["n"]
    S, d0, df = jac_columns(Jm, n)
    Sx = closed_S(system, row, LD(float(t)))
    y0 = np.asarray(row, dtype=float).astype(LD)
    f0 = sysd["f"](y0)
    ye = y0.copy()
    ye[:n], ye[n] = eck.exact_flow(system, row, LD(float(t))), LD(float(t))
    dtf_exact = sysd["f"](ye)
    Jxf_abs = np.abs(np.asarray(jacobian_of(system)(ye), dtype=float)[:, :n])
    Sx64 = Sx.astype(float)
    w = pck.compare(S[None], Sx[None], pck.stm_bound(Sx64[None], np.array([eS])), f"{what}: S")
    b0, bf = pck.time_column_bounds(Sx64[None], np.array([eS]), f0.astype(float)[None], Jxf_abs[None], np.asarray(B, dtype=float)[None],
                                    dtf_exact.astype(float)[None])
    w = max(w, pck.compare(d0[None], (-(Sx[:, :n] @ f0))[None], b0, f"{what}: d x / d t0"))
    return max(w, pck.compare(df[None], dtf_exact[None], bf, f"{what}: d x / d t"))


def time_shift(f, fj, row, t_from, t_to, opt, tight=1.0e-3):
    """S(t_to) - S(t_from) of the variational flow, both integrated at a tolerance `tight` times AbsTol: what carries a restated S
    from the time the restatement returned to the time the device returned"""
    if float(t_from) == float(t_to):
        return 0.0
    o = tight_options(opt, tight)
    a, b = (pck.propagate(f, fj, row, float(t), 1, o, stm=True) for t in (t_from, t_to))
    assert a["status"] == 0 and b["status"] == 0
    return b["S"] - a["S"]


def compare_item_restated(f, Jfun, row, n, ref, got, eS, dS, B, what, shift=0.0):
    """Where there is no closed form: one item of the device, got = (t, J[n, N + 1]), against the float64 restatement's ref = (t, x, S),
    at TWICE the bounds -- each side is within 4 eS + 16 u |S| (+ the rounding term 8 dS / 2 of an arc whose step sequence does not
    depend on the tolerance) of the exact S AT ITS OWN TIME.  The two times differ (another root finder; an error estimate at rounding
    level that gives another step and with it another end time), so the restated S is first carried to the device's time by
    `shift` = time_shift(...).  The time columns through their closed forms, as propagate_checker.time_column_bounds forms them:
    d / d t0 = -S_x f(x0), and the last column f at the item's state -- within B (one side's state bound) of the exact state on each
    side, hence 2 B, and moved by at most 2 |f| |t_got - t_ref| in the state and 2 |d f / d t| |t_got - t_ref| (first order, the
    factor 2 for the remainder).  Returns the worst ratio."""
    row = np.asarray(row, dtype=float)
    t_r, x_r, S_r = float(ref[0]), np.asarray(ref[1], dtype=float), np.asarray(ref[2], dtype=float)
    t_g, J_g = float(got[0]), np.asarray(got[1], dtype=float)
    S, d0, df = jac_columns(J_g, n)
    y = row.copy()
    y[:n], y[n] = x_r, t_r
    Jy, f_r, f0 = np.asarray(Jfun(y), dtype=float), np.asarray(f(y), dtype=float), np.asarray(f(row), dtype=float)
    dt = abs(t_g - t_r)
    S_r = S_r + shift
    bS = 2.0 * pck.stm_bound(S_r[None], np.array([eS]))[0] + 8.0 * np.asarray(dS, dtype=float)
    w = pck.compare(S, S_r, bS, f"{what}: S against the restatement")
    b0 = bS[:, :n] @ np.abs(f0) + 16.0 * U * (np.abs(S_r[:, :n]) @ np.abs(f0))
    w = max(w, pck.compare(d0, -(S_r[:, :n] @ f0), b0, f"{what}: d x / d t0"))
    bf = np.abs(Jy[:, :n]) @ (2.0 * np.asarray(B, dtype=float) + 2.0 * np.abs(f_r) * dt) + 2.0 * np.abs(Jy[:, n]) * dt + 64.0 * U * np.abs(f_r).max()
    return max(w, pck.compare(df, f_r, bf, f"{what}: d x / d t"))
