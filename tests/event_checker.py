"""Independent restatement of the batched propagation with events (csrc/propagate_event_kernels.h behind asset_hip_propagate_events and
asset_asrl_amd/integrator.py), its error bounds, and the loader of the 50-digit fixture tests/golden/propagate_events/events.npz
(tests/golden/make_golden_propagate_events.py).  Pure numpy; nothing here touches the code under test.

What is restated.  The step rule of tests/propagate_checker.py / tests/integ_checker.py (their tableau, options and defaults are
imported) for ONE initial-value problem with held controls and parameters and ns = 1.  An event is (g, direction, stop); after every
ACCEPTED step event j occurred iff g_j(prev) g_j(next) < 0 and (direction == 0 or g_j(next) has the sign of direction); every event is
examined for the step; when an event with stop = k > 0 reaches its k-th occurrence the propagation ends at the END of that accepted
step (`stopped`: the lowest such event).  An occurrence is located on the integrator: x(theta) is ONE step of size theta h from the
start of the bracketing step, G(theta) = g(x(theta), t_i + theta h, u, p).  The root finder here is PLAIN BISECTION in theta, run down to
the contract's termination rule -- |G| < EventTol, or the bracket's half-width in time < EventTol (the trial is then the midpoint) --
whatever number of evaluations that takes: nothing below rests on the device's method.  The first max_locs occurrences of an event
are located, later ones counted.  The right-hand side and the events are numpy callbacks on rows [x, t, u, p] in `dtype`.

Bounds (none measured against the code under test).  B = propagate_checker.state_bound(S_max, accepted64 + 1, AbsTol): a local error of
at most the tolerance per accepted step -- one more for the location's sub-step -- carried by the flow's sensitivity.
    event time    dt = EventTol + 2 (EventTol + sum_k |dg/dx_k| B_k) / |gdot(t*)|: the located point has |G| < EventTol or lies within
                  EventTol of the root of G; G differs from g on the exact flow by at most sum |dg/dx| B; the 2 covers the variation of
                  gdot across the bracket, true when |gddot| (bracketing step) <= |gdot(t*)| / 2 (asserted by the generator and by
                  tests/test_propagate_events_cpu.py for every fixture event).
    event state   B_k + 2 |f_k(x*, t*)| dt.
    counts        equal to the exact ones: no accepted step of the restatement spans more than half the gap between neighbouring
                  crossings (asserted the same way; MaxStepSize is chosen for it).
    end state     not stopped: |xf - x_exact(tf)| <= B.  Stopped: the end time depends on the step sequence, so xf is compared with the
                  exact flow AT THE END TIME THAT WAS RETURNED, within B, and that time lies past the stopping event's by less than
                  MaxStepSize (and not before it by more than dt).
QUARTER.  The generator and tests/test_propagate_events_cpu.py hold the float64 restatement to a quarter of each bound, as the other
propagation fixtures do.  The EventTol terms of dt are not an error estimate but what the termination rule ALLOWS: a root finder that
stops at |G| just below EventTol is off by EventTol / |gdot| in time, a third of dt, whatever the integration error is.  A quarter of
the bound is therefore asked of the restatement run with a QUARTER OF EventTol (every ingredient of the bound at a quarter: the
finder's tolerance, and the integration error against B / 4); run with EventTol itself it is held to the whole bound.
Recorded, so that the argument can be checked: the float64 restatement run at EventTol itself against a QUARTER of the bounds misses in
six of the ten fixture cases -- time ratio (error / (dt / 4)) of the first occurrence that misses: osc_any_stop0 1.10,
osc_up_stop1 1.10, osc_down_stop3 1.46, fall_impact 1.94, kepler_apsides 1.20, kepler_backward 1.03 (state ratios there 0.51 .. 0.97) --
all of them in the event time of an occurrence whose search ended
on |G| < EventTol with |G| above three quarters of EventTol.  (Against the whole bounds the same run
uses 0.27, 0.27, 0.37, 0.14, 0.21, 0.49, 0.37, 0.011, 0.26 and 0.11 of them, case by case in the fixture's order; at EventTol / 4
against a quarter: 0.34, 0.24, 0.24, 0.40, 0.12, 0.84, 0.36, 0.0073, 0.30, 0.34.)
The 50-digit values are stored rounded to float64 (a relative 2^-53, far below every bound above)."""
from __future__ import annotations

import json
import os

import numpy as np

import integ_checker as gck
import propagate_checker as pck

_HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(_HERE, "golden", "propagate_events", "events.npz")
U = gck.U
LD = gck.LD
BISECT_CAP = 400          # the restatement's own cap on bisection steps (not the device's MaxEventIters)


# ------------------------------------------------------------------------------------------------ the systems of the fixture
# name -> (n, uv, pv, f(y) -> [n], events {name: (g(y), dg/dx(y) -> [n])}); y = [x, t, u, p] in any float dtype
def _osc_f(y):
    return np.array([y[1], -y[0]], dtype=y.dtype)


def _fall_f(y):
    return np.array([y[1], -y[3]], dtype=y.dtype)


def _kepler_f(y):
    r3 = (y[0] * y[0] + y[1] * y[1] + y[2] * y[2]) ** y.dtype.type(1.5)
    return np.array([y[3], y[4], y[5], -y[0] / r3 + y.dtype.type(0.01) * y[7], -y[1] / r3 + y.dtype.type(0.01) * y[8],
                     -y[2] / r3 + y.dtype.type(0.01) * y[9]], dtype=y.dtype)


def _vdp_f(y):
    x0, x1, t, u, mu = y[0], y[1], y[2], y[3], y[4]
    return np.array([x1, mu * (1 - x0 * x0) * x1 - x0 + u * np.exp(-t / 10)], dtype=y.dtype)


def _shape_f(n, m, p):
    """tests/helpers.py: make_shape, as numpy"""
    def f(y):
        x, t, u, par = y[:n], y[n], y[n + 1:n + 1 + m], y[n + 1 + m:]
        out = []
        for k in range(n):
            v = np.sin(x[(k + 1) % n]) * x[(k + 2) % n]
            if m > 0:
                v = v * u[k % m]
            v = v - x[k] / 2 + y.dtype.type(0.3) * np.cos(t) * x[(k + 3) % n]
            if m > 0:
                v = v + y.dtype.type(0.1) * u[(k + 1) % m] * u[(k + 1) % m]
            if p > 0:
                v = v + par[0] * x[k] * x[(k + 1) % n] + par[p - 1] * np.cos(t)
            out.append(v)
        return np.array(out, dtype=y.dtype)
    return f


SHAPE_LEVEL = 0.25        # the event of the shape ODE: x0 - SHAPE_LEVEL


def _unit(n, k):
    return lambda y: np.eye(n, dtype=y.dtype)[k]


SYSTEMS = {
    "oscillator": dict(n=2, uv=0, pv=0, f=_osc_f, events={
        "x0": (lambda y: y[0], _unit(2, 0)),
        "x0m": (lambda y: y[0] - y.dtype.type(0.01), _unit(2, 0)),
        "x1": (lambda y: y[1], _unit(2, 1))}),
    "freefall": dict(n=2, uv=0, pv=1, f=_fall_f, events={"height": (lambda y: y[0], _unit(2, 0))}),
    "twobody_lt": dict(n=6, uv=3, pv=0, f=_kepler_f, events={
        "rv": (lambda y: y[0] * y[3] + y[1] * y[4] + y[2] * y[5], lambda y: np.concatenate([y[3:6], y[0:3]])),
        "pos": (lambda y: y[0] * y[0] + y[1] * y[1] + y[2] * y[2], lambda y: np.concatenate([2 * y[0:3], 0 * y[0:3]]))}),
    "vanderpol": dict(n=2, uv=1, pv=1, f=_vdp_f, events={"x1": (lambda y: y[1], _unit(2, 1)),
                                                         "pos": (lambda y: y[0] * y[0] + 1, lambda y: np.array([2 * y[0], 0 * y[0]]))}),
    "shape_11_4_2": dict(n=11, uv=4, pv=2, f=_shape_f(11, 4, 2), events={"x0c": (lambda y: y[0] - y.dtype.type(SHAPE_LEVEL), _unit(11, 0))}),
}


def exact_flow(system: str, row, t, dtype=LD):
    """x(t) of the closed-form systems (oscillator, freefall, twobody_lt with zero thrust) in `dtype`."""
    row = np.asarray(row).astype(dtype)
    t = dtype(t)
    if system == "oscillator":
        d = t - row[2]
        c, s = np.cos(d), np.sin(d)
        return np.array([row[0] * c + row[1] * s, -row[0] * s + row[1] * c], dtype=dtype)
    if system == "freefall":
        d = t - row[2]
        return np.array([row[0] + row[1] * d - row[3] * d * d / 2, row[1] - row[3] * d], dtype=dtype)
    if system == "twobody_lt":
        # Lagrange coefficients through the change of eccentric anomaly dE:  n dt = dE - (1 - r0 / a) sin dE + sig (1 - cos dE),
        # sig = r0 . v0 / sqrt(a)   (mu = 1)
        assert not np.any(row[7:10] != 0)
        r0v, v0v = row[0:3], row[3:6]
        r0, v2, rv = np.sqrt(r0v @ r0v), v0v @ v0v, r0v @ v0v
        a = 1 / (2 / r0 - v2)
        sa = np.sqrt(a)
        nm, sig, dt = 1 / (a * sa), rv / sa, t - row[6]
        M = nm * dt
        dE = M
        for _ in range(60):
            F = dE - (1 - r0 / a) * np.sin(dE) + sig * (1 - np.cos(dE)) - M
            dF = 1 - (1 - r0 / a) * np.cos(dE) + sig * np.sin(dE)
            step = F / dF
            dE = dE - step
            if abs(step) < 4 * np.finfo(dtype).eps * max(dtype(1), abs(dE)):
                break
        cE, sE = np.cos(dE), np.sin(dE)
        r = a + (r0 - a) * cE + sig * sa * sE
        fl, gl = 1 - a * (1 - cE) / r0, dt - (dE - sE) / nm
        fd, gd = -sa * sE / (r * r0), 1 - a * (1 - cE) / r
        return np.concatenate([fl * r0v + gl * v0v, fd * r0v + gd * v0v]).astype(dtype)
    raise KeyError(system)


# ------------------------------------------------------------------------------------------------ the restatement
def rk_step(f, row, x, tc, hs, tab, dtype):
    """(order-8 state, order-7 state) of one 13-stage step of size hs from (x, tc)."""
    A, Cc, Bw, Bh = tab
    n = x.size
    y = np.asarray(row).astype(dtype).copy()
    Ks = np.zeros((13, n), dtype=dtype)
    for s in range(13):
        xst = x.copy()
        for q in range(s):
            xst = xst + A[s - 1][q] * Ks[q]
        y[:n], y[n] = xst, (tc if s == 0 else tc + Cc[s - 1] * hs)
        Ks[s] = f(y) * hs
    xn, xe = x.copy(), x.copy()
    for s in range(13):
        xn = xn + Bw[s] * Ks[s]
        xe = xe + Bh[s] * Ks[s]
    return xn, xe


def propagate_events(f, gs, row, tf, direction, stop, opt, event_tol=1.0e-6, max_locs=8, dtype=float):
    """One problem -> dict(x[n] (NaN unless status 0), t_end, stopped, count[ne], locs[ne] = lists of dict(x, t, resid, conv, h) --
    h the bracketing step --, steps (accepted, rejected), status, accepted_steps = [(t_i, t_i+1)])."""
    tab = gck.tableau(dtype)
    row = np.asarray(row, dtype=float)
    n, ne = f(row.astype(dtype)).size, len(gs)
    out = dict(x=np.full(n, np.nan, dtype=dtype), t_end=float(tf), stopped=-1, count=[0] * ne, locs=[[] for _ in range(ne)], steps=(0, 0),
               status=0, accepted_steps=[])
    if not (np.isfinite(row[:n + 1]).all() and np.isfinite(tf)):
        out["status"] = 2
        return out
    x, tc, tfd = row[:n].astype(dtype), dtype(row[n]), dtype(tf)
    H = tfd - tc
    if H == 0:
        out["x"] = x
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
            xn, xe = rk_step(f, row, x, tc, hs, tab, dtype)
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
                        for _ in range(BISECT_CAP):
                            final = (b - a) / 2 * abs(hs) < tol
                            th = (a + b) / 2
                            xt, _ = rk_step(f, row, x, tc, th * hs, tab, dtype)
                            G = gall(xt, tc + th * hs)[j]
                            if final or abs(G) < tol:
                                break
                            if (G < 0) == (Ga < 0):
                                a, Ga = th, G
                            else:
                                b = th
                        out["locs"][j].append(dict(x=xt, t=tc + th * hs, resid=G, conv=bool(final or abs(G) < tol), h=float(hs)))
                    if stop[j] > 0 and out["count"][j] == stop[j] and out["stopped"] < 0:
                        out["stopped"] = j
            x, tc, gp = xn, tnext, gn
            if last or out["stopped"] >= 0:
                break
    out["steps"] = (acc_n, rej_n)
    if out["status"] == 0:
        out["x"] = x
    out["t_end"] = float(tc) if out["stopped"] >= 0 else float(tf)
    return out


def restate_case(case, dtype=float, tol_factor=1.0):
    """The restatement of every problem of a fixture case; tol_factor scales EventTol (QUARTER, below)."""
    sysd = SYSTEMS[case["system"]]
    gs = [sysd["events"][e][0] for e in case["events"]]
    opt = case_options(case)
    return [propagate_events(sysd["f"], gs, r, t, case["direction"], case["stop"], opt, case["event_tol"] * tol_factor, case["max_locs"],
                             dtype) for r, t in zip(case["rows"], case["tfs"])]


# ------------------------------------------------------------------------------------------------ bounds
def state_bounds(case, accepted64):
    """B[m, n]: one more accepted step than the restatement took, for the location's sub-step."""
    return pck.state_bound(case["S_max"], np.asarray(accepted64) + 1, case_options(case)["abs_tol"])


def event_time_bound(event_tol, dgdx_abs, B, gdot_abs):
    """dt[...] = EventTol + 2 (EventTol + sum_k |dg/dx_k| B_k) / |gdot|;  dgdx_abs[..., n], B[n] (one problem), gdot_abs[...]"""
    return event_tol + 2.0 * (event_tol + (np.asarray(dgdx_abs) * np.asarray(B)).sum(axis=-1)) / np.asarray(gdot_abs)


def event_state_bound(B, f_abs, dt):
    """[..., n] = B_k + 2 |f_k| dt"""
    return np.asarray(B) + 2.0 * np.asarray(f_abs) * np.asarray(dt)[..., None]


def check_conditions(case, res):
    """The conditions the bounds rest on, for the restatement `res` of `case` (generator, CPU test): |gddot| (bracketing step) <=
    |gdot| / 2 at every fixture event, and no accepted step spans more than half the smallest gap between neighbouring crossings."""
    for i, r in enumerate(res):
        longest = max((abs(b - a) for a, b in r["accepted_steps"]), default=0.0)
        assert longest <= 0.5 * case["min_gap"][i] * (1 + 1e-12), (case["name"], i, longest, case["min_gap"][i])
        for j in range(len(case["events"])):
            for k, loc in enumerate(r["locs"][j]):
                assert abs(case["gddot"][i, j, k]) * abs(loc["h"]) <= 0.5 * abs(case["gdot"][i, j, k]), (case["name"], i, j, k)


def compare_case(case, got, B, factor=1.0, what=""):
    """got: per problem dict(x, t_end, stopped, count[ne], locs[ne] = [dict(x, t)] -- the located (converged) occurrences in order).
    Asserts counts, stopped, event times and states, end states within `factor` times the bounds; returns the worst ratio."""
    worst = 0.0
    ne, n = len(case["events"]), case["rows"].shape[1] - 1 - SYSTEMS[case["system"]]["uv"] - SYSTEMS[case["system"]]["pv"]
    for i, g in enumerate(got):
        tag = f"{what} {case['name']} problem {i}"
        assert list(g["count"]) == list(case["count"][i]), (tag, "counts", list(g["count"]), list(case["count"][i]))
        assert int(g["stopped"]) == int(case["stopped"][i]), (tag, "stopped", g["stopped"], case["stopped"][i])
        for j in range(ne):
            nloc = min(int(case["count"][i, j]), case["max_locs"])
            assert len(g["locs"][j]) == nloc, (tag, "event", j, "located", len(g["locs"][j]), "of", nloc)
            for k, loc in enumerate(g["locs"][j]):
                dt = event_time_bound(case["event_tol"], case["dgdx_abs"][i, j, k], B[i], abs(case["gdot"][i, j, k]))
                rt = abs(float(loc["t"]) - case["t_event"][i, j, k]) / (factor * dt)
                bx = event_state_bound(B[i], case["f_abs"][i, j, k], dt)
                rx = float((np.abs(np.asarray(loc["x"], dtype=float)[:n] - case["x_event"][i, j, k]) / (factor * bx)).max())
                worst = max(worst, rt, rx)
                assert rt <= 1.0 and rx <= 1.0, (tag, "event", j, "occurrence", k, "time ratio", rt, "state ratio", rx)
        if case["stopped"][i] >= 0:
            ts, dts = case["t_stop"][i], case["dt_stop"][i]
            sg = 1.0 if case["tfs"][i] > case["rows"][i, n] else -1.0
            past = sg * (float(g["t_end"]) - ts)
            assert -factor * dts <= past < case["options"]["max_step"], (tag, "t_end", g["t_end"], "stop event", ts)
            ref = exact_flow(case["system"], case["rows"][i], LD(float(g["t_end"]))).astype(float)
        else:
            assert float(g["t_end"]) == float(case["tfs"][i]), (tag, "t_end")
            ref = case["x_end"][i]
        rx = float((np.abs(np.asarray(g["x"], dtype=float) - ref) / (factor * B[i])).max())
        worst = max(worst, rx)
        assert rx <= 1.0, (tag, "end state ratio", rx)
    print(f"{what} {case['name']}: worst |got - exact| / bound = {worst:.3g}")
    return worst


def case_from_restatement(name, system, events, direction, stop, rows, tfs, options, event_tol, max_locs, S_max):
    """Where there is no 50-digit fixture: a case whose reference values are the float64 restatement's own (each side is within its
    bound of the exact values, so the two are compared at TWICE the bounds: compare_case(..., factor=2)).  S_max [m, n, n] is the
    caller's.  Returns (case, B)."""
    sysd = SYSTEMS[system]
    n, ne, K = sysd["n"], len(events), max_locs
    rows, tfs = np.atleast_2d(np.asarray(rows, dtype=float)), np.asarray(tfs, dtype=float).ravel()
    m = rows.shape[0]
    case = dict(name=name, system=system, events=list(events), direction=list(direction), stop=list(stop), options=dict(options),
                event_tol=event_tol, max_locs=max_locs, rows=rows, tfs=tfs, S_max=np.asarray(S_max, dtype=float))
    res = restate_case(case)
    case.update({k: np.full((m, ne, K), np.nan) for k in ("t_event", "gdot")})
    case.update({k: np.full((m, ne, K, n), np.nan) for k in ("x_event", "f_abs", "dgdx_abs")})
    case["count"] = np.array([r["count"] for r in res]).reshape(m, ne)
    case["stopped"] = np.array([r["stopped"] for r in res])
    case["accepted64"] = np.array([r["steps"][0] for r in res])
    case["x_end"], case["t_stop"], case["dt_stop"] = np.full((m, n), np.nan), np.full(m, np.nan), np.full(m, np.nan)
    B = state_bounds(case, case["accepted64"])
    for i, r in enumerate(res):
        assert r["status"] == 0, (name, i, r["status"])
        for j in range(ne):
            for k, loc in enumerate(r["locs"][j]):
                assert loc["conv"]
                y = rows[i].copy()
                y[:n], y[n] = np.asarray(loc["x"], dtype=float), float(loc["t"])
                fv, dg = sysd["f"](y), sysd["events"][events[j]][1](y)
                case["t_event"][i, j, k], case["x_event"][i, j, k] = float(loc["t"]), y[:n]
                case["gdot"][i, j, k], case["f_abs"][i, j, k], case["dgdx_abs"][i, j, k] = float(dg @ fv), np.abs(fv), np.abs(dg)
        if r["stopped"] >= 0:
            j, k = r["stopped"], stop[r["stopped"]] - 1
            case["t_stop"][i] = case["t_event"][i, j, k]
            case["dt_stop"][i] = event_time_bound(event_tol, case["dgdx_abs"][i, j, k], B[i], abs(case["gdot"][i, j, k]))
        else:
            case["x_end"][i] = np.asarray(r["x"], dtype=float)
    return case, B


def restatement_as_got(res):
    return [dict(x=r["x"], t_end=r["t_end"], stopped=r["stopped"], count=r["count"],
                 locs=[[loc for loc in lj if loc["conv"]] for lj in r["locs"]]) for r in res]


# ------------------------------------------------------------------------------------------------ the fixture
_CACHE = None
ARRAYS = ("rows", "tfs", "count", "stopped", "t_event", "x_event", "gdot", "gddot", "f_abs", "dgdx_abs", "S_max", "x_end", "t_stop",
          "dt_stop", "min_gap", "accepted64")


def fixture():
    """(meta, cases): cases[name] = the case's meta data (system, events, direction, stop, event_tol, max_locs, options) with the arrays
    rows [m, N], tfs [m], count [m, ne] (exact), stopped [m], t_event / gdot / gddot [m, ne, K] and x_event / f_abs / dgdx_abs [m, ne, K, n]
    of the first K = max_locs exact occurrences (NaN where there is none), S_max [m, n, n], x_end [m, n] (exact at tf; NaN for a problem
    that stops), t_stop [m] (the stopping event's exact time, NaN) with its time bound dt_stop, min_gap [m] (smallest gap between
    neighbouring crossings of one event, the start excluded), accepted64 [m] (accepted steps of the float64 restatement)."""
    global _CACHE
    if _CACHE is None:
        z = np.load(FIXTURE)
        meta = json.loads(str(z["meta"]))
        cases = {}
        for c in meta["cases"]:
            d = dict(c)
            for a in ARRAYS:
                d[a] = z[f"{c['name']}.{a}"]
            cases[c["name"]] = d
        _CACHE = (meta, cases)
    return _CACHE


def case_names():
    return list(fixture()[1]) if os.path.exists(FIXTURE) else []


def case_options(case):
    return gck.options(**case["options"])
