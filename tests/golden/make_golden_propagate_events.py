"""Generates tests/golden/propagate_events/events.npz: exact (50-digit, mpmath) event times, event states, counts and end states of the
cases below, with the conditions the bounds of tests/event_checker.py rest on recorded beside them and asserted here on the float64
restatement.  Run from the repository root:  python tests/golden/make_golden_propagate_events.py

Exact flows: the oscillator and the free fall in closed form; twobody_lt with zero thrust through Kepler's equation (Lagrange
coefficients in the change of eccentric anomaly); vanderpol by mpmath's Taylor-series integrator at 50 digits.  Crossings of an event
are found by a scan of g along the exact flow (a grid far finer than the gap between crossings) and a bracketed root search to 45
digits; gdot and gddot by numerical differentiation of g along the flow at 50 digits; S_max by differences of the exact flow in the
initial state (relative step 1e-25) at nine equally spaced times and every event time."""
from __future__ import annotations

import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import event_checker as eck  # noqa: E402

mp.mp.dps = 50
OPT = dict(def_step=0.1, min_step=1.0e-5, max_step=1.0, max_step_change=3.0, adaptive=True, max_steps=100000, abs_tol=1.0e-12, rel_tol=0.0)


def osc_row(A, t0):
    return [float(A * mp.cos(t0)), float(-A * mp.sin(t0)), float(t0)]


def kepler_row(e, nu, inc, t0):
    """a = 1, mu = 1; true anomaly nu, the orbit plane tilted by inc about the x axis; zero thrust"""
    e, nu, inc = mp.mpf(e), mp.mpf(nu), mp.mpf(inc)
    p = 1 - e * e
    r = p / (1 + e * mp.cos(nu))
    xp, yp = r * mp.cos(nu), r * mp.sin(nu)
    vx, vy = -mp.sin(nu) / mp.sqrt(p), (e + mp.cos(nu)) / mp.sqrt(p)
    c, s = mp.cos(inc), mp.sin(inc)
    return [float(v) for v in (xp, yp * c, yp * s, vx, vy * c, vy * s)] + [float(t0), 0.0, 0.0, 0.0]


TWO_PI = float(2 * mp.pi)
CASES = [
    dict(name="osc_any_stop0", system="oscillator", events=["x0"], direction=[0], stop=[0], event_tol=1.0e-6, max_locs=8, options=OPT,
         rows=[osc_row(1.0, 0.0), osc_row(2.0, 0.3), osc_row(0.5, -0.4), osc_row(1.5, 1.0)], length=11.0),
    dict(name="osc_up_stop1", system="oscillator", events=["x0"], direction=[1], stop=[1], event_tol=1.0e-6, max_locs=8, options=OPT,
         rows=[osc_row(1.0, 0.0), osc_row(2.0, 0.3), osc_row(0.5, -0.4), osc_row(1.5, 1.0)], length=11.0),
    dict(name="osc_down_stop3", system="oscillator", events=["x0"], direction=[-1], stop=[3], event_tol=1.0e-6, max_locs=8, options=OPT,
         rows=[osc_row(1.0, 0.0), osc_row(2.0, 0.3), osc_row(0.5, -0.4)], length=17.0),
    dict(name="osc_backward_stop2", system="oscillator", events=["x0"], direction=[-1], stop=[2], event_tol=1.0e-6, max_locs=8, options=OPT,
         rows=[osc_row(1.0, 0.0), osc_row(2.0, 0.3), osc_row(0.5, -0.4)], length=-14.0),
    dict(name="osc_tight_tol", system="oscillator", events=["x0"], direction=[0], stop=[0], event_tol=1.0e-10, max_locs=8, options=OPT,
         rows=[osc_row(1.0, 0.0), osc_row(1.5, 1.0)], length=7.0),
    dict(name="fall_impact", system="freefall", events=["height"], direction=[-1], stop=[1], event_tol=1.0e-6, max_locs=8,
         options=dict(OPT, max_step=0.5),
         rows=[[10.0, 0.0, 0.0, 9.81], [25.0, 0.0, 0.5, 3.71], [40.0, 0.0, -1.0, 1.62], [15.0, 0.0, 0.0, 24.79], [50.0, 0.0, 2.0, 8.87]],
         tfs="impact"),
    dict(name="kepler_apsides", system="twobody_lt", events=["rv"], direction=[0], stop=[0], event_tol=1.0e-6, max_locs=8,
         options=dict(OPT, max_step=0.75),
         rows=[kepler_row(0.3, 0.7, 0.2, 0.0), kepler_row(0.5, 2.0, 0.9, 0.5), kepler_row(0.1, 4.0, 0.0, -1.0)], length=1.6 * TWO_PI),
    dict(name="kepler_next_periapsis_tight", system="twobody_lt", events=["rv"], direction=[1], stop=[1], event_tol=1.0e-10, max_locs=8,
         options=dict(OPT, max_step=0.75),
         rows=[kepler_row(0.3, 0.7, 0.2, 0.0), kepler_row(0.5, 2.0, 0.9, 0.5), kepler_row(0.6, 3.5, 0.4, 0.0)], length=1.6 * TWO_PI),
    dict(name="kepler_backward", system="twobody_lt", events=["rv"], direction=[0], stop=[2], event_tol=1.0e-6, max_locs=8,
         options=dict(OPT, max_step=0.75),
         rows=[kepler_row(0.3, 0.7, 0.2, 0.0), kepler_row(0.5, 2.0, 0.9, 0.5)], length=-1.6 * TWO_PI),
    dict(name="vdp_x1", system="vanderpol", events=["x1"], direction=[0], stop=[0], event_tol=1.0e-6, max_locs=8,
         options=dict(OPT, max_step=0.5),
         rows=[[1.0, 0.5, 0.0, 0.3, 1.0], [-0.5, 1.5, 0.2, -0.2, 0.7]], length=6.0),
]


# ------------------------------------------------------------------------------------------------ exact flows
_VDP = {}


def flow(system, row, t):
    """x(t) as a list of mpf; row: exact rationals of the float64 row"""
    t = mp.mpf(t)
    if system == "oscillator":
        d = t - row[2]
        c, s = mp.cos(d), mp.sin(d)
        return [row[0] * c + row[1] * s, -row[0] * s + row[1] * c]
    if system == "freefall":
        d = t - row[2]
        return [row[0] + row[1] * d - row[3] * d * d / 2, row[1] - row[3] * d]
    if system == "twobody_lt":
        r0v, v0v = row[0:3], row[3:6]
        dot = lambda a, b: sum(x * y for x, y in zip(a, b))
        r0, v2, rv = mp.sqrt(dot(r0v, r0v)), dot(v0v, v0v), dot(r0v, v0v)
        a = 1 / (2 / r0 - v2)
        sa = mp.sqrt(a)
        nm, sig, dt = 1 / (a * sa), rv / sa, t - row[6]
        M = nm * dt
        dE = mp.findroot(lambda E: E - (1 - r0 / a) * mp.sin(E) + sig * (1 - mp.cos(E)) - M, M, tol=mp.mpf(10) ** -47, maxsteps=200)
        cE, sE = mp.cos(dE), mp.sin(dE)
        r = a + (r0 - a) * cE + sig * sa * sE
        fl, gl = 1 - a * (1 - cE) / r0, dt - (dE - sE) / nm
        fd, gd = -sa * sE / (r * r0), 1 - a * (1 - cE) / r
        return [fl * p + gl * q for p, q in zip(r0v, v0v)] + [fd * p + gd * q for p, q in zip(r0v, v0v)]
    if system == "vanderpol":
        key = tuple(str(v) for v in row)
        if key not in _VDP:
            u, mu, t0 = row[3], row[4], row[2]
            rhs = lambda tt, y: [y[1], mu * (1 - y[0] * y[0]) * y[1] - y[0] + u * mp.exp(-tt / 10)]
            _VDP[key] = (mp.odefun(rhs, t0, [row[0], row[1]], tol=mp.mpf(10) ** -45), t0)
        sol, t0 = _VDP[key]
        assert t >= t0
        return list(sol(t))
    raise KeyError(system)


def g_mp(system, event, row, x, t):
    if (system, event) == ("twobody_lt", "rv"):
        return x[0] * x[3] + x[1] * x[4] + x[2] * x[5]
    if event == "x0" or event == "height":
        return x[0]
    if event == "x1":
        return x[1]
    raise KeyError((system, event))


def f_mp(system, row, x, t):
    if system == "oscillator":
        return [x[1], -x[0]]
    if system == "freefall":
        return [x[1], -row[3]]
    if system == "twobody_lt":
        r3 = (x[0] ** 2 + x[1] ** 2 + x[2] ** 2) ** mp.mpf(1.5)
        return [x[3], x[4], x[5], -x[0] / r3, -x[1] / r3, -x[2] / r3]
    if system == "vanderpol":
        return [x[1], row[4] * (1 - x[0] * x[0]) * x[1] - x[0] + row[3] * mp.exp(-t / 10)]
    raise KeyError(system)


def crossings(G, t0, tf, grid=4000):
    """roots of G between t0 and tf (exclusive), in the order the propagation meets them"""
    t0, tf = mp.mpf(t0), mp.mpf(tf)
    ts = [t0 + (tf - t0) * k / grid for k in range(grid + 1)]
    vals = [G(t) for t in ts]
    assert vals[0] != 0
    out = []
    for k in range(grid):
        assert vals[k + 1] != 0
        if vals[k] * vals[k + 1] < 0:
            lo, hi = (ts[k], ts[k + 1]) if ts[k] < ts[k + 1] else (ts[k + 1], ts[k])
            out.append(mp.findroot(G, (lo, hi), solver="anderson", tol=mp.mpf(10) ** -45, maxsteps=200))
    return out


def build_case(c):
    system, n = c["system"], eck.SYSTEMS[c["system"]]["n"]
    rows = np.array(c["rows"], dtype=float)
    m, ne, K = rows.shape[0], len(c["events"]), c["max_locs"]
    if c.get("tfs") == "impact":                     # the free fall: half as long again as the fall takes
        tfs = np.array([r[2] + 1.5 * float(mp.sqrt(2 * mp.mpf(r[0]) / mp.mpf(r[3]))) for r in rows])
    else:
        tfs = rows[:, n] + c["length"]
    opt = eck.gck.options(**c["options"])
    A = {k: np.full((m, ne, K), np.nan) for k in ("t_event", "gdot", "gddot")}
    A.update({k: np.full((m, ne, K, n), np.nan) for k in ("x_event", "f_abs", "dgdx_abs")})
    count, stopped = np.zeros((m, ne), dtype=int), np.full(m, -1)
    t_stop, x_end, min_gap, S_max = np.full(m, np.nan), np.full((m, n), np.nan), np.full(m, 1.0e300), np.zeros((m, n, n))
    for i in range(m):
        row = [mp.mpf(float(v)) for v in rows[i]]
        t0, tf = row[n], mp.mpf(float(tfs[i]))
        sg = 1 if tf > t0 else -1
        occ = []                                     # (time, event, matches its direction)
        for j, e in enumerate(c["events"]):
            G = (lambda ev: lambda t: g_mp(system, ev, row, flow(system, row, t), t))(e)
            tc = crossings(G, t0, tf + sg * mp.mpf(c["options"]["max_step"]))      # (and what lies right behind tf)
            gaps = [abs(b - a) for a, b in zip(tc, tc[1:])]
            if gaps:
                min_gap[i] = min(min_gap[i], float(min(gaps)))
            for ts in tc:
                after = G(ts + sg * mp.mpf(10) ** -8)
                d = c["direction"][j]
                occ.append((ts, j, d == 0 or (after > 0) == (d > 0), G))
        occ.sort(key=lambda o: sg * o[0])
        sample_t = [t0 + (tf - t0) * k / 8 for k in range(9)]
        for ts, j, match, G in occ:
            if sg * (ts - tf) >= 0 or not match:
                continue
            if stopped[i] >= 0:                      # nothing else may occur in the step that stops the propagation
                assert sg * (ts - t_stop[i]) > c["options"]["max_step"], (c["name"], i, "a crossing right behind the stop")
                continue
            k = count[i, j]
            count[i, j] += 1
            if k < K:
                x = flow(system, row, ts)
                A["t_event"][i, j, k] = float(ts)
                A["x_event"][i, j, k] = [float(v) for v in x]
                A["gdot"][i, j, k] = float(mp.diff(G, ts, 1, h=mp.mpf(10) ** -12))
                A["gddot"][i, j, k] = float(mp.diff(G, ts, 2, h=mp.mpf(10) ** -10))
                A["f_abs"][i, j, k] = [abs(float(v)) for v in f_mp(system, row, x, ts)]
                y = np.array([float(v) for v in x] + [float(ts)] + list(rows[i, n + 1:]))
                A["dgdx_abs"][i, j, k] = np.abs(eck.SYSTEMS[system]["events"][c["events"][j]][1](y))
                sample_t.append(ts)
            if c["stop"][j] > 0 and count[i, j] == c["stop"][j]:
                stopped[i], t_stop[i] = j, float(ts)
        if stopped[i] < 0:
            x_end[i] = [float(v) for v in flow(system, row, tf)]
        # S_max: differences of the exact flow in the initial state
        for q in range(n):
            d = mp.mpf(10) ** -25 * max(1, abs(row[q]))
            rp = list(row)
            rp[q] = row[q] + d
            for ts in sample_t:
                col = [(a - b) / d for a, b in zip(flow(system, rp, ts), flow(system, row, ts))]
                S_max[i, :, q] = np.maximum(S_max[i, :, q], [abs(float(v)) for v in col])
        print(f"  {c['name']} problem {i}: counts {count[i].tolist()} stopped {stopped[i]} min gap {min_gap[i]:.3g}", flush=True)
    case = dict({k: c[k] for k in ("name", "system", "events", "direction", "stop", "event_tol", "max_locs", "options")},
                rows=rows, tfs=tfs, count=count, stopped=stopped, t_stop=t_stop, x_end=x_end, min_gap=min_gap, S_max=S_max, **A)
    # the float64 restatement: the conditions, and a quarter of every bound
    res = eck.restate_case(case)
    assert all(r["status"] == 0 for r in res)
    case["accepted64"] = np.array([r["steps"][0] for r in res])
    B = eck.state_bounds(case, case["accepted64"])
    case["dt_stop"] = np.full(m, np.nan)
    for i in range(m):
        if stopped[i] >= 0:
            j, k = stopped[i], c["stop"][stopped[i]] - 1
            case["dt_stop"][i] = eck.event_time_bound(c["event_tol"], A["dgdx_abs"][i, j, k], B[i], abs(A["gdot"][i, j, k]))
    eck.check_conditions(case, res)
    eck.compare_case(case, eck.restatement_as_got(res), B, what="float64 restatement:")
    eck.compare_case(case, eck.restatement_as_got(eck.restate_case(case, tol_factor=0.25)), B, factor=0.25,
                     what="float64 restatement at EventTol / 4, a quarter of the bounds:")
    return case


def main():
    out, meta = {}, dict(digits=mp.mp.dps, cases=[])
    for c in CASES:
        print(c["name"], flush=True)
        case = build_case(c)
        meta["cases"].append({k: case[k] for k in ("name", "system", "events", "direction", "stop", "event_tol", "max_locs", "options")})
        for a in eck.ARRAYS:
            out[f"{case['name']}.{a}"] = np.asarray(case[a])
    os.makedirs(os.path.join(HERE, "propagate_events"), exist_ok=True)
    path = os.path.join(HERE, "propagate_events", "events.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
