"""Generate tests/golden/mesh_error.npz (run once, here; commit the file): the de Boor mesh-error estimate in 50-digit arithmetic.

What is computed, from the formulas (ODEPhase<DODE>::get_meshinfo_deboor of the reference, OptimalControl/ODEPhase.h:442-585):
    y_i = sum_j [ x_j XW_j + f_j DXW_j h_i ] / h_i^Order        over the cs nodes of block i, h_i = t_last - t_first,
          XW_j = Cardinal_XPower_Weights[j][0] Order!,  DXW_j = Cardinal_DXPower_Weights[j][0] Order!   (the leading power weights of the
          scheme's Hermite interpolant: y_i is its Order-th derivative); Trapezoidal: XW = {0, 0}, DXW = {-1, 1}, Order 2, no factorial;
          BlockConstant control: f of the block's last node is evaluated under the first node's controls;
    e_i = |y_i - y_(i-1)| / |h_i + h_(i-1)| + |y_(i+1) - y_i| / |h_i + h_(i+1)|,   at the ends 2 |y_0 - y_1| / |h_0 + h_1| and its mirror;
    mesh_dist_i = e_i^(1/(Order+1)),   mesh_errors_i = e_i |h_i|^(Order+1) ErrorWeight  (Trapezoidal: 1/12);   the last column repeats the
    one before;   tsnd_i = (t_first,i - T0) / (TF - T0), tsnd_nb = 1.
Scheme constants come from tests/golden/lgl_tables.json only (the reference's coefficient header parsed as data).  The right-hand sides
are the generic-scalar ODEs of make_golden.py evaluated in mpf; `vanderpol`, tests/helpers.py: make_shape, the integrator x' = u and the
cart-pole are restated here.  Nothing of asset_asrl_amd/csrc, asset_asrl_amd/mesh.py or oracle/mesh.cpp is used.  Every result is
rounded to float64 once.

With each case go the two arrays of tests/mesh_checker.py's bound (tau = 16 u tau_s + eps_f tau_phi), and the meta data hold eps_f: per ODE
the worst |f_oracle - f_mp| / |f_mp|_inf over the fixture's own rows, f_oracle the oracle's float64 ``OdeStruct.f`` through ctypes
(tests/interp_checker.py: oracle_rhs), and the factor 8 the tests multiply it by.  (`cartpole` has no case: its eps_f, for the adaptive-mesh
test, is measured on 400 random rows.)

The generator asserts what keeps a case from hiding a failure: random-state cases have tau / e <= 1e-9 wherever the 50-digit e is not
zero, smooth coarse cases tau / e <= 1e-3; entries with e = 0 (a state without curvature) are counted per case in the meta data; at most a
quarter of the cases are smooth fine ones, where rounding dominates (tau >= e may happen).

Usage:  python tests/golden/make_golden_mesh.py            (writes tests/golden/mesh_error.npz)
"""
from __future__ import annotations

import json
import math
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import interp_checker as ick  # noqa: E402      (ragged_traj; oracle_rhs)
import mesh_checker as mck  # noqa: E402        (the numpy bound: tolerance_data)
from make_golden import ODES as GOLDEN_ODES  # noqa: E402

mp.mp.dps = 50
MODE_CS = {"Trapezoidal": 2, "LGL3": 2, "LGL5": 3, "LGL7": 4}
EPS_F_FACTOR = 8.0
_TABLES = json.load(open(os.path.join(HERE, "lgl_tables.json")))["tables"]


class M:
    """math namespace for plain mpf (make_golden's MP is for its AD scalar)"""
    sin, cos, tan, exp, sqrt = (staticmethod(f) for f in (mp.sin, mp.cos, mp.tan, mp.exp, mp.sqrt))


# --------------------------------------------------------------------------- right-hand sides restated here
def ode_vanderpol(y, M):
    x0, x1, t, u, mu = y
    return [x1, mu * (1.0 - x0 * x0) * x1 - x0 + u * M.exp(-0.1 * t)]


def ode_shape(n, m, p):
    def f(y, M):
        t, u, par = y[n], y[n + 1:n + 1 + m], y[n + 1 + m:]
        out = []
        for k in range(n):
            v = M.sin(y[(k + 1) % n]) * y[(k + 2) % n]
            if m > 0:
                v = v * u[k % m]
            v = v - 0.5 * y[k] + 0.3 * M.cos(t) * y[(k + 3) % n]
            if m > 0:
                v = v + 0.1 * u[(k + 1) % m] * u[(k + 1) % m]
            if p > 0:
                v = v + par[0] * y[k] * y[(k + 1) % n] + par[p - 1] * M.cos(t)
            out.append(v)
        return out
    return f


def ode_integrator(y, M):
    return [y[2]]


def ode_cartpole(y, M):
    l, m1, m2, g = 0.5, 1.0, 0.3, 9.81
    q2, q1d, q2d, u = y[1], y[2], y[3], y[5]
    s2, c2 = M.sin(q2), M.cos(q2)
    den = m1 + m2 * (1.0 - c2 * c2)
    return [q1d, q2d, (l * m2 * s2 * (q2d * q2d) + u + (m2 * g) * c2 * s2) / den,
            -1.0 * (l * m2 * c2 * s2 * (q2d * q2d) + u * c2 + (m1 * g + m2 * g) * s2) / (l * den)]


# name -> (generic-scalar right-hand side, (xv, uv, pv))
ODES = {"reentry": (GOLDEN_ODES["reentry"], (5, 2, 0)), "twobody_lt": (GOLDEN_ODES["twobody_lt"], (6, 3, 0)),
        "betts_lowthrust": (GOLDEN_ODES["betts_lowthrust"], (7, 3, 1)), "brachistochrone": (GOLDEN_ODES["brachistochrone"], (3, 1, 0)),
        "vanderpol": (ode_vanderpol, (2, 1, 1)), "shape_1_0_0": (ode_shape(1, 0, 0), (1, 0, 0)),
        "shape_5_3_2": (ode_shape(5, 3, 2), (5, 3, 2)), "integrator": (ode_integrator, (1, 1, 0)), "cartpole": (ode_cartpole, (4, 1, 0))}


def rhs_mp(ode, row):
    """f(row) in mpf; row: float64 values, promoted exactly."""
    return [mp.mpf(v) for v in ODES[ode][0]([mp.mpf(float(v)) for v in row], M)]


# --------------------------------------------------------------------------- the estimate
def scheme_mp(mode):
    """(cs, Order, ErrorWeight, XW[cs], DXW[cs]) in mpf."""
    if mode == "Trapezoidal":
        return 2, 2, mp.mpf(1) / 12, [mp.mpf(0), mp.mpf(0)], [mp.mpf(-1), mp.mpf(1)]
    cs = MODE_CS[mode]
    t = _TABLES[str(cs)]
    order = int(t["Order"])
    fact = mp.mpf(math.factorial(order))
    return (cs, order, mp.mpf(t["ErrorWeight"]), [mp.mpf(r[0]) * fact for r in t["Cardinal_XPower_Weights"]],
            [mp.mpf(r[0]) * fact for r in t["Cardinal_DXPower_Weights"]])


def estimate_mp(ode, mode, blocked, traj):
    """-> (tsnd[nb+1], e[xv, nb+1], mesh_errors[xv, nb+1], mesh_dist[xv, nb+1]) float64, and the mpf right-hand sides by block
    f[nb][cs][xv] (BlockConstant: the last node's under the first node's controls)."""
    xv, uv, pv = ODES[ode][1]
    cs, order, ew, XW, DXW = scheme_mp(mode)
    K = cs - 1
    nb = (traj.shape[0] - 1) // K
    assert nb >= 2 and nb * K + 1 == traj.shape[0]
    fnode = [rhs_mp(ode, r) for r in traj]
    t = [mp.mpf(float(v)) for v in traj[:, xv]]
    hs, ys, fs = [], [], []
    for i in range(nb):
        s = K * i
        h = t[s + K] - t[s]
        fb = [fnode[s + j] for j in range(cs)]
        if blocked and uv > 0:
            row = traj[s + K].copy()
            row[xv + 1:xv + 1 + uv] = traj[s, xv + 1:xv + 1 + uv]
            fb[-1] = rhs_mp(ode, row)
        hp = h ** order
        ys.append([sum((mp.mpf(float(traj[s + j, k])) * XW[j] + fb[j][k] * DXW[j] * h for j in range(cs)), mp.mpf(0)) / hp
                   for k in range(xv)])
        hs.append(h), fs.append(fb)
    e = []
    for i in range(nb):
        if 0 < i < nb - 1:
            e.append([abs((ys[i][k] - ys[i - 1][k]) / (hs[i] + hs[i - 1])) + abs((ys[i + 1][k] - ys[i][k]) / (hs[i] + hs[i + 1]))
                      for k in range(xv)])
        else:
            o = 1 if i == 0 else i - 1
            e.append([abs(2 * (ys[i][k] - ys[o][k]) / (hs[i] + hs[o])) for k in range(xv)])
    p = mp.mpf(1) / (order + 1)
    dist = [[v ** p if v != 0 else mp.mpf(0) for v in row] for row in e]
    err = [[v * abs(hs[i]) ** (order + 1) * ew for v in row] for i, row in enumerate(e)]
    tsnd = [(t[K * i] - t[0]) / (t[-1] - t[0]) for i in range(nb)] + [mp.mpf(1)]
    col = lambda a: np.array([[float(v) for v in row] for row in a + a[-1:]]).T.reshape(xv, nb + 1)
    return (np.array([float(v) for v in tsnd]), col(e), col(err), col(dist)), fs, e


# --------------------------------------------------------------------------- trajectories
def kepler_mp(t, ecc=0.4):
    """State of the Kepler orbit a = 1, mu = 1, eccentricity `ecc`, at time t from periapsis: (r[3], v[3]) in mpf."""
    t, ecc = mp.mpf(float(t)), mp.mpf(ecc)
    E = t
    for _ in range(200):
        dE = (E - ecc * mp.sin(E) - t) / (1 - ecc * mp.cos(E))
        E = E - dE
        if abs(dE) < mp.mpf(10) ** -48:
            break
    b = mp.sqrt(1 - ecc * ecc)
    d = 1 - ecc * mp.cos(E)
    return [mp.cos(E) - ecc, b * mp.sin(E), mp.mpf(0), -mp.sin(E) / d, b * mp.cos(E) / d, mp.mpf(0)]


def poly_coeffs(degree, seed):
    """c_0 .. c_degree ~ U(-1, 1), the leading one kept away from zero."""
    c = np.random.default_rng(seed).uniform(-1.0, 1.0, degree + 1)
    c[-1] = math.copysign(0.5 + 0.5 * abs(c[-1]), c[-1])
    return c


def poly_mp(c, t, deriv=0):
    t = mp.mpf(float(t))
    return sum((mp.mpf(float(c[k])) * mp.mpf(math.factorial(k) // math.factorial(k - deriv)) * t ** (k - deriv)
                for k in range(deriv, len(c))), mp.mpf(0))


def make_traj(spec):
    ode, mode, nb, seed = spec["ode"], spec["mode"], spec["nb"], spec["seed"]
    sizes = ODES[ode][1]
    kind = spec["family"]
    if kind == "random":
        named = ode in ("reentry", "twobody_lt", "betts_lowthrust", "brachistochrone")
        return ick.ragged_traj(ode, mode, nb, seed=seed, sizes=None if named else sizes)
    xv = sizes[0]
    traj = ick.ragged_traj(ode, mode, nb, seed=seed, T=2.0, sizes=None if ode == "twobody_lt" else sizes)
    t = traj[:, xv]
    if ode == "twobody_lt":                                   # exact Kepler samples, no thrust
        traj[:, xv + 1:] = 0.0
        for i, ti in enumerate(t):
            traj[i, :6] = [float(v) for v in kepler_mp(ti)]
    else:                                                     # the integrator on x = P(t), u = P'(t)
        c = np.asarray(spec["poly"])
        for i, ti in enumerate(t):
            traj[i, 0], traj[i, 2] = float(poly_mp(c, ti)), float(poly_mp(c, ti, 1))
    return traj


def _specs():
    out = []

    def add(family, ode, mode, blocked, nb, **kw):
        name = f"{ode}_{mode}{'_blocked' if blocked else ''}_{nb}" + kw.pop("tag", "")
        out.append(dict(name=name, family=family, ode=ode, mode=mode, blocked=bool(blocked), nb=nb, seed=kw.pop("seed", 500 + len(out)),
                        sizes=list(ODES[ode][1]), **kw))
    add("random", "reentry", "LGL7", False, 257)
    add("random", "reentry", "LGL7", False, 65)
    add("random", "reentry", "LGL3", False, 64)
    add("random", "twobody_lt", "LGL5", True, 75)
    add("random", "twobody_lt", "Trapezoidal", True, 21)
    add("random", "betts_lowthrust", "LGL5", False, 33)
    add("random", "brachistochrone", "Trapezoidal", False, 40)
    for mode in ("Trapezoidal", "LGL3", "LGL5", "LGL7"):
        for nb in (2, 3, 4):
            add("random", "reentry", mode, False, nb)
    add("random", "shape_1_0_0", "LGL7", True, 19)          # the BlockConstant flag without controls to relabel
    add("random", "shape_5_3_2", "LGL5", True, 23)          # controls and parameters
    add("random", "vanderpol", "LGL3", False, 30)
    # Exact Kepler samples on 16 ragged segments over [0, 2].  Measured here: tau / e <= 1.1e-9 (Trapezoidal), 1.3e-6 (LGL3), but 2.3e-3 ..
    # 2.6e-2 (LGL5) and 1 .. 3.4 (LGL7) over six mesh seeds -- and 7e-2 for LGL7 even on 16 EQUAL segments: dividing by h^5 and h^7 at
    # h = 0.02 .. 0.3 already costs what the coarse family may not lose, so these two are counted with the rounding-limited family.
    for mode, family in (("Trapezoidal", "smooth-coarse"), ("LGL3", "smooth-coarse"), ("LGL5", "smooth-fine"), ("LGL7", "smooth-fine")):
        add(family, "twobody_lt", mode, False, 16, tag="_kepler")
    for mode, order in (("Trapezoidal", 2), ("LGL3", 3), ("LGL5", 5), ("LGL7", 7)):
        # (mesh seed 541: widths spread 14 x, smallest 0.07; of 25 seeds tried for LGL7, 10 kept tau / e below the family's 1e-3 --
        #  a 7-segment mesh whose smallest block is below 0.06 already loses more than that to the division by h^7)
        add("smooth-coarse", "integrator", mode, False, 7, tag="_poly", seed=541,
            poly=[float(v) for v in poly_coeffs(order + 1, 77 + order)])
    for mode in ("LGL5", "LGL7"):
        add("smooth-fine", "twobody_lt", mode, False, 400, tag="_kepler")
    return out


SPECS = _specs()


def up32(a):
    """A bound needs three digits, not sixteen: float32, rounded up (the file stays small)."""
    a32 = np.asarray(a).astype(np.float32)
    return np.where(a32.astype(np.float64) < a, np.nextafter(a32, np.float32(np.inf)), a32).astype(np.float32)


def make_case(spec, traj=None):
    """The forward and the time-reversed case of one spec: (traj, {"fwd"/"rev": arrays}, zero_e counts, [(rows, f_mp)] for eps_f)."""
    ode, mode, blocked = spec["ode"], spec["mode"], spec["blocked"]
    xv, uv, pv = ODES[ode][1]
    traj = make_traj(spec) if traj is None else traj
    arrays, zero, rows_f = {}, [], []
    for tag, tr in (("fwd", traj), ("rev", traj[::-1].copy())):
        (tsnd, e, err, dist), fs, e_mp = estimate_mp(ode, mode, blocked, tr)
        rows = mck.block_rows(tr, mode, blocked, xv, uv)
        f64 = np.array([[[float(v) for v in fj] for fj in fb] for fb in fs]).reshape(rows.shape[0], rows.shape[1], xv)
        tau_s, tau_phi = mck.tolerance_data(tr, mode, blocked, xv, uv, lambda r, f64=f64: f64.reshape(-1, xv))
        arrays[tag] = dict(tsnd=tsnd, e=e, mesh_errors=err, mesh_dist=dist, tau_s=up32(tau_s), tau_phi=up32(tau_phi))
        zero.append(int(sum(1 for row in e_mp for v in row if v == 0)))
        rows_f.append((rows.reshape(-1, rows.shape[2]), [fj for fb in fs for fj in fb]))
    return traj, arrays, zero, rows_f


def measure_eps_f(oracle, ode, rows, f_mp):
    """worst |f_oracle - f_mp| / |f_mp|_inf over the rows."""
    f64 = ick.oracle_rhs(oracle, ode)(rows)
    worst = mp.mpf(0)
    for a, b in zip(f64, f_mp):
        nrm = max(abs(v) for v in b)
        if nrm == 0:
            assert all(float(v) == 0.0 for v in a)
            continue
        worst = max(worst, max(abs(mp.mpf(float(x)) - y) for x, y in zip(a, b)) / nrm)
    return float(worst)


def check_conditions(spec, arrays, eps):
    """The ratios the module docstring promises; returns the worst tau / e of the case."""
    worst = 0.0
    for tag in ("fwd", "rev"):
        a = arrays[tag]
        tau = mck.tau_of(a["tau_s"], a["tau_phi"], EPS_F_FACTOR * eps)
        e = a["e"][:, :-1]
        nz = e != 0.0
        if nz.any():
            worst = max(worst, float((tau[nz] / e[nz]).max()))
    limit = {"random": 1e-9, "smooth-coarse": 1e-3, "smooth-fine": np.inf}[spec["family"]]
    assert worst <= limit, (spec["name"], worst, limit)
    return worst


def main():
    from oracle import bindings as oracle
    oracle.build()
    out, cases, per_ode, kept = {}, [], {}, []
    for spec in SPECS:
        traj, arrays, zero, rows_f = make_case(spec)
        out[spec["name"] + ".traj"] = traj
        for tag in ("fwd", "rev"):
            for k, v in arrays[tag].items():
                out[f"{spec['name']}.{tag}.{k}"] = v
        for rows, f_mp in rows_f:
            per_ode[spec["ode"]] = max(per_ode.get(spec["ode"], 0.0), measure_eps_f(oracle, spec["ode"], rows, f_mp))
        cases.append(dict(spec, zero_e=zero))
        kept.append((spec, arrays))
        print(f"{spec['name']}: zero-e entries {zero}", flush=True)
    # an ODE without a case: the cart-pole of the adaptive-mesh test, on random rows in the range of its swing-up
    rng = np.random.default_rng(4)
    rows = np.column_stack([rng.uniform(-2, 2, 400), rng.uniform(-4, 4, 400), rng.uniform(-5, 5, 400), rng.uniform(-10, 10, 400),
                            rng.uniform(0, 2, 400), rng.uniform(-20, 20, 400)])
    per_ode["cartpole"] = measure_eps_f(oracle, "cartpole", rows, [rhs_mp("cartpole", r) for r in rows])
    for spec, arrays in kept:
        worst = check_conditions(spec, arrays, per_ode[spec["ode"]])
        print(f"{spec['name']}: worst tau / e {worst:.3e}", flush=True)
    fine = sum(1 for c in cases if c["family"] == "smooth-fine")
    assert 4 * fine <= len(cases), (fine, len(cases))
    meta = dict(dps=mp.mp.dps, mpmath=mp.__version__, eps_f_measured=per_ode, eps_f_factor=EPS_F_FACTOR, cases=cases)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "mesh_error.npz")
    np.savez_compressed(path, **out)
    print("eps_f measured:", {k: f"{v:.3e}" for k, v in per_ode.items()})
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes;", len(cases), "specs, forward and time-reversed")


if __name__ == "__main__":
    main()
