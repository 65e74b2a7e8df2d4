"""Independent reference of the propagation with a controller (csrc/propagate_ctrl_kernels.h behind asset_hip_propagate_ctrl /
asset_hip_propagate_ctrl_stm and ``ode.integrator(def_step, ucon, varlocs)``), and the loader of the 50-digit fixture
tests/golden/propagate_controller/controller.npz (tests/golden/make_golden_propagate_controller.py).  Pure numpy; nothing here touches the
code under test, and no control law goes through ``vf``: LAWS holds every law of tests/controller_cases.py and its Jacobian as numpy
callbacks written by hand.

The closed loop of an ODE f with the law u = K(y[varlocs]) is itself a right-hand side of the row [x, t, u, p],
    f_c(y) = f(y with u := K(y[varlocs])),      fj_c(y): J_c = J with J[:, u] J_K added into the varlocs columns and the u columns zeroed,
and these two callbacks are handed to propagate_checker.propagate as it is -- the restatement of the step rule stays the one already
trusted.  Its S = d x(tf) / d [x0, u, p] then has u columns that are exactly zero, the layout the device returns.

Bounds: those of propagate_checker (state_bound, stm_bound, time_column_bounds), none measured against the code under test; the one
condition is that the float64 restatement uses at most a quarter of each (check_restatement, asserted by the generator and by the CPU
test).  The controls of a returned row: |u - K(row)| <= 16 u |K| + sum_j |dK/dz_j| B_j, the law's Lipschitz bound at the row times the
bound of the state entries it reads (the time and the parameters are exact)."""
from __future__ import annotations

import json
import os

import numpy as np

import propagate_checker as pck

_HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(_HERE, "golden", "propagate_controller", "controller.npz")   # (a directory of its own, as propagate/)
U, LD = pck.U, pck.LD

# ------------------------------------------------------------------------------------------------ right-hand sides not in the oracle
SIZES = {"pd": (2, 1, 1), "vanderpol": (2, 1, 1), "twobody_lt": (6, 3, 0), "shape_5_3_2": (5, 3, 2), "shape_8_3_1": (8, 3, 1),
         "shape_11_4_0": (11, 4, 0), "coupled16": (16, 3, 2)}


def pd_f(y):
    """x0' = x1, x1' = u on the row [x0, x1, t, u, p0]"""
    return np.array([y[1], y[3]], dtype=float)


def pd_fj(y):
    J = np.zeros((2, 5))
    J[0, 1], J[1, 3] = 1.0, 1.0
    return pd_f(y), J


def rhs(oracle, system):
    """(f, fj) of a system: numpy for ``pd``, the oracle's otherwise."""
    if system == "pd":
        return pd_f, pd_fj
    return pck.oracle_f(oracle, system), pck.oracle_fj(oracle, system)


# ------------------------------------------------------------------------------------------------ the laws, by hand
def _shape_law(uv, with_p):
    def K(z):
        k = np.arange(uv, dtype=float)
        v = 0.3 * np.sin(z[0] + 0.5 * k) + 0.2 * np.cos((k + 1.0) * z[1])
        return v + 0.1 * (k + 1.0) * z[2] * z[0] if with_p else v

    def JK(z):
        k = np.arange(uv, dtype=float)
        J = np.zeros((uv, 3 if with_p else 2))
        J[:, 0] = 0.3 * np.cos(z[0] + 0.5 * k)
        J[:, 1] = -0.2 * (k + 1.0) * np.sin((k + 1.0) * z[1])
        if with_p:
            J[:, 0] += 0.1 * (k + 1.0) * z[2]
            J[:, 2] = 0.1 * (k + 1.0) * z[0]
        return J
    return K, JK


def _tangential():
    def K(v):
        return 0.01 * v / np.sqrt(v @ v)

    def JK(v):
        r = np.sqrt(v @ v)
        return 0.01 * (np.eye(3) / r - np.outer(v, v) / r ** 3)
    return K, JK


# name -> (system, varlocs, K(z), J_K(z)); z = row[varlocs]
LAWS = {
    "pd": ("pd", [0, 1, 4], lambda z: np.array([-z[2] * z[0] - 0.4 * z[1]]), lambda z: np.array([[-z[2], -0.4, -z[0]]])),
    "pd_nan": ("pd", [0, 1, 4], lambda z: np.array([-np.sqrt(z[2]) * z[0] - 0.4 * z[1]]),
               lambda z: np.array([[-np.sqrt(z[2]), -0.4, -0.5 * z[0] / np.sqrt(z[2])]])),
    "vdp_fb": ("vanderpol", [1, 2], lambda z: np.array([-0.5 * np.tanh(z[0]) * np.cos(z[1])]),
               lambda z: np.array([[-0.5 * np.cos(z[1]) / np.cosh(z[0]) ** 2, 0.5 * np.tanh(z[0]) * np.sin(z[1])]])),
    "vdp_pass": ("vanderpol", [4], lambda z: np.array([z[0]]), lambda z: np.array([[1.0]])),
    "tangential": ("twobody_lt", [3, 4, 5], *_tangential()),
    "shape_5_3_2": ("shape_5_3_2", [0, 5, 9], *_shape_law(3, True)),
    "shape_8_3_1": ("shape_8_3_1", [0, 8, 12], *_shape_law(3, True)),
    "shape_11_4_0": ("shape_11_4_0", [0, 11], *_shape_law(4, False)),
    "coupled16": ("coupled16", [0, 16, 20], *_shape_law(3, True)),
}


def law_value(name, rows):
    """K at every row of rows[..., N] -> [..., UV]"""
    _, varlocs, K, _ = LAWS[name]
    rows = np.asarray(rows, dtype=float)
    with np.errstate(all="ignore"):
        return np.array([K(r[varlocs]) for r in rows.reshape(-1, rows.shape[-1])]).reshape(rows.shape[:-1] + (-1,))


def law_lipschitz(name, rows):
    """|J_K| at every row, scattered to the state columns: [..., UV, n] (what a state error does to the controls)."""
    system, varlocs, _, JK = LAWS[name]
    n = SIZES[system][0]
    rows = np.asarray(rows, dtype=float)
    out = []
    for r in rows.reshape(-1, rows.shape[-1]):
        J = np.abs(JK(r[varlocs]))
        L = np.zeros((J.shape[0], n))
        for q, v in enumerate(varlocs):
            if v < n:
                L[:, v] = J[:, q]
        out.append(L)
    return np.array(out).reshape(rows.shape[:-1] + out[0].shape)


def closed_loop(f, fj, sizes, varlocs, K, JK):
    """(f_c, fj_c) on the full row [x, t, u, p]; the row's own u entries are not read."""
    n, uv, _ = sizes
    us = slice(n + 1, n + 1 + uv)
    varlocs = list(varlocs)

    def with_u(y):
        y = np.array(y, dtype=float)
        with np.errstate(all="ignore"):
            y[us] = K(y[varlocs])
        return y

    def f_c(y):
        return f(with_u(y))

    def fj_c(y):
        yc = with_u(y)
        fv, J = fj(yc)
        Jc = np.array(J, dtype=float)
        with np.errstate(all="ignore"):
            Jc[:, varlocs] += J[:, us] @ JK(yc[varlocs])
        Jc[:, us] = 0.0
        return fv, Jc
    return f_c, fj_c


def closed_loop_of(oracle, name):
    system, varlocs, K, JK = LAWS[name]
    f, fj = rhs(oracle, system)
    return closed_loop(f, fj, SIZES[system], varlocs, K, JK)


def control_bound(name, rows, B):
    """[..., UV]: 16 u |K(row)| + sum_j |dK/dx_j|(row) B[..., j] for rows[..., N] and state bounds B[..., n]; |K| is the largest
    component of the law's value at the row (the terms of a component, not the component itself, set its rounding error)."""
    Kv = np.abs(law_value(name, rows)).max(axis=-1, keepdims=True)
    return 16.0 * U * Kv + (law_lipschitz(name, rows) * np.asarray(B, dtype=float)[..., None, :]).sum(axis=-1)


# ------------------------------------------------------------------------------------------------ the fixture
_CACHE = None


def fixture():
    """(meta, cases) as propagate_checker.fixture: cases[name] holds the case's meta data (law, ode, sizes, ns, options) and the arrays of
    propagate_checker.ARRAYS, S of width C = N - 1 with exactly zero u columns, and for the fixed-step case xld, Sld."""
    global _CACHE
    if _CACHE is None:
        z = np.load(FIXTURE)
        meta = json.loads(str(z["meta"]))
        cases = {}
        for c in meta["cases"]:
            d = dict(c)
            for a in pck.ARRAYS:
                d[a] = z[f"{c['name']}.{a}"]
            for a in ("xld", "Sld"):
                d[a] = z[f"{c['name']}.{a}_hi"].astype(LD) + z[f"{c['name']}.{a}_lo"].astype(LD)
            cases[c["name"]] = d
        _CACHE = (meta, cases)
    return _CACHE


def case_names():
    return list(fixture()[1]) if os.path.exists(FIXTURE) else []


def restate_case(oracle, case):
    """propagate_checker.restate_case with the closed loop's callbacks: x64, x64_end, S64, steps64, steps64_end, steps64_stm, eS, and for
    a fixed-step case xld, Sld, d64, dS64."""
    f, fj = closed_loop_of(oracle, case["law"])
    rows, tfs, ns = case["rows"], case["tfs"], case["ns"]
    opt = pck.case_options(case)
    out = {}
    x64, _, st, status = pck.propagate_batch(f, fj, rows, tfs, ns, opt)
    assert (status == 0).all()
    out["x64"], out["steps64"] = x64, st
    x1, S64, st1, status = pck.propagate_batch(f, fj, rows, tfs, 1, opt, stm=True)
    assert (status == 0).all()
    out["x64_end"], out["S64"], out["steps64_end"], out["steps64_stm"] = x1[:, 0], S64, st1, st1
    eS = np.abs(S64.astype(LD) - case["S_exact"].astype(LD)).astype(float).max(axis=(1, 2))
    if opt["adaptive"]:
        for fac in pck.TOL_FACTORS:
            if fac == 1.0:
                continue
            _, Sf, _, status = pck.propagate_batch(f, fj, rows, tfs, 1, pck.case_options(case, fac), stm=True)
            assert (status == 0).all()
            eS = np.maximum(eS, np.abs(Sf.astype(LD) - case["S_exact"].astype(LD)).astype(float).max(axis=(1, 2)))
    else:
        xl, Sl, stl, status = pck.propagate_batch(f, fj, rows, tfs, 1, opt, dtype=LD, stm=True)
        assert (status == 0).all() and np.array_equal(stl, st1)
        out["xld"], out["Sld"] = xl[:, 0], Sl
        out["d64"] = np.abs(x1[:, 0].astype(LD) - xl[:, 0]).astype(float)
        out["dS64"] = np.abs(S64.astype(LD) - Sl).astype(float)
    out["eS"] = eS
    return out


def check_restatement(case, r, f_c):
    """propagate_checker.check_restatement (states within B / 4) and the same quarter for the STM and the two time columns of an adaptive
    case: the float64 restatement at AbsTol itself against the exact values.  `f_c`: the closed loop's right-hand side.  Returns the fractions of the QUARTER bounds used."""
    used = pck.check_restatement(case, r)
    opt = pck.case_options(case)
    if opt["adaptive"]:
        n = case["sizes"][0]
        S64 = r["S64"].astype(float)
        eS = np.maximum(np.asarray(r["eS"], dtype=float), 0.0)
        bS = pck.stm_bound(case["S_exact"], eS) / 4.0
        dS = np.abs(S64.astype(LD) - case["S_exact"].astype(LD)).astype(float)
        with np.errstate(invalid="ignore", divide="ignore"):
            used["stm"] = float(np.nanmax(np.where(bS > 0, dS / bS, np.where(dS == 0, 0.0, np.inf))))
        B = pck.state_bound(case["S_max"], r["steps64_end"][:, 0], opt["abs_tol"])
        b0, bf = pck.time_column_bounds(case["S_exact"], eS, case["f0"], case["Jxf_abs"], B, case["dtf_exact"])
        d0, df = pck.time_columns(f_c, case["rows"], case["tfs"], r["x64_end"], S64, dtype=float)
        for tag, got, ref, bound in (("dt0", d0, case["dt0_exact"], b0 / 4.0), ("dtf", df, case["dtf_exact"], bf / 4.0)):
            d = np.abs(got - ref)
            with np.errstate(invalid="ignore", divide="ignore"):
                used[tag] = float(np.nanmax(np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))))
        for tag in ("stm", "dt0", "dtf"):
            assert used[tag] <= 1.0, (case["name"], tag, used[tag])
    return used
