"""Per-entry check of the trajectory table against tests/golden/traj_table/<case>.npz (made by
tests/golden/make_golden_traj_table.py): the 50-digit value of EVERY entry of the interpolated rows and of their time derivatives at a
set of query times (every node time, both neighbours of every block boundary, the ends, random interior times, points outside both
ends), and for every entry a running error bound E in units of u = 2^-53.  ``load``, ``check`` and ``bound`` are pure numpy; nothing
under test is touched here.

    bound(E, kind) = kappa_kind * u * E          an entry with E = 0 has no rounded term: it must be EXACTLY the stored value
                                                 (the time's derivative 1.0, BlockConstant controls and their derivative 0.0)

The two kappa are measured, not chosen, and never on the device (``measure_constants``): ``model`` below is the algorithm the head of
csrc/interp_kernels.h documents, in float64 -- s, h and 1 / h in float64, every basis value the 50-digit polynomial at that float64 s
rounded once, the sums over the nodes in float64 in the kernel's order, the right-hand side the oracle's (tests/interp_checker.py:
oracle_rhs; the fixture generator's restatement rounded to float64 for a family the oracle does not hold).  It is run over the whole
fixture, the worst |model - ref| / (u E) per quantity is multiplied by 8 and rounded up to a power of two.  The factor 8 is the
project's (tests/defect_checker.py); here it stands for the device's right-hand side, which is generated code with its own operation
order and FMA contraction.  The measured ratios and the constants are in every fixture's metadata (``constants``) and in DESIGN.md
section 2; tests/test_traj_table_cpu.py holds KAPPA below to them.

``model`` takes mutations (tests/test_traj_table_cpu.py: each must put an entry of a named case over its bound): plain double Horner,
a boundary time given to the block that starts there, BlockConstant from the block's last row, a ``tb`` entry left at zero, the search
run with dir = +1."""
from __future__ import annotations

import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "traj_table")
U = 2.0 ** -53
KINDS = ("val", "der")
MODE_CS = {"Trapezoidal": 2, "LGL3": 2, "LGL5": 3, "LGL7": 4}
ORACLE_ODES = ("brachistochrone", "reentry", "twobody_lt", "betts_lowthrust", "synthetic32", "vanderpol", "coupled12")

# 8 x (worst ratio of the float64 model), rounded up to a power of two -- see measure_constants() and the fixtures' metadata
KAPPA = {"val": 8.0, "der": 8.0}


def all_cases():
    return sorted(fn[:-4] for fn in os.listdir(DIR) if fn.endswith(".npz"))


_CACHE = {}


def load(name: str):
    """The fixture of a case: dict of traj[nodes, N], times[nq], block[nq], outside, val / der[nq, N], the bounds valE / derE (float32,
    rounded upward), meta, and from it xv, N, cs, K, nb.  Loaded once; treat as read-only."""
    if name not in _CACHE:
        with np.load(os.path.join(DIR, name + ".npz")) as f:
            d = {k: f[k] for k in f.files}
        d["meta"] = m = json.loads(str(d["meta"]))
        d["outside"] = int(d["outside"])
        d["xv"], d["N"], d["cs"] = m["sizes"][0], d["traj"].shape[1], MODE_CS[m["mode"]]
        d["K"] = d["cs"] - 1
        d["nb"] = (d["traj"].shape[0] - 1) // d["K"]
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = d
    return _CACHE[name]


def bound(E, kind):
    return KAPPA[kind] * U * np.asarray(E, dtype=np.float64)


def check(got, fixture, query_ids, kind, kappa=None):
    """Every entry of ``got[n, N]`` (no sampling) against fixture query ``query_ids[r]`` for row r.  -> dict(worst = the largest
    |got - ref| / bound (inf for a difference at an entry with E = 0 or a NaN), where = (row, column) of it, over = the number of
    entries over their bound, n = entries compared)."""
    ids = np.asarray(query_ids, dtype=np.int64)
    got = np.asarray(got, dtype=np.float64).reshape(ids.size, -1)
    ref, E = fixture[kind][ids], fixture[kind + "E"][ids].astype(np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    b = (KAPPA[kind] if kappa is None else kappa) * U * E
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0.0, 0.0, d / b)                  # (b = 0, d > 0: inf;  NaN from the device: stays NaN and counts below)
    over = int((~(q <= 1.0)).sum())
    q = np.where(np.isnan(q), np.inf, q)
    i, j = np.unravel_index(int(q.argmax()), q.shape) if q.size else (0, 0)
    return dict(worst=float(q.max()) if q.size else 0.0, where=(int(i), int(j)), over=over, n=int(got.size))


def pow2_ceil(x: float) -> float:
    return 2.0 ** math.ceil(math.log2(x))


# --------------------------------------------------------------------------- the float64 model of the documented algorithm
def _weights(cs):
    t = json.load(open(os.path.join(HERE, "golden", "lgl_tables.json")))["tables"][str(cs)]
    return [t[k] for k in ("Cardinal_XPower_Weights", "Cardinal_DXPower_Weights", "Cardinal_UPolyPower_Weights")]


def _poly_once(w, s):
    """(p(s), p'(s)) of the polynomial with coefficients w (highest power first): exact at the float64 s, rounded once"""
    import mpmath as mp
    with mp.workdps(50):
        x, p, d = mp.mpf(s), mp.mpf(0), mp.mpf(0)
        for c in w:
            d = d * x + p
            p = p * x + mp.mpf(c)
        return float(p), float(d)


def _poly_plain(w, s):
    """the same by plain Horner in float64, the derivative from its own coefficients k w_k"""
    n = len(w)
    p, d = np.float64(w[0]), np.float64(0.0)
    for k in range(1, n):
        d = d * s + np.float64(n - k) * np.float64(w[k - 1])
        p = p * s + np.float64(w[k])
    return float(p), float(d)


def restated_rhs(ode: str):
    """rows -> f(rows): the fixture generator's restatement in 50 digits, rounded to float64 (a family the oracle does not hold)"""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden_traj_table as g

    def rhs(rows):
        return np.array([[float(v.v) for v in g.rhs_S(ode, row)] for row in np.atleast_2d(rows)])
    return rhs


def rhs_of(oracle, ode: str):
    import interp_checker as ick
    return ick.oracle_rhs(oracle, ode) if ode in ORACLE_ODES else restated_rhs(ode)


def model(f, rhs, horner="once", boundary="end", blocked_row="first", tb_zero=None, direction=None):
    """(val[nq, N], der[nq, N], outside) of fixture ``f`` by the documented algorithm in float64.  Mutations: horner="plain";
    boundary="start" (a boundary time goes to the block that starts there); blocked_row="last"; tb_zero=k (tb[k] left at 0.0);
    direction=+1.0 (the search's direction, whatever the data's)."""
    traj, times = f["traj"], f["times"]
    xv, N, cs, K, nb = f["xv"], f["N"], f["cs"], f["K"], f["nb"]
    blocked = bool(f["meta"]["blocked"])
    Xw, DXw, Uw = _weights(cs)
    poly = _poly_once if horner == "once" else _poly_plain
    F = rhs(traj)
    tb = traj[::K, xv].copy()
    if tb_zero is not None:
        tb[tb_zero] = 0.0
    t0, tf = tb[0], tb[nb]
    dr = np.float64((1.0 if tf > t0 else -1.0) if direction is None else direction)
    val, der = np.zeros((times.size, N)), np.zeros((times.size, N))
    outside = 0
    with np.errstate(all="ignore"):
        for q, tau in enumerate(times):
            dtau = dr * tau
            lo, hi = 0, nb - 1
            while lo < hi:
                mid = (lo + hi) >> 1
                if (dtau <= dr * tb[mid + 1]) if boundary == "end" else (dtau < dr * tb[mid + 1]):
                    hi = mid
                else:
                    lo = mid + 1
            outside += int(not (dtau >= dr * t0 and dtau <= dr * tf))
            tb0 = tb[lo]
            h = tb[lo + 1] - tb0
            s = (tau - tb0) / h
            ih = np.float64(1.0) / h
            rows, fr = traj[lo * K:lo * K + cs], F[lo * K:lo * K + cs]
            v, dv = np.zeros(N), np.zeros(N)
            for i in range(cs):
                phi, dphi = poly(Xw[i], s)
                psi, dpsi = poly(DXw[i], s)
                ups, dups = poly(Uw[i], s)
                phi, dphi, hpsi, dpsi = np.float64(phi), np.float64(dphi) * ih, np.float64(psi) * h, np.float64(dpsi)
                ups, dups = np.float64(ups), np.float64(dups) * ih
                v[:xv] = (v[:xv] + rows[i, :xv] * phi) + fr[i] * hpsi
                dv[:xv] = (dv[:xv] + rows[i, :xv] * dphi) + fr[i] * dpsi
                v[xv + 1:] = v[xv + 1:] + rows[i, xv + 1:] * ups
                dv[xv + 1:] = dv[xv + 1:] + rows[i, xv + 1:] * dups
            v[xv], dv[xv] = tb0 + h * s, 1.0
            if blocked:
                v[xv + 1:], dv[xv + 1:] = rows[0 if blocked_row == "first" else K, xv + 1:], 0.0
            val[q], der[q] = v, dv
    return val, der, outside


def measure_constants():
    """dict(worst = {kind: worst |model - ref| / (u E) over every entry of every fixture}, at = where, kappa = {kind: ...},
    inexact = entries with E = 0 the model does not reproduce exactly (must be 0))."""
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import bindings as ob
    ob.build()
    worst, at, inexact = {k: 0.0 for k in KINDS}, {k: None for k in KINDS}, 0
    for name in all_cases():
        f = load(name)
        val, der, outside = model(f, rhs_of(ob, f["meta"]["ode"]))
        assert outside == f["outside"], name
        ids = np.arange(f["times"].size)
        for k, got in (("val", val), ("der", der)):
            zero = f[k + "E"] == 0
            inexact += int(np.sum(got[zero] != f[k][zero]))
            r = check(np.where(zero, f[k], got), f, ids, k, kappa=1.0)
            if r["worst"] > worst[k]:
                worst[k], at[k] = r["worst"], [name, r["where"][0], r["where"][1]]
    kappa = {k: pow2_ceil(8.0 * worst[k]) for k in KINDS}
    return dict(worst=worst, at=at, kappa=kappa, inexact=inexact, factor=8.0)
