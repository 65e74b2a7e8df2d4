"""Generate tests/golden/root/root.npz: the cases of tests/root_cases.py (``vf.ScalarRootFinder``, ``astro.KeplerPropagator``) at
NAPP = 193 points each, with value, Jacobian and adjoint Hessian lam^T H at 50 digits and a bound per entry (run once; commit the .npz).

Reference values.  Every equation is solved by Newton's iteration carried out in ``make_golden.D2`` arithmetic -- second-order forward
AD over mpf -- from the guess as a CONSTANT, until two consecutive iterates agree to 1e-40 in value and in every first and second
derivative: the derivatives of the converged iteration are those of its fixed point.  That is another route than the implicit-function
rule under test (vf/ir.py), and nothing of the package enters: the functions below are a second statement of tests/root_cases.py over a
small namespace of mathematical functions (mpf / D2 here, Python floats for the float64 restatement).

Bounds, none measured against the code under test.  The float64 iteration stops with |F| < tol: what it returns is the exact root of
``F - eps`` for some |eps| < tol, known to 4u|s*| -- an error of the root of at most ``delta = tol / |F_s| + 4u |s*|``.  The implicit
function of ``F = eps`` has the formulas of that of ``F = 0`` evaluated at the moved root, so the reference run is repeated on
``F -+ eta`` (eta = 1e-25, per root) and the central difference is de/deps of every entry; an entry's bound is
``sum over roots |de/deps| (tol + 4u |s*| |F_s|)`` plus the rounding allowance ``tests/vf_cases.py`` gives entries of that magnitude:
``tolerance(E_ref) x max(|ref_ij|, 1e-3 max|ref|)``, E_ref being the error, in that file's metric, of the SAME D2 iteration run in
53-bit arithmetic, the worst over the case's points, per case and array as in that file.  Its condition on the sampling domain is applied
point by point: a draw at which 16 x E_ref exceeds CAP_DEVICE (the cap of the device tests, which use these bounds) is badly conditioned
and replaced, as a case of that file gets another domain; the arcs of the propagator differ by orders of magnitude in conditioning.  The cases use tol = 1e-14 and an ``iters`` for which the float64 restatement of the loop (``solve_float``) stops on
the tolerance, not on the count, at every point: a drawn point that fails this is replaced by the next draw, the bound is never widened.

``kepler_prop`` is ``KeplerPropagator(1.0, roottol=1e-14)``: the three Kepler arcs of tests/golden/propagate/propagate.npz first, then
elliptic arcs with alpha in [0.05, 1.4] and hyperbolic arcs with alpha in [-1.5, -0.05], dt of both signs and such that the anomaly
swept is O(1) -- drawn from those ranges, so no point lies near the parabolic band.  Asserted here: the three fixture arcs reproduce ``x_exact``, ``S_exact[:, :6]`` and
``dtf_exact`` of that file, which stores them rounded to float64, to that rounding (|difference| <= 2^-53 |value| + 1e-20).  One extra
set, values only, lies INSIDE the band |psi| < conictol (alpha in [0, 3e-12] and |psi| < conictol / 2; the logarithmic guess of the hyperbolic side does not
reach the root in 19 passes that close to the parabola, so that side has no points): the reference there is the propagator with the
exact Stumpff functions, the bound twice its 50-digit difference to the propagator with the constants 1/2 and 1/6, plus the root and
rounding terms above.

The run that wrote the committed file: no draw replaced in kepler_eq, cubic, given_step, composed and twice; in kepler_prop 7 draws
replaced because the float64 loop ran out of its 19 passes and 9 because they were badly conditioned (209 draws for 190 random arcs);
the float64 loop needs at most 6 / 8 / 15 / 4 / 6 / 16 passes in the six cases.  Largest E_ref: kepler_eq 3.2e-16 / 2.6e-15 / 8.8e-15
(f / J / H), cubic 2.2e-16 / 2.9e-16 / 4.1e-14, given_step 2.2e-16 / 3.0e-16 / 1.0e-14, composed 1.5e-15 / 4.4e-14 / 1.9e-14, twice
8.6e-14 / 1.4e-14 / 1.3e-13, kepler_prop 3.8e-13 / 4.4e-13 / 6.0e-13.

Usage:  python tests/golden/make_golden_root.py
"""
from __future__ import annotations

import math
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import vf_cases  # noqa: E402
from make_golden import D2, MP  # noqa: E402

mp.mp.dps = 50
NAPP = vf_cases.NAPP
U = 2.0 ** -53
TOL = 1.0e-14
ETA = mp.mpf(10) ** -25
AGREE = mp.mpf(10) ** -40
CONICTOL = 1.0e-11
NBAND = 16
PATH = os.path.join(HERE, "root", "root.npz")
ITERS = {"kepler_eq": 30, "cubic": 30, "given_step": 60, "composed": 30, "twice": 30, "kepler_prop": 19}   # tests/root_cases.py reads these from the file


# --------------------------------------------------------------------------- the two namespaces
class MPX(MP):
    """make_golden.MP and what the propagator needs beside it"""

    @staticmethod
    def sinh(a):
        s, c = mp.sinh(a.v), mp.cosh(a.v)
        return a._un(s, c, s)

    @staticmethod
    def cosh(a):
        s, c = mp.sinh(a.v), mp.cosh(a.v)
        return a._un(c, s, c)

    @staticmethod
    def log(a):
        return a._un(mp.log(a.v), 1 / a.v, -1 / (a.v * a.v))


class FL:
    sin, cos, sinh, cosh, log, exp, sqrt = math.sin, math.cos, math.sinh, math.cosh, math.log, math.exp, math.sqrt


def val(x):
    return x.v if isinstance(x, D2) else x


# --------------------------------------------------------------------------- the equations: (F, F_s, the step's divisor or None)
def _stumpff(psi, K, const_band=True):
    p = val(psi)
    if p > CONICTOL or (not const_band and p > 0):
        sq = K.sqrt(psi)
        return (1.0 - K.cos(sq)) / psi, (sq - K.sin(sq)) / (sq * psi)
    if p < -CONICTOL or (not const_band and p < 0):
        sh = K.sqrt(-psi)
        return (1.0 - K.cosh(sh)) / psi, (K.sinh(sh) - sh) / (sh * (-psi))
    return 0.5, 1.0 / 6.0


def _universal(s, p, K, const_band=True):
    alpha, sigma, r, smdt = p
    s2 = s * s
    psi = alpha * s2
    c2, c3 = _stumpff(psi, K, const_band)
    rho = s2 * c2 + sigma * s * (1.0 - psi * c3) + r * (1.0 - psi * c2)
    return smdt - s2 * s * c3 - sigma * s2 * c2 - r * s * (1.0 - psi * c3), rho, s2, psi, c2, c3


EQS = {
    "kepler": (lambda s, p, K: s - p[0] * K.sin(s) - p[1], lambda s, p, K: 1.0 - p[0] * K.cos(s), None),
    "cubic": (lambda s, p, K: s * s * s + p[0] * s - p[1], lambda s, p, K: 3.0 * (s * s) + p[0], None),
    "cubic_given": (lambda s, p, K: s * s * s + p[0] * s - p[1], lambda s, p, K: 3.0 * (s * s) + p[0],
                    lambda s, p, K: 3.0 * (s * s) + p[0] + 0.1),
    "wave": (lambda s, p, K: s + 0.5 * p[1] * K.sin(s) - p[0], lambda s, p, K: 1.0 + 0.5 * p[1] * K.cos(s), None),
    "lag": (lambda s, p, K: s - 0.4 * p[1] * K.sin(s) - p[0], lambda s, p, K: 1.0 - 0.4 * p[1] * K.cos(s), None),
    "universal": (lambda s, p, K: _universal(s, p, K)[0], lambda s, p, K: -1.0 * _universal(s, p, K)[1], None),
    "universal_exact": (lambda s, p, K: _universal(s, p, K, False)[0], lambda s, p, K: -1.0 * _universal(s, p, K, False)[1], None),
}


# --------------------------------------------------------------------------- the functions (a second statement of tests/root_cases.py)
def _propagator(y, K, solve, exact_stumpff=False):
    R, V, dt = y[0:3], y[3:6], y[6]
    rn = K.sqrt(R[0] * R[0] + R[1] * R[1] + R[2] * R[2])
    rv = R[0] * V[0] + R[1] * V[1] + R[2] * V[2]
    al = 2.0 / rn - (V[0] * V[0] + V[1] * V[1] + V[2] * V[2])
    if val(al) >= 0.0:
        guess = dt * al
    else:
        sgn = 1.0 if val(dt) > 0 else (-1.0 if val(dt) < 0 else 0.0)
        am = -1.0 / al
        guess = sgn * K.sqrt(am) * K.log(-2.0 * al * dt / (rv + sgn * K.sqrt(am) * (1.0 - rn * al)))
    p = [al, rv, rn, dt]
    x = solve("universal_exact" if exact_stumpff else "universal", guess, p)
    _, rho, x2, psi, c2, c3 = _universal(x, p, K, not exact_stumpff)
    f, g = 1.0 - x2 * c2 / rn, dt - x2 * x * c3
    fd, gd = x * (psi * c3 - 1.0) / (rho * rn), 1.0 - x2 * c2 / rho
    return [f * R[i] + g * V[i] for i in range(3)] + [fd * R[i] + gd * V[i] for i in range(3)]


def _twice(y, K, solve):
    s1 = solve("cubic", y[0], [1.0 + y[1] * y[1], y[2]])
    s2 = solve("lag", y[0], [s1, y[3]])
    return [s1 * y[3] + s2, s2 * s2 - s1 * y[1]]


def _composed(y, K, solve):
    s = solve("wave", y[0], [K.sin(y[1]) * y[2], y[3] * y[3]])
    return [K.exp(-s) * y[4] + s * s]


FUNCS = {
    "kepler_eq": (lambda y, K, solve: [solve("kepler", y[0], [y[1], y[2]])], 3, 1),
    "cubic": (lambda y, K, solve: [solve("cubic", y[0], [y[1], y[2]])], 3, 1),
    "given_step": (lambda y, K, solve: [solve("cubic_given", y[0], [y[1], y[2]])], 3, 1),
    "composed": (_composed, 5, 1),
    "twice": (_twice, 4, 2),
    "kepler_prop": (_propagator, 7, 6),
}


# --------------------------------------------------------------------------- three ways to solve
def solve_float(iters, log):
    """the loop as the float64 code runs it; log gets (stopped on the tolerance?, passes) per root"""
    def solve(eq, guess, p):
        F, Fs, step = EQS[eq]
        s, hit = float(guess), False
        for k in range(iters):
            r = F(s, p, FL)
            if abs(r) < TOL:
                hit = True
                break
            s -= r / (step or Fs)(s, p, FL)
        log.append((hit, k))
        return s
    return solve


def solve_exact(n, eps, log, passes=None):
    """Newton in D2 from the guess as a constant, on F - eps[r] for the r-th root of the function; to agreement (log gets
    (s*, F_s(s*), passes)) or, where `passes` is given, that many passes per root (the 53-bit run)"""
    def solve(eq, guess, p):
        F, Fs, _ = EQS[eq]
        r = len(log)
        e = eps.get(r, 0)
        s = D2.const(val(guess), n)
        k = 0
        while True:
            k += 1
            new = s - (F(s, p, MPX) - e) / Fs(s, p, MPX)
            if passes is None:
                gap = max([abs(new.v - s.v)] + [abs(a) for a in (new.g - s.g)] + [abs(a) for a in (new.h - s.h).ravel()])
                s = new
                if gap < AGREE:
                    break
                assert k < 400, (eq, "no convergence")
            else:
                s = new
                if k >= passes[r]:
                    break
        log.append((s.v, val(Fs(s, p, MPX)), k))
        return s
    return solve


def arrays(outs, lam, n):
    f = np.array([o.v for o in outs], dtype=object)
    J = np.array([o.g for o in outs], dtype=object).reshape(len(outs), n)
    H = sum(mp.mpf(float(l)) * o.h for l, o in zip(lam, outs))
    return f, J, H


def point(name, y, lam, func=None, **kw):
    """(reference arrays, sensitivity terms, 53-bit arrays) of one point; None where the float64 loop does not stop on the tolerance"""
    fn, n, _ = FUNCS[name]
    fn = func or fn
    flog = []
    fn([float(v) for v in y], FL, solve_float(ITERS[name], flog), **kw)
    if not all(h for h, _ in flog):
        return None
    Y = [D2.var(float(v), i, n) for i, v in enumerate(y)]
    log = []
    ref = arrays(fn(Y, MPX, solve_exact(n, {}, log), **kw), lam, n)
    sens = [np.zeros(a.shape) for a in ref]
    for r, (s, fs, _) in enumerate(log):
        hi = arrays(fn(Y, MPX, solve_exact(n, {r: ETA}, []), **kw), lam, n)
        lo = arrays(fn(Y, MPX, solve_exact(n, {r: -ETA}, []), **kw), lam, n)
        w = TOL + 4.0 * U * float(abs(s) * abs(fs))
        for k in range(3):
            sens[k] = sens[k] + np.vectorize(lambda a, b: float(abs(a - b) / (2 * ETA)))(hi[k], lo[k]).astype(float) * w
    with mp.workprec(53):
        dbl = arrays(fn(Y, MPX, solve_exact(n, {}, [], passes=[k + 2 for _, _, k in log]), **kw), lam, n)
    e_ref = []
    for a in range(3):
        hi = np.vectorize(float)(ref[a]).astype(float)[None]
        d64 = hi + np.vectorize(lambda x, y: float(x - y))(dbl[a], ref[a]).astype(float)[None]       # (the 53-bit result, to first order)
        e_ref.append(float(vf_cases.entry_errors(d64, hi).max()))
    return ref, sens, dbl, max(k for _, k in flog), e_ref


# --------------------------------------------------------------------------- the points
def draw(name, rng):
    if name == "kepler_eq":
        M = rng.uniform(-3.14, 3.14)
        return [M, rng.uniform(0.0, 0.9), M]
    if name in ("cubic", "given_step"):
        return [0.0, rng.uniform(0.5, 2.0), rng.uniform(-2.0, 2.0)]
    if name == "composed":
        return [rng.uniform(-0.5, 0.5)] + list(rng.uniform(-1.0, 1.0, 4))
    if name == "twice":
        return [rng.uniform(-0.3, 0.3)] + list(rng.uniform(0.2, 1.0, 3))      # (one sign: the sums of the outputs and of their second derivatives do not cancel)
    raise KeyError(name)


def draw_arc(rng, hyperbolic):
    while True:
        R = rng.normal(size=3)
        R *= rng.uniform(0.7, 1.5) / np.linalg.norm(R)
        r = np.linalg.norm(R)
        alpha = rng.uniform(-1.5, -0.05) if hyperbolic else rng.uniform(0.05, min(1.4, 1.8 / r))
        V = rng.normal(size=3)
        V *= np.sqrt(2.0 / r - alpha) / np.linalg.norm(V)
        if np.linalg.norm(np.cross(R, V)) < 0.3:
            continue
        # (the anomaly swept, about |alpha|^1.5 |dt|, between 0.8 and 2.4: |psi| = O(1), away from the cancellation in the Stumpff
        #  functions at small |psi|, which is a matter of conditioning and not of the root finder)
        dt = rng.uniform(0.8, 2.4) / abs(alpha) ** 1.5 * rng.choice([-1.0, 1.0])
        y = np.concatenate([R, V, [dt]])
        a = 2.0 / np.linalg.norm(y[:3]) - y[3:6] @ y[3:6]          # (as float64 forms it from the rounded state)
        if (a <= -0.05) if hyperbolic else (a >= 0.05):
            return list(y)


def draw_band(rng):
    R = rng.normal(size=3)
    R *= rng.uniform(0.8, 1.3) / np.linalg.norm(R)
    V = rng.normal(size=3)
    V *= np.sqrt(2.0 / np.linalg.norm(R)) / np.linalg.norm(V)
    V *= 1.0 - rng.uniform(0.02e-12, 0.2e-12)               # alpha = 2 eps |V|^2: about 0.06e-12 .. 1e-12
    return list(np.concatenate([R, V, [rng.uniform(0.3, 0.9) * rng.choice([-1.0, 1.0])]]))


def fixture_arcs():
    fx = np.load(os.path.join(HERE, "propagate", "propagate.npz"))
    out = []
    for c in ("kepler_quarter", "kepler_full", "kepler_back"):
        row, tf = fx[c + ".rows"][0], fx[c + ".tfs"][0]
        out.append((list(row[:6]) + [tf - row[6]], fx[c + ".x_exact"][0, -1], fx[c + ".S_exact"][0][:, :6], fx[c + ".dtf_exact"][0]))
    return out


def same_as_stored(mine, stored, what):
    for a, b in zip(np.ravel(mine), np.ravel(stored)):
        assert abs(a - mp.mpf(float(b))) <= mp.mpf(2) ** -53 * abs(a) + mp.mpf(10) ** -20, (what, a, b)


def split(v):
    hi = float(v)
    return hi, float(v - mp.mpf(hi))


def main():
    out = {"tol": TOL, "conictol": CONICTOL}
    for ci, name in enumerate(FUNCS):
        fn, n, no = FUNCS[name]
        rng = np.random.default_rng(7100 + ci)
        P, L, recs, replaced, illcond, arcs = [], [], [], 0, 0, fixture_arcs() if name == "kepler_prop" else []
        while len(P) < NAPP:
            k = len(P)
            if name == "kepler_prop":
                y = arcs[k][0] if k < 3 else draw_arc(rng, hyperbolic=bool(k % 2))
            else:
                y = draw(name, rng)
            lam = rng.uniform(0.25, 2.0, no) * rng.choice([-1.0, 1.0], no)
            rec = point(name, y, lam)
            if rec is None:
                assert not (name == "kepler_prop" and k < 3), "a fixture arc does not stop on the tolerance"
                replaced += 1
                continue
            if vf_cases.MARGIN * max(rec[4]) > vf_cases.CAP_DEVICE:      # vf_cases' condition on the sampling domain, point by point
                assert not (name == "kepler_prop" and k < 3), "a fixture arc is badly conditioned"
                illcond += 1
                continue
            if name == "kepler_prop" and k < 3:
                f, J, _ = rec[0]
                same_as_stored(f, arcs[k][1], "x_exact")
                same_as_stored(J[:, :6], arcs[k][2], "S_exact")
                same_as_stored(J[:, 6], arcs[k][3], "dtf_exact")
            P.append(y)
            L.append(lam)
            recs.append(rec)
            if k % 32 == 0:
                print(f"  {name}: point {k}", flush=True)
        # the rounding allowance: vf_cases' metric and rule, E_ref from the 53-bit run
        ref = [np.array([r[0][a] for r in recs], dtype=object) for a in range(3)]
        dbl = [np.array([r[2][a] for r in recs], dtype=object) for a in range(3)]
        sens = [np.array([r[1][a] for r in recs]) for a in range(3)]
        for a, key in enumerate(("f", "J", "H")):
            hi = np.vectorize(float)(ref[a]).astype(float)
            lo = np.vectorize(lambda v: float(v - mp.mpf(float(v))))(ref[a]).astype(float)
            e_pt = np.array([r[4][a] for r in recs])
            e_typ, e_ref = float(np.median(e_pt)), float(e_pt.max())
            tol = vf_cases.tolerance(e_ref, vf_cases.CAP_DEVICE)         # per case and array, as vf_cases sets it
            flat = np.abs(hi).reshape(NAPP, -1)
            scale = np.maximum(np.abs(hi), 1.0e-3 * flat.max(axis=1).reshape((NAPP,) + (1,) * (hi.ndim - 1)))
            bound = (sens[a] + tol * scale) * (1.0 + 2.0 ** -40)
            bound[hi == 0.0] = np.where(sens[a][hi == 0.0] == 0.0, 0.0, bound[hi == 0.0])   # a structural zero stays one
            out[f"{name}_{key}"], out[f"{name}_{key}lo"], out[f"{name}_{key}B"] = hi, lo, bound
            out[f"{name}_{key}tol"] = tol
            print(f"{name} {key}: E_ref median {e_typ:.3g}, largest {e_ref:.3g}; largest root term {sens[a].max():.3g}, largest bound {bound.max():.3g}", flush=True)
        out[f"{name}_P"], out[f"{name}_lam"], out[f"{name}_iters"] = np.array(P, dtype=float), np.array(L), ITERS[name]
        print(f"{name}: {replaced} draws replaced (the loop ran out of passes), {illcond} (badly conditioned); the float64 loop needs at most {max(r[3] for r in recs)} passes of {ITERS[name]}", flush=True)
    # ---- inside the parabolic band: values only
    rng = np.random.default_rng(7200)
    P, F, B = [], [], []
    ftol = float(out["kepler_prop_ftol"])
    while len(P) < NBAND:
        y = draw_band(rng)
        a = 2.0 / np.linalg.norm(y[:3]) - np.dot(y[3:6], y[3:6])
        rec = point("kepler_prop", y, np.ones(6)) if 0.0 <= a < 3.0e-12 else None
        if rec is None:
            continue
        const = rec[0][0]
        Y = [D2.var(float(v), i, 7) for i, v in enumerate(y)]
        log = []
        with mp.workdps(100):           # (the exact Stumpff functions cancel twelve digits at |psi| = 1e-12, more in their derivatives)
            exact = arrays(_propagator(Y, MPX, solve_exact(7, {}, log), exact_stumpff=True), np.ones(6), 7)[0]
        if abs(a * float(log[0][0]) ** 2) >= 0.5 * CONICTOL:          # (a long way along the parabola: not safely inside the band)
            continue
        hi = np.array([float(v) for v in exact])
        diff = np.array([float(abs(x - c)) for x, c in zip(exact, const)])
        P.append(y)
        F.append(hi)
        B.append((2.0 * diff + rec[1][0] + ftol * np.maximum(np.abs(hi), 1.0e-3 * np.abs(hi).max())) * (1.0 + 2.0 ** -40))
    out["kepler_prop_band_P"], out["kepler_prop_band_f"], out["kepler_prop_band_fB"] = np.array(P), np.array(F), np.array(B)
    print(f"band: {NBAND} points, bounds {np.min(B):.3g} .. {np.max(B):.3g}", flush=True)
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
