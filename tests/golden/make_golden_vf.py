"""Generate tests/golden/vf_ops.npz: the 50-digit reference of the DSL operation tests (run once; commit the .npz).

Every case of tests/vf_cases.py is written here a SECOND time, over sympy, from the formulas in that file's text -- nothing of
``asset_asrl_amd.vf`` is imported: no expression graph, no differentiation rule, no evaluator, no printer.  sympy differentiates the
second statement symbolically; the derivatives are evaluated with mpmath at 50 digits and rounded ONCE to double.  Per case, for all
193 points:

    Y[napp, N]   the points            LAM[napp, n]   the multipliers
    f[napp, n]   J[napp, n, N] = df/dy   g[napp, N] = J^T lam   H[napp, N(N+1)/2] = sum_k lam_k d2f_k/dy2, lower triangle by rows

Constants are the doubles the DSL definitions hold (``sympy.Rational(0.7)`` is the exact value of the double 0.7), so the reference
is the same real function.  The piecewise cases (ifelse, abs, sign) pick their branch with a Python ``if`` on the point and
differentiate that branch only, as the reference implementation's IfElseFunction does: the branch not taken is never evaluated, so
the rows on a threshold (``guarded``: y0 = 0.0, y1 = 0.5, y2 = 0.0) are finite by construction.  Every stored number is asserted
finite; no point is left out.

E_ref[case, array]: the worst per-entry error (tests/vf_cases.py: entry_errors) of the SAME sympy expressions evaluated in plain
double (lambdified over ``math``) against their 50-digit values -- the conditioning of the points measured from the reference
alone.  The tests allow 16 x E_ref, floored at 1e-14 and capped at 1e-12 (host) / 1e-11 (device).  Measured (this file, this seed):

    case        E_ref f    E_ref J    E_ref g    E_ref H
    trig        8.6e-15    3.9e-14    8.5e-15    3.1e-14    (1 redrawn)
    hyper       3.0e-14    1.5e-14    4.0e-14    3.1e-14    (1 redrawn)
    inverse     6.1e-15    1.2e-14    1.7e-14    3.7e-14    (0 redrawn)
    powers      1.6e-14    2.7e-14    2.4e-14    3.6e-14    (0 redrawn)
    recip       4.9e-14    2.1e-14    2.5e-14    4.6e-14    (0 redrawn)
    piecewise   3.7e-14    2.2e-16    2.0e-14    4.4e-14    (1 redrawn)
    guarded     6.0e-16    2.2e-16    5.0e-15    3.4e-14    (0 redrawn)
    composed    4.0e-15    4.4e-14    4.2e-14    4.3e-14    (7 redrawn)
    bigbody     1.8e-15    2.3e-14    3.0e-14    4.3e-14    (1 redrawn)

"redrawn": candidates the sampler rejected because the reference's own plain-double evaluation was off by more than COND_LIMIT
(golden_case) -- with the whole boxes E_ref reached 1.6e-13 and 16 x E_ref passed the host cap, so the domains exclude those slabs.

Size: 193 points x (f, J, g, H) x nine cases are about 49 000 full-entropy doubles; the file is ~415 KB (H as its lower triangle only,
deflate level 9), well above the 88 KB of synthetic32_LGL7.npz and well below the 1 MiB limit of a committed file.  Fewer points or
arrays would be a weaker check, so the size gave way.

The second part of the file is the reference of csrc/asset_math.h (asset_sin / asset_cos / asset_tan): the argument sets ``am_x``
(``am_set`` names the set of every argument) and sin, cos, tan at 50 digits as a double plus a float32 remainder (hi + lo), so
that the header's absolute bound of 2e-16 is not blurred by the half ulp a single double would lose; and 1 + tan^2 as one double.

Usage:  python tests/golden/make_golden_vf.py        (writes tests/golden/vf_ops.npz, bit for bit the committed file)
"""
from __future__ import annotations

import io
import math
import os
import sys
import zipfile

import mpmath as mp
import numpy as np
import sympy as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import vf_cases  # noqa: E402   (sizes, sampling domains, the metric: no expression code)

mp.mp.dps = 50
NAPP = vf_cases.NAPP


def R(x: float):
    """The exact value of the double x."""
    return sp.Rational(float(x))


# --------------------------------------------------------------------------- the functions, second statement (y: symbols, p: the point)

def ref_trig(y, p):
    w = R(0.7) * y[0] + y[1] * y[2]
    return [sp.sin(w) * sp.cos(w) + y[2],
            sp.sin(y[0] * y[1] - R(0.3) * y[2]) * y[2],
            sp.tan(R(0.5) * y[0] + R(0.25) * y[1] * y[2]) + sp.cos(y[1] + y[2] ** 2) * y[0]]


def ref_hyper(y, p):
    return [sp.exp(R(0.5) * y[0] * y[1]) * sp.log(R(1.5) + y[2] + y[0] ** 2) + sp.tanh(y[1] - R(0.4) * y[2]),
            sp.sinh(y[0] + R(0.3) * y[1] * y[2]) * sp.cosh(R(0.6) * y[1] - y[2]) + sp.tanh(y[0] * y[2]) * sp.log(2 + y[1])]


def ref_inverse(y, p):
    return [sp.asin(R(0.9) * y[0] * y[1]) * y[2] + sp.acos(R(0.45) * (y[0] + y[1])),
            sp.atan(y[0] * y[2] + 2 * y[1]) + sp.atan2(y[2], y[3]) * y[0]]


def ref_powers(y, p):
    r = sp.sqrt(y[0] ** 2 + y[1] ** 2 + y[2] ** 2)
    return [y[0] ** 3 * y[1] + y[1] ** 5 - y[2] ** 7 * y[0],
            y[2] / y[0] ** 2 + 1 / (y[1] * y[2]) ** 3 + (y[0] + y[1]) ** sp.Rational(3, 2),
            y[1] / sp.sqrt(y[0] * y[2]) + (y[1] + y[2] / 2) ** sp.Rational(5, 2),
            r ** 3 * y[0] + y[1] / r + y[0] / r ** 3 * y[1] + y[2] / r ** 5 * y[0]]


def ref_recip(y, p):
    den = 1 + y[0] ** 2 + y[1] ** 2 / 2
    return [y[0] / den + y[1] * y[2] / den,
            sp.sin(y[2]) / den + 1 / den,
            (y[0] - y[2]) / den * y[1] + y[2] / (2 + y[0] * y[1])]


def ref_piecewise(y, p):
    d = y[0] - R(0.2)
    f0 = (d if p[0] > 0.2 else -d) * y[1] + (1 if p[1] > 0.0 else -1) * y[2] * y[0]
    if p[0] > 0.1 and p[1] <= 0.3:
        f1 = y[0] ** 2 * y[2]
    elif p[2] < -0.2 or p[0] >= 0.6:
        f1 = sp.sin(y[1]) * y[2]
    else:
        f1 = y[1] * y[2] + y[0]
    u = sp.exp(y[0] * y[1] / 2)
    f2 = u * y[0] if p[2] > 0.0 else u + y[1]
    return [f0, f1, f2]


def ref_guarded(y, p):
    f0 = sp.sqrt(y[0]) * y[1] if p[0] > 0.0 else y[1] * y[2]
    f1 = (sp.log(y[1] - R(0.5)) if p[1] > 0.5 else 0) + y[0] * y[2]
    f2 = y[0] / y[2] if (p[2] > 0.0 or p[2] < 0.0) else y[0]
    return [f0, f1, f2]


def ref_composed(y, p):
    r0 = (sp.sqrt(y[0]) * y[1] if p[0] > 0.0 else y[1] * y[2]) + y[3] * y[4]
    r1 = sp.sin(y[0] * y[2]) + y[1] * y[3] - y[4] / 2
    s = sp.exp(R(0.3) * r0 * r1)
    c = [r0 * r1 + s * sp.cos(r1), r1 ** 2 * r0 + s / (2 + r0 ** 2), sp.sin(r0 + r1 / 2) * s]
    w = y[0] * y[1] + y[2] ** 2 + sp.cos(y[3] * y[4])
    return [c[0] + w ** 2 * c[2], c[1] * w + c[2]]


def ref_bigbody(y, p):
    f0, f1 = 0, 0
    for k in range(1, vf_cases.BIG_TERMS + 1):
        c = R(0.125 * k)
        f0 += sp.sin(c * y[0] + y[1] * y[2]) * sp.exp(-c * y[1]) + sp.tanh(c * y[2] * y[0]) / (1 + c * y[1] ** 2)
        f1 += (1 + y[0] ** 2 + c * y[1] ** 2) ** sp.Rational(3, 2) * sp.cos(c * y[2]) + sp.atan(c * y[0] * y[1]) * sp.log(2 + c + y[2])
        f1 += sp.sqrt(y[0] - c + 1) * y[1] if p[0] > 0.125 * k - 1.0 else c * y[2]
    return [f0, f1]


REFS = {"trig": ref_trig, "hyper": ref_hyper, "inverse": ref_inverse, "powers": ref_powers, "recip": ref_recip,
        "piecewise": ref_piecewise, "guarded": ref_guarded, "composed": ref_composed, "bigbody": ref_bigbody}


# --------------------------------------------------------------------------- the points

def draw(name: str, rng, k: int):
    """One candidate for row k: y from the case's domain, lam ~ U(-1, 1).  The piecewise cases are interleaved by the row number, so
    that neighbouring applications (lanes of one wave) take different branches, with rows exactly on every threshold of `guarded`."""
    case = vf_cases.CASES[name]
    y = np.empty(case.N)
    for i, d in enumerate(case.domain):
        y[i] = rng.uniform(d[1], d[2]) * rng.choice([-1.0, 1.0]) if d[0] == "pm" else rng.uniform(d[0], d[1])
    lam = rng.uniform(-1.0, 1.0, case.n)
    side = lambda m: 1.0 if (k // m) % 2 == 0 else -1.0
    if name == "piecewise":
        y[2] = abs(y[2]) * side(1)
        y[1] = abs(y[1]) * side(2)
        lo, hi = [(-1.0, 0.1), (0.1, 0.6), (0.6, 1.0)][k % 3]
        y[0] = lo + (hi - lo) * rng.uniform(0.02, 0.98)
    elif name == "guarded":
        y[0] = 0.0 if k % 7 == 0 else abs(y[0]) * side(1)           # exactly on the thresholds (rows 0 and 91: on several at once)
        y[1] = 0.5 if k % 11 == 0 else 0.5 + abs(y[1] - 0.5) * side(2)
        y[2] = 0.0 if k % 13 == 0 else abs(y[2]) * side(4)
    elif name == "composed":
        y[0] = 0.0 if k % 9 == 0 else abs(y[0]) * side(1)
    elif name == "bigbody":
        y[0] = abs(y[0]) * side(1)
    return y, lam


# --------------------------------------------------------------------------- f, J, g, H of one statement

_compiled = {}


def compiled(exprs, ys, ls):
    """(50-digit evaluator, plain double evaluator) of [f, J, g, H lower] of the expressions, cached per branch pattern."""
    key = tuple(exprs)
    if key not in _compiled:
        n, N = len(exprs), len(ys)
        J = [sp.diff(e, v) for e in exprs for v in ys]
        S = sum(l * e for l, e in zip(ls, exprs))
        g = [sp.diff(S, v) for v in ys]
        H = [sp.diff(g[i], ys[j]) for i in range(N) for j in range(i + 1)]
        out = list(exprs) + J + g + H
        args = list(ys) + list(ls)
        _compiled[key] = (sp.lambdify(args, out, modules="mpmath", cse=True), sp.lambdify(args, out, modules="math", cse=True))
    return _compiled[key]


COND_LIMIT = 5.0e-14      # 16 x this stays below the host cap of 1e-12


def golden_case(name: str, seed: int):
    """The sampling domain of a case is its box WITHOUT the thin slabs where an entry of f, J, g or H cancels to below a thousandth
    of its array: there the plain double evaluation of the reference's own expression is off by ~1e-13 in the metric of the tests
    (one ulp of the array's largest entry against a floor a thousand times smaller), whatever code evaluates it.  A candidate whose
    own plain-double error exceeds COND_LIMIT is drawn again -- a property of the reference alone; nothing of the code under test
    enters.  Every row that is stored is tested."""
    case = vf_cases.CASES[name]
    N, n = case.N, case.n
    ys, ls = sp.symbols(f"y0:{N}", real=True), sp.symbols(f"l0:{n}", real=True)
    rng = np.random.default_rng(seed)
    nh = N * (N + 1) // 2
    cut = np.cumsum([n, n * N, N])
    Y, LAM = np.empty((NAPP, N)), np.empty((NAPP, n))
    ref = np.empty((NAPP, n + n * N + N + nh))
    dbl = np.empty_like(ref)
    redrawn = 0
    for a in range(NAPP):
        for attempt in range(200):
            y, lam = draw(name, rng, a)
            hi, lo = compiled(REFS[name](ys, [float(v) for v in y]), ys, ls)
            r = np.array([[float(v) for v in hi(*[mp.mpf(float(v)) for v in y], *[mp.mpf(float(v)) for v in lam])]])
            assert np.all(np.isfinite(r)), f"{name}: a reference entry is not finite at {y}"
            d = np.array([[float(v) for v in lo(*[float(v) for v in y], *[float(v) for v in lam])]])
            if max(vf_cases.entry_errors(dd, rr).max() for dd, rr in zip(np.split(d, cut, axis=1), np.split(r, cut, axis=1))) <= COND_LIMIT:
                break
            redrawn += 1
        else:
            raise RuntimeError(f"{name}: no well-conditioned point for row {a}")
        Y[a], LAM[a], ref[a], dbl[a] = y, lam, r[0], d[0]
    assert np.all(np.isfinite(ref)), f"{name}: a reference entry is not finite"
    out = {"Y": Y, "LAM": LAM}
    eref = []
    for key, r, d in zip(vf_cases.ARRAYS, np.split(ref, cut, axis=1), np.split(dbl, cut, axis=1)):
        out[key] = r.reshape(NAPP, n, N) if key == "J" else r
        eref.append(float(vf_cases.entry_errors(d, r).max()))
    out["E_ref"] = np.array(eref)
    out["redrawn"] = np.array(redrawn)
    return out


# --------------------------------------------------------------------------- csrc/asset_math.h

AM_SETS = ("quarter_pi", "ten", "thousand", "exact_range", "beyond", "half_pi_multiples", "edges")


def asset_math_reference(seed: int = 950):
    rng = np.random.default_rng(seed)
    sets = [rng.uniform(-math.pi / 4, math.pi / 4, 128), rng.uniform(-10.0, 10.0, 128), rng.uniform(-1.0e3, 1.0e3, 128),
            rng.uniform(-8.2e5, 8.2e5, 128),
            10.0 ** rng.uniform(6.0, 9.0, 128) * rng.choice([-1.0, 1.0], 128)]
    near = []
    for k in range(-40, 41):                                      # the doubles at and next to k pi/2
        x = float(mp.mpf(k) * mp.pi / 2)
        near += [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]
    sets.append(np.array(near))
    sets.append(np.array([0.0, -0.0, 1e-300, -1e-300, 5e-324, -5e-324]))
    x = np.concatenate(sets)
    which = np.concatenate([np.full(s.size, i, dtype=np.int8) for i, s in enumerate(sets)])
    out = {"am_x": x, "am_set": which, "am_set_names": np.array(AM_SETS)}
    for nm, fn in (("sin", mp.sin), ("cos", mp.cos), ("tan", mp.tan)):
        v = [fn(mp.mpf(float(t))) for t in x]
        hi = np.array([float(t) for t in v])
        out[f"am_{nm}_hi"] = np.copysign(hi, np.where(hi == 0.0, x if nm != "cos" else 1.0, hi))   # sin(-0.0) = -0.0
        out[f"am_{nm}_lo"] = np.array([float(t - mp.mpf(h)) for t, h in zip(v, hi)], dtype=np.float32)
    out["am_sec2"] = np.array([float(1 + mp.tan(mp.mpf(float(t))) ** 2) for t in x])
    assert all(np.all(np.isfinite(np.asarray(v, dtype=float))) for k, v in out.items() if k != "am_set_names")
    return out


def write_npz(path, data):
    """An .npz of ``data`` that depends on nothing but its contents: members in sorted order, one fixed time stamp (np.savez stamps
    the time of day on every member), deflate level 9.  ``path``: a file name or a binary file object."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(data):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(data[key]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)


def main():
    data = {}
    print(f"    {'case':<11} " + "    ".join(f"E_ref {k}" for k in vf_cases.ARRAYS))
    for i, name in enumerate(vf_cases.CASES):
        out = golden_case(name, 2000 + i)
        print(f"    {name:<11} " + "    ".join(f"{e:.1e}" for e in out["E_ref"]) + f"    ({int(out['redrawn'])} redrawn)", flush=True)
        for key, v in out.items():
            data[f"{name}_{key}"] = v
    data.update(asset_math_reference())
    path = os.path.join(HERE, "vf_ops.npz")
    write_npz(path, data)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
