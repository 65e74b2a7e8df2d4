"""Generate tests/golden/interp_nd/tables.npz: four small tables (bicubic and bilinear on 6 x 7, tricubic and trilinear on
5 x 6 x 7; per grid one evenly spaced axis, the others uneven), 65 query points each, and at every point the value, gradient and
Hessian of the table's interpolant as 50-digit numbers, each with a running error bound of its own (run once; commit the .npz).

What is computed (mpmath, 50 digits): the data of a smooth non-polynomial function with O(1) values, rounded to float64 -- from there
on the float64 numbers ARE the table; the nodal derivatives of the cubic kind by five-point stencils whose weights are the
derivatives of the five Lagrange polynomials at the abscissa, applied in the reference's order (InterpTable2D.h:114-199: dz/dy, dz/dx,
d2z/dxdy as the x-stencil of dz/dy; InterpTable3D.h:220-228: fx, fy, fz, fxy = d/dy fx, fxz = d/dz fx, fyz = d/dz fy,
fxyz = d/dz fxy); the element of each axis by the reference's rule in float64 (division on the evenly spaced axis, bisection
elsewhere, clamped); and the tensor-product Hermite interpolant of that cell (bilinear / trilinear for the linear kind) in its
nested form, differentiated exactly by second-order forward AD.

Bounds: everything runs over the scalars with a running error of make_golden_defect_entries.py (``S`` for the weights and the nodal
derivatives, ``DE`` for the interpolant; the rules are in that file's docstring): abscissae, data and query points are exact, every
difference, product, quotient and sum of the float64 evaluation adds its rounding.  u E then bounds, to first order, the rounding
error of a float64 evaluation of that entry; an entry with E = 0 (the pure second derivatives of a linear table) has no rounded term.
Nothing of the package enters.  Before writing, the float64 restatement of tests/interp_nd_checker.py -- the tensor-product form,
another order of the operations -- is held to a QUARTER of every bound.

Query points: cell interiors; exactly on grid lines and on grid nodes (the first and the last node among them); the first and last
cells; past both ends of every axis, singly and together; one pair in different cells that differ in the element of one axis only;
the rest drawn over the grid widened by a fifth either side.  Point 0 is an interior point; the others are shuffled, so neighbouring
applications of a device test sit in different cells and in and out of range.

Usage:  python tests/golden/make_golden_interp_nd.py
"""
from __future__ import annotations

import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import interp_nd_checker as ck  # noqa: E402
from make_golden_defect_entries import DE, S  # noqa: E402

mp.mp.dps = 50
NPTS = 65

AXES2 = [np.array([-1.0 + 0.5 * k for k in range(6)]), np.array([0.0, 0.3, 0.5, 1.0, 1.2, 1.7, 2.0])]
AXES3 = [np.array([-1.0, -0.4, 0.1, 0.45, 1.0]), np.array([0.25 * k for k in range(6)]), np.array([-0.5, -0.2, 0.0, 0.35, 0.6, 1.1, 1.5])]


def data2(x, y):
    return mp.sin(mp.mpf("1.3") * x + mp.mpf("0.4")) * mp.exp(-y / 2) + mp.mpf("0.3") * mp.cos(x * y)


def data3(x, y, z):
    return mp.sin(mp.mpf("1.1") * x + mp.mpf("0.3")) * mp.cos(mp.mpf("0.7") * y) * mp.exp(-mp.mpf("0.4") * z) + mp.mpf("0.2") * x * z / (1 + y * y)


def sample(axes, fn):
    """The data as the constructors take it: Zs[iy, ix] / Fs[ix, iy, iz], rounded to float64."""
    if len(axes) == 2:
        return np.array([[float(fn(mp.mpf(float(x)), mp.mpf(float(y)))) for x in axes[0]] for y in axes[1]])
    return np.array([[[float(fn(mp.mpf(float(x)), mp.mpf(float(y)), mp.mpf(float(z)))) for z in axes[2]] for y in axes[1]] for x in axes[0]])


# --------------------------------------------------------------------------- nodal derivatives over S
def diff_exact(a: float, b: float) -> S:
    """a - b of two float64 numbers as float64 forms it: one rounding, none where the difference is a float64 number"""
    r = mp.mpf(float(a)) - mp.mpf(float(b))
    return S(r, 0.0 if mp.mpf(float(r)) == r else abs(float(r)))


def weights(ts, i):
    n = ts.size
    start = i - 2 if 2 <= i <= n - 3 else (0 if i < n - 1 - i else n - 5)
    x, j = ts[start:start + 5], i - start
    w = [None] * 5
    for k in range(5):
        if k == j:
            acc = None
            for m in range(5):
                if m != j:
                    t = diff_exact(x[j], x[m]).recip()
                    acc = t if acc is None else acc + t
            w[k] = acc
            continue
        num, den = None, None
        for m in range(5):
            if m != k:
                d = diff_exact(x[k], x[m])
                den = d if den is None else den * d
                if m != j:
                    e = diff_exact(x[j], x[m])
                    num = e if num is None else num * e
        w[k] = num * den.recip()
    return start, w


def diff_axis(A, ts, axis):
    """A: object array of S"""
    A = np.moveaxis(A, axis, 0)
    out = np.empty_like(A)
    for i in range(ts.size):
        start, w = weights(ts, i)
        for idx in np.ndindex(*A.shape[1:]):
            acc = w[0] * A[(start,) + idx]
            for k in range(1, 5):
                acc = acc + w[k] * A[(start + k,) + idx]
            out[(i,) + idx] = acc
    return np.moveaxis(out, 0, axis)


def quantities(axes, data, kind):
    dim = len(axes)
    da = ck.DATA_AXIS[dim]
    f = np.empty(data.shape, dtype=object)
    for idx in np.ndindex(*data.shape):
        f[idx] = S(mp.mpf(float(data[idx])), 0.0)
    d = lambda A, a: diff_axis(A, axes[a], da[a])      # noqa: E731
    if kind == "linear":
        return [f]
    if dim == 2:
        zy = d(f, 1)
        return [f, d(f, 0), zy, d(zy, 0)]
    fx, fy, fz = d(f, 0), d(f, 1), d(f, 2)
    fxy = d(fx, 1)
    return [f, fx, fy, fxy, fz, d(fx, 2), d(fy, 2), d(fxy, 2)]


# --------------------------------------------------------------------------- the interpolant over DE
def const(s: S, n: int) -> DE:
    c = DE.const(s.v, n)
    c.ev = s.e
    return c


def interpolant(axes, Q, kind, p):
    dim, cubic = len(axes), kind == "cubic"
    da = ck.DATA_AXIS[dim]
    elems = [ck.locate(a, ck.is_even(a), float(v)) for a, v in zip(axes, p)]
    W = []
    for a in range(dim):
        t0, t1 = axes[a][elems[a]], axes[a][elems[a] + 1]
        step = const(diff_exact(t1, t0), dim)
        x = (DE.var(float(p[a]), a, dim) - float(t0)) / step
        if cubic:
            x2 = x * x
            x3 = x2 * x
            W.append((2.0 * x3 - 3.0 * x2 + 1.0, 3.0 * x2 - 2.0 * x3, (x3 - 2.0 * x2 + x) * step, (x3 - x2) * step))
        else:
            W.append((1.0 - x, x))
    V = {}
    for q in range(len(Q)):
        V[q] = {}
        for c in range(1 << dim):
            idx = [0] * dim
            for a in range(dim):
                idx[da[a]] = elems[a] + ((c >> a) & 1)
            V[q][c] = const(Q[q][tuple(idx)], dim)
    for a in range(dim):
        w, rest = W[a], dim - a - 1
        nV = {}
        for q in range(1 << rest) if cubic else (0,):
            for c in range(1 << rest):
                qq = (q << 1) if cubic else 0
                r = V[qq][c << 1] * w[0] + V[qq][(c << 1) | 1] * w[1]
                if cubic:
                    r = r + V[qq | 1][c << 1] * w[2] + V[qq | 1][(c << 1) | 1] * w[3]
                nV.setdefault(q, {})[c] = r
        V = nV
    return V[0][0]


# --------------------------------------------------------------------------- query points
def points(axes, seed):
    rng = np.random.default_rng(seed)
    dim = len(axes)
    mid = [0.5 * (a[2] + a[3]) + 0.01 for a in axes]
    P = []
    for a in range(dim):
        ax = axes[a]
        for v in (ax[2], ax[0], ax[-1], ax[-2]):                                   # on a grid line of this axis, the others inside
            p = list(mid)
            p[a] = v
            P.append(p)
        for v in (ax[0] - 0.37, ax[-1] + 0.61, 0.5 * (ax[0] + ax[1]), 0.5 * (ax[-2] + ax[-1])):   # past either end; first and last cell
            p = list(mid)
            p[a] = v
            P.append(p)
    P += [[a[1] for a in axes], [a[0] for a in axes], [a[-1] for a in axes], [a[3] for a in axes]]     # on grid nodes
    P += [[a[0] - 0.3 for a in axes], [a[-1] + 0.45 for a in axes]]                                      # past every end at once
    pair = [0.25 * a[2] + 0.75 * a[3] for a in axes]                                                     # one pair: the x element only
    twin = list(pair)
    twin[0] = 0.25 * axes[0][3] + 0.75 * axes[0][4]
    P += [pair, twin]
    while len(P) < NPTS - 1:
        P.append([rng.uniform(a[0] - 0.2 * (a[-1] - a[0]), a[-1] + 0.2 * (a[-1] - a[0])) for a in axes])
    P = np.array(P, dtype=np.float64)[rng.permutation(len(P))]
    first = np.array([[0.3 * a[1] + 0.7 * a[2] for a in axes]])
    return np.concatenate([first, P])


def main():
    out = {}
    for name in ck.TABLES:
        dim, kind = ck.DIM[name], ck.KIND[name]
        axes = AXES2 if dim == 2 else AXES3
        data = sample(axes, data2 if dim == 2 else data3)
        Q = quantities(axes, data, kind)
        P = points(axes, 950 + dim)
        m = P.shape[0]
        vals = {k: np.zeros(s) for k, s in (("v", m), ("vlo", m), ("vE", m), ("g", (m, dim)), ("glo", (m, dim)), ("gE", (m, dim)),
                                            ("H", (m, dim, dim)), ("Hlo", (m, dim, dim)), ("HE", (m, dim, dim)))}

        def put(key, idx, val, e):
            hi = float(val)
            vals[key][idx] = hi
            vals[key + "lo"][idx] = float(val - mp.mpf(hi))
            vals[key + "E"][idx] = float(e) * (1.0 + 2.0 ** -40) if e else 0.0       # (the bound's own float64 roundings: upward)
        for k, p in enumerate(P):
            r = interpolant(axes, Q, kind, p)
            put("v", k, r.v, r.ev)
            for i in range(dim):
                put("g", (k, i), r.g[i], r.eg[i])
                for j in range(dim):
                    put("H", (k, i, j), r.h[i][j], r.eh[i][j])
        for l, a in zip("xyz", axes):
            out[f"{name}_{l}s"] = a
        out[f"{name}_data"], out[f"{name}_P"] = data, P
        for k, v in vals.items():
            out[f"{name}_{k}"] = v
        print(f"{name}: {m} points, max E: value {vals['vE'].max():.3g}, gradient {vals['gE'].max():.3g}, Hessian {vals['HE'].max():.3g}", flush=True)
    used = ck.check_quarter(out)
    print("float64 restatement, largest share of the full bound:", {k: round(v, 4) for k, v in used.items()})
    os.makedirs(os.path.dirname(ck.PATH), exist_ok=True)
    np.savez_compressed(ck.PATH, **out)
    print("wrote", ck.PATH, os.path.getsize(ck.PATH), "bytes")


if __name__ == "__main__":
    main()
