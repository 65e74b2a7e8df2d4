"""Checker of the tables over two and three axes (``vf.InterpTable2D`` / ``vf.InterpTable3D``): the fixture
tests/golden/interp_nd/tables.npz (made by tests/golden/make_golden_interp_nd.py) and a restatement of the interpolant in numpy that
imports nothing from the package.

The fixture holds, per table, its axes, data and kind, 65 query points, and for every point the value, gradient and Hessian of the
interpolant as 50-digit numbers (stored as a float64 pair hi + lo) with a bound E per entry in units of u = 2^-53: the running
first-order rounding error of a float64 evaluation of that entry (the rules of tests/golden/make_golden_defect_entries.py).  An entry
with E = 0 has no rounded term and must be exactly the stored value.  ``check`` compares in long double, so the stored pair enters with
its full length.

The restatement (``Table``): nodal derivatives by five-point stencils -- the weights are the derivatives of the five Lagrange
polynomials at the abscissa, written as products and quotients of differences -- applied in the reference's order (2-D: dz/dy, dz/dx,
d2z/dxdy as the x-stencil of dz/dy; 3-D: fx, fy, fz, fxy = d/dy fx, fxz = d/dz fx, fyz = d/dz fy, fxyz = d/dz fxy); the element of each
axis by division where it is evenly spaced and by bisection elsewhere, clamped to [0, size - 2]; and the interpolant in its
TENSOR-PRODUCT form: the sum over the corners and quantities of the cell of quantity times the product of one 1-D Hermite weight (or
its first or second derivative) per axis.  The package evaluates the same polynomial nested, axis by axis: another order of the same
operations.  QUARTER: this float64 restatement is held to a quarter of every bound, by the generator and by
tests/test_interp_nd_cpu.py."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "interp_nd", "tables.npz")
U = 2.0 ** -53
QUARTER = 0.25
TABLES = ("c2", "l2", "c3", "l3")          # cubic / linear over two axes, cubic / linear over three
DIM = {"c2": 2, "l2": 2, "c3": 3, "l3": 3}
KIND = {"c2": "cubic", "l2": "linear", "c3": "cubic", "l3": "linear"}
# the axis of the data array that runs along argument a: Zs[iy, ix] and Fs[ix, iy, iz]
DATA_AXIS = {2: (1, 0), 3: (0, 1, 2)}


def five_point_weights(ts, i):
    """(start, w): sum_k w[k] v[start + k] is dv/dt at ts[i], exact for quartics."""
    n = ts.size
    if 2 <= i <= n - 3:
        start = i - 2
    elif i < n - 1 - i:
        start = 0
    else:
        start = n - 5
    x, j = ts[start:start + 5], i - start
    w = np.zeros(5, dtype=ts.dtype)
    for k in range(5):
        if k == j:
            for m in range(5):
                if m != j:
                    w[k] += 1 / (x[j] - x[m])
            continue
        num, den = ts.dtype.type(1), ts.dtype.type(1)
        for m in range(5):
            if m != k:
                den *= x[k] - x[m]
                if m != j:
                    num *= x[j] - x[m]
        w[k] = num / den
    return start, w


def diff_axis(A, ts, axis):
    A = np.moveaxis(A, axis, 0)
    out = np.empty_like(A)
    for i in range(ts.size):
        start, w = five_point_weights(ts, i)
        acc = w[0] * A[start]
        for k in range(1, 5):
            acc = acc + w[k] * A[start + k]
        out[i] = acc
    return np.moveaxis(out, 0, axis)


def is_even(ts):
    return bool(np.max(np.abs(ts - np.linspace(ts[0], ts[-1], ts.size))) <= abs(ts[-1] - ts[0]) * 1.0e-12)


def locate(ts, even, t):
    if even:
        e = int((t - ts[0]) / (ts[1] - ts[0]))
    else:
        e = int(np.searchsorted(ts, t, side="right")) - 1
    return max(min(e, ts.size - 2), 0)


def _weights(kind, x, step, order):
    if kind == "linear":
        return ((1 - x, x), (-1 / step, 1 / step), (0 * x, 0 * x))[order]
    x2, x3 = x * x, x * x * x
    if order == 0:
        return (2 * x3 - 3 * x2 + 1, -2 * x3 + 3 * x2, (x3 - 2 * x2 + x) * step, (x3 - x2) * step)
    if order == 1:
        return ((6 * x2 - 6 * x) / step, (-6 * x2 + 6 * x) / step, 3 * x2 - 4 * x + 1, 3 * x2 - 2 * x)
    return ((12 * x - 6) / (step * step), (-12 * x + 6) / (step * step), (6 * x - 4) / step, (6 * x - 2) / step)


class Table:
    """The restatement of one table.  axes: the abscissae in argument order; data as the constructors of the package take it."""

    def __init__(self, axes, data, kind, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.axes = [np.asarray(a, dtype=np.float64) for a in axes]
        self.even = [is_even(a) for a in self.axes]                     # (decided in float64, as the table itself decides)
        self.axes_w = [a.astype(self.dtype) for a in self.axes]
        self.dim, self.kind = len(axes), kind
        self.data_axis = DATA_AXIS[self.dim]
        f = np.asarray(data, dtype=np.float64).astype(self.dtype)
        d = lambda A, a: diff_axis(A, self.axes_w[a], self.data_axis[a])      # noqa: E731
        if kind == "linear":
            self.Q = [f]
        elif self.dim == 2:
            zy = d(f, 1)
            self.Q = [f, d(f, 0), zy, d(zy, 0)]
        else:
            fx, fy, fz = d(f, 0), d(f, 1), d(f, 2)
            fxy = d(fx, 1)
            self.Q = [f, fx, fy, fxy, fz, d(fx, 2), d(fy, 2), d(fxy, 2)]

    def elems(self, p):
        return [locate(a, ev, float(v)) for a, ev, v in zip(self.axes, self.even, p)]

    def _at(self, elems, W):
        dim, cubic = self.dim, self.kind == "cubic"
        total = self.dtype.type(0)
        for q in range(len(self.Q)):
            for c in range(1 << dim):
                idx = [0] * dim
                prod = self.dtype.type(1)
                for a in range(dim):
                    far = (c >> a) & 1
                    idx[self.data_axis[a]] = elems[a] + far
                    prod = prod * W[a][far + (2 if cubic and (q >> a) & 1 else 0)]
                total = total + self.Q[q][tuple(idx)] * prod
        return total

    def eval(self, p, deriv=2):
        """(value, gradient[dim], Hessian[dim, dim]) of the interpolant at the point p."""
        dim, T = self.dim, self.dtype.type
        elems = self.elems(p)
        xs, steps = [], []
        for a in range(dim):
            t0, t1 = self.axes_w[a][elems[a]], self.axes_w[a][elems[a] + 1]
            steps.append(t1 - t0)
            xs.append((T(p[a]) - t0) / steps[a])
        W = [[_weights(self.kind, xs[a], steps[a], o) for o in range(3)] for a in range(dim)]
        at = lambda orders: self._at(elems, [W[a][orders[a]] for a in range(dim)])      # noqa: E731
        v = at([0] * dim)
        g = np.zeros(dim, dtype=self.dtype)
        H = np.zeros((dim, dim), dtype=self.dtype)
        if deriv > 0:
            for i in range(dim):
                g[i] = at([int(a == i) for a in range(dim)])
        if deriv > 1:
            for i in range(dim):
                for j in range(i + 1):
                    if i == j and self.kind == "linear":
                        continue
                    H[i, j] = H[j, i] = at([int(a == i) + int(a == j) for a in range(dim)])
        return v, g, H


# --------------------------------------------------------------------------- the fixture
_CACHE = {}


def load():
    if not _CACHE:
        with np.load(PATH) as z:
            _CACHE.update({k: z[k] for k in z.files})
        for a in _CACHE.values():
            a.setflags(write=False)
    return _CACHE


def axes_of(name, fx=None):
    fx = load() if fx is None else fx
    return [fx[f"{name}_{l}s"] for l in "xyz"[:DIM[name]]]


def restated(name, dtype=np.float64, fx=None):
    fx = load() if fx is None else fx
    return Table(axes_of(name, fx), fx[f"{name}_data"], KIND[name], dtype)


def entries(name, fx=None):
    """{"v": (hi, lo, E), "g": ..., "H": ...} of a table: arrays over its points."""
    fx = load() if fx is None else fx
    return {k: (fx[f"{name}_{k}"], fx[f"{name}_{k}lo"], fx[f"{name}_{k}E"]) for k in ("v", "g", "H")}


def check(got, hi, lo, E, what="", fraction=1.0, extra=0.0):
    """|got - (hi + lo)| <= fraction * u * E + extra, entry by entry (E = 0 and extra = 0: exactly); returns the largest used share
    of the bound.  `extra`: an absolute allowance per entry, for roundings the caller adds on top of the fixture's entry."""
    got = np.asarray(got, dtype=np.float64).reshape(np.shape(hi))
    err = np.abs((got.astype(np.longdouble) - np.asarray(hi, dtype=np.longdouble)) - np.asarray(lo, dtype=np.longdouble)).astype(np.float64)
    bound = fraction * U * np.asarray(E, dtype=np.float64) + extra
    bad = err > bound
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))) if err.size else 0.0
    if np.any(bad):
        k = np.unravel_index(int(np.argmax(np.where(bad, err - bound, -1.0))), err.shape)
        raise AssertionError(f"{what}: entry {k}: |got - ref| = {err[k]:.3e} > bound {np.broadcast_to(bound, err.shape)[k]:.3e} "
                             f"(got {got[k]!r}, ref {np.asarray(hi)[k]!r}); {int(bad.sum())} of {err.size} entries miss")
    return worst


def restatement_blocks(name, fx=None):
    """The float64 restatement at every point of a fixture table: (v[m], g[m, dim], H[m, dim, dim])."""
    fx = load() if fx is None else fx
    tab, P = restated(name, fx=fx), fx[f"{name}_P"]
    out = [tab.eval(p) for p in P]
    return (np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.float64),
            np.array([o[2] for o in out], dtype=np.float64))


def check_quarter(fx=None):
    """The QUARTER rule on every table of the fixture; returns {table: largest share of the full bound the restatement uses}."""
    used = {}
    for name in TABLES:
        v, g, H = restatement_blocks(name, fx)
        e = entries(name, fx)
        used[name] = max(check(v, *e["v"], f"{name} value (restatement)", QUARTER), check(g, *e["g"], f"{name} gradient (restatement)", QUARTER),
                         check(H, *e["H"], f"{name} Hessian (restatement)", QUARTER)) * QUARTER
    return used
