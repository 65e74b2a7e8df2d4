"""The tables, functions and ODEs of the tests of ``vf.InterpTable2D`` / ``vf.InterpTable3D`` (tests/test_interp_nd_cpu.py,
tests/test_gpu_interp_nd.py, and the pre-build of __graft_entry__.build()).

Fixture tables: the four tables of tests/golden/interp_nd/tables.npz as ``vf`` objects (``table``) -- tests/interp_nd_checker.py
holds their restatement, written without the package.

Polynomial tables: data sampled from a polynomial the table reproduces exactly -- degree <= 3 per variable for the cubic kind (the
five-point stencils are exact for quartics, so the nodal derivatives are those of the polynomial and the cell's Hermite polynomial
is the polynomial itself), degree <= 1 per variable for the linear kind -- everywhere, extrapolation included.  A function or ODE on
such a table and its twin written directly in the DSL are two float64 forms of one function."""
from __future__ import annotations

import functools

import numpy as np

import interp_nd_checker as ck

# ---- polynomials: C[i, j(, k)] x^i y^j (z^k), O(1) coefficients
POLY = {
    "cubic2": np.array([[0.4, -0.2, 0.1, -0.04], [0.3, 0.25, 0.0, 0.02], [-0.15, 0.06, 0.03, 0.0], [0.05, 0.0, -0.02, 0.01]]),
    "linear2": np.array([[0.3, -0.4], [0.5, 0.2]]),
    "cubic3": np.array([[[0.3, 0.1, 0.0, -0.02], [-0.2, 0.05, 0.03, 0.0], [0.1, 0.0, 0.0, 0.01], [-0.03, 0.02, 0.0, 0.0]],
                        [[0.25, -0.1, 0.04, 0.0], [0.15, 0.2, 0.0, 0.0], [0.0, -0.05, 0.0, 0.0], [0.02, 0.0, 0.0, 0.005]],
                        [[-0.1, 0.0, 0.03, 0.0], [0.05, 0.0, 0.0, 0.0], [0.0, 0.02, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]],
                        [[0.04, 0.0, 0.0, 0.0], [0.0, -0.01, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.002]]]),
    "linear3": np.array([[[0.2, 0.15], [-0.25, -0.2]], [[0.3, 0.0], [0.1, 0.05]]]),
}
# the grids: per polynomial, the axes in argument order (some evenly spaced, some not)
_UNEVEN7 = np.array([-1.6, -1.1, -0.4, 0.0, 0.5, 1.2, 1.6])
_EVEN6 = np.linspace(-1.5, 1.5, 6)
_TIME6 = np.array([-0.5, 0.0, 0.4, 1.0, 1.7, 2.5])
GRID = {"cubic2": (_UNEVEN7, _EVEN6), "linear2": (_EVEN6, _UNEVEN7), "cubic3": (_EVEN6, _UNEVEN7, _TIME6), "linear3": (_UNEVEN7, _EVEN6, _TIME6)}


def poly_np(name, p, orders=None):
    """The polynomial `name`, or its partial derivative of the given order per variable, at the point p (numpy)."""
    C = POLY[name]
    orders = [0] * C.ndim if orders is None else orders
    out = C
    for a in range(C.ndim):
        # contract the leading axis with the powers of p[a] (differentiated `orders[a]` times)
        k = np.arange(out.shape[0], dtype=float)
        w = np.ones_like(k)
        for o in range(orders[a]):
            w = w * (k - o)
        pw = np.where(k - orders[a] >= 0, float(p[a]) ** np.maximum(k - orders[a], 0), 0.0) * w
        out = np.tensordot(pw, out, axes=(0, 0))
    return float(out)


def poly_blocks(name, p):
    """(value, gradient, Hessian) of the polynomial at p."""
    d = POLY[name].ndim
    g = np.array([poly_np(name, p, [int(a == i) for a in range(d)]) for i in range(d)])
    H = np.array([[poly_np(name, p, [int(a == i) + int(a == j) for a in range(d)]) for j in range(d)] for i in range(d)])
    return poly_np(name, p), g, H


def poly_vf(name, args):
    """The polynomial over scalar ``vf`` functions, term by term."""
    C = POLY[name]
    total = None
    for idx in np.ndindex(*C.shape):
        if C[idx] == 0.0:
            continue
        term = None
        for a, k in enumerate(idx):
            for _ in range(k):
                term = args[a] if term is None else term * args[a]
        term = float(C[idx]) if term is None else term * float(C[idx])
        total = term if total is None else total + term
    return total


def poly_data(name):
    """The polynomial on its grid, as the constructors take the data: Zs[iy, ix] / Fs[ix, iy, iz]."""
    axes = GRID[name]
    if len(axes) == 2:
        return np.array([[poly_np(name, (x, y)) for x in axes[0]] for y in axes[1]])
    return np.array([[[poly_np(name, (x, y, z)) for z in axes[2]] for y in axes[1]] for x in axes[0]])


@functools.lru_cache(maxsize=None)
def poly_table(name):
    from asset_asrl_amd import vf
    kind = "cubic" if name.startswith("cubic") else "linear"
    cls = vf.InterpTable2D if len(GRID[name]) == 2 else vf.InterpTable3D
    tab = cls(*GRID[name], poly_data(name), kind=kind)
    tab.WarnOutOfBounds = False
    return tab


def poly_restated(name, dtype=np.float64):
    """The checker's restatement of a polynomial table (numpy callbacks of the propagation tests)."""
    return ck.Table(GRID[name], poly_data(name), "cubic" if name.startswith("cubic") else "linear", dtype)


@functools.lru_cache(maxsize=None)
def table(name):
    """A table of the fixture ('c2', 'l2', 'c3', 'l3') as a ``vf`` object."""
    from asset_asrl_amd import vf
    fx = ck.load()
    cls = vf.InterpTable2D if ck.DIM[name] == 2 else vf.InterpTable3D
    tab = cls(*ck.axes_of(name), fx[f"{name}_data"], kind=ck.KIND[name])
    tab.WarnOutOfBounds = False
    return tab


# ---- plain functions on the fixture tables
MIX_TERMS = (0.5, -0.25)          # out0 = c2(y0, y1) + 0.5 y4,  out1 = c3(y2, y3, y4) - 0.25 y0


def function(name):
    """'c2' ... 'l3': the table over its own arguments; 'mixed': a 2-D and a 3-D table and an ordinary term, 5 inputs, 2 outputs."""
    from asset_asrl_amd import vf
    if name == "mixed":
        a = vf.Arguments(5)
        return vf.stack([table("c2")(a[0], a[1]) + MIX_TERMS[0] * a[4], table("c3")(a[2], a[3], a[4]) + MIX_TERMS[1] * a[0]])
    return table(name).vf()


def device_name(name):
    return "interpnd_" + name


FUNCTIONS = ck.TABLES + ("mixed",)

# ---- the ODE (2, 1, 0) on a 2-D cubic table over (state, control) and a 3-D linear table over (state, state, time); its twin
ODE_MODES = (("LGL3", False), ("LGL7", True), ("Trapezoidal", False))


@functools.lru_cache(maxsize=None)
def make_ode(twin: bool = False):
    from asset_asrl_amd import vf
    from asset_asrl_amd.ode import ODEArguments, ODEBase

    class TableOde(ODEBase):
        def __init__(self):
            a = ODEArguments(2, 1, 0)
            x0, x1 = a.XVec().tolist()
            t, u = a.TVar(), a.UVar(0)
            if twin:
                c2, l3 = poly_vf("cubic2", [x0, u]), poly_vf("linear3", [x0, x1, t])
            else:
                c2, l3 = poly_table("cubic2")(x0, u), poly_table("linear3")(x0, x1, t)
            super().__init__(vf.stack([x1 + 0.3 * c2, -1.0 * x0 + 0.5 * l3 + u]), 2, 1, 0, name="interp_nd_poly" if twin else "interp_nd_table")

    return TableOde()


def ode_callbacks(dtype=np.float64):
    """(f, fj) of the table ODE on the row [x0, x1, t, u], from the checker's restatement of its two tables."""
    c2, l3 = poly_restated("cubic2", dtype), poly_restated("linear3", dtype)

    def fj(y):
        y = np.asarray(y)
        v2, g2, _ = c2.eval((y[0], y[3]), 1)
        v3, g3, _ = l3.eval((y[0], y[1], y[2]), 1)
        f = np.array([y[1] + 0.3 * v2, -y[0] + 0.5 * v3 + y[3]], dtype=y.dtype)
        J = np.zeros((2, 4), dtype=y.dtype)
        J[0, 0], J[0, 1], J[0, 3] = 0.3 * g2[0], 1.0, 0.3 * g2[1]
        J[1, 0], J[1, 1], J[1, 2], J[1, 3] = -1.0 + 0.5 * g3[0], 0.5 * g3[1], 0.5 * g3[2], 1.0
        return f, J
    return (lambda y: fj(y)[0]), fj


# ---- an event on the oscillator of event_cases, a law on the double integrator of controller_cases
EVENT_LEVEL = 0.45
LAW_VARLOCS = [0, 2]              # u = cubic2(x0, t) on the row [x0, x1, t, u, p0]


def event_function():
    """g = cubic2(x0, x1) - EVENT_LEVEL over the oscillator's input row [x0, x1, t]."""
    from asset_asrl_amd import vf
    a = vf.Arguments(3)
    return poly_table("cubic2")(a[0], a[1]) - EVENT_LEVEL


def control_law():
    from asset_asrl_amd import vf
    a = vf.Arguments(2)
    return poly_table("cubic2")(a[0], a[1]), list(LAW_VARLOCS)


def prebuild(jit):
    import controller_cases
    import event_cases
    for name in FUNCTIONS:
        jit.ensure_function(function(name), device_name(name))
    for twin in (False, True):
        for mode, blocked in ODE_MODES:                       # (the LGL3 module holds the ODE's propagation kernels)
            jit.ensure_kernel(make_ode(twin), mode, blocked)
    jit.ensure_event_module(event_cases.make_ode("oscillator"), [event_function()])
    jit.ensure_controller_module(controller_cases.make_ode("pd"), *control_law())
