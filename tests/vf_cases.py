"""The case table of the DSL operation tests (tests/test_vf_ops_cpu.py, tests/test_gpu_vf_ops.py): every operation of the ``vf``
expression DSL in a handful of small functions, each with several outputs and products of distinct inputs, so that the Jacobian mixes
rows in ``g = J^T lam`` and the adjoint Hessian has off-diagonal entries.

    CASES[name] = Case(build, N, n, domain)

``build(a)`` takes ``vf.Arguments(N)`` and returns the function R^N -> R^n.  ``domain`` is one entry per input: ``(lo, hi)``, uniform,
or ``("pm", lo, hi)``, uniform in magnitude with either sign (points in all quadrants, away from zero).  The committed fixture
tests/golden/vf_ops.npz holds, for 193 points of every case, f, J, g and H at 50 digits from a SECOND statement of the same functions
over sympy (tests/golden/make_golden_vf.py) -- that generator reads the sizes, the domains and the metric below from this file and
nothing of ``vf``; the points it adds to the domain (thresholds of the piecewise cases) are its own.

The comparison (``entry_errors``): per entry of an array at one point, ``|got - ref| / max(|ref_ij|, 1e-3 max|ref|)`` with the maximum
over that array at that point -- a wrong small entry cannot hide behind a large one.  The tolerance of a case and an array is
``16 x E_ref`` (floored at 1e-14), E_ref being the error of the reference's OWN expression in plain double against its 50-digit value in
the same metric: generated code is the same real function in another order (shared sub-expressions, one more rounding per lowered
quotient, fma contraction on the device, 2-3 ulp trigonometric functions), so it may lose a small multiple of what the plain
evaluation loses and no more.  CAP_HOST / CAP_DEVICE are conditions on the sampling domains, not measurements: a case whose tolerance
would exceed them is badly conditioned and gets another domain.
"""
import contextlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "build N n domain")

NAPP = 193                     # no multiple of 64: the last wave of the function kernels is partial
MARGIN, TOL_FLOOR = 16.0, 1.0e-14
CAP_HOST, CAP_DEVICE = 1.0e-12, 1.0e-11
ARRAYS = ("f", "J", "g", "H")
BIG_TERMS = 7                  # terms of `bigbody`: enough for more than codegen.SPLIT_OPS operations


def entry_errors(got, ref):
    """Per-entry error of `got` against `ref`, both [napp, ...]: |got - ref| / max(|ref_ij|, 1e-3 max|ref| of the array at that point).
    Where the whole array is zero at a point the entries must be zero: the error is 0 where they are and inf elsewhere."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    flat_g, flat_r = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    top = np.abs(flat_r).max(axis=1, keepdims=True)
    den = np.maximum(np.abs(flat_r), 1.0e-3 * top)
    diff = np.abs(flat_g - flat_r)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(den > 0.0, diff / np.where(den > 0.0, den, 1.0), np.where(diff == 0.0, 0.0, np.inf))
    return err.reshape(got.shape)


def tolerance(e_ref: float, cap: float) -> float:
    tol = max(MARGIN * float(e_ref), TOL_FLOOR)
    assert tol <= cap, f"16 x E_ref = {tol:.2e} is above the cap {cap:.0e}: the sampling domain is badly conditioned"
    return tol


# --------------------------------------------------------------------------- the functions

def _trig(a):
    from asset_asrl_amd import vf
    y0, y1, y2 = a.tolist()
    w = 0.7 * y0 + y1 * y2
    return vf.stack([vf.sin(w) * vf.cos(w) + y2,                                  # a sin / cos pair on one argument: one sincos on the device
                     vf.sin(y0 * y1 - 0.3 * y2) * y2,                             # a lone sin in the value body
                     vf.tan(0.5 * y0 + 0.25 * y1 * y2) + vf.cos(y1 + y2 * y2) * y0])


def _hyper(a):
    from asset_asrl_amd import vf
    y0, y1, y2 = a.tolist()
    return vf.stack([vf.exp(0.5 * y0 * y1) * vf.log(1.5 + y2 + y0 * y0) + vf.tanh(y1 - 0.4 * y2),
                     vf.sinh(y0 + 0.3 * y1 * y2) * vf.cosh(0.6 * y1 - y2) + vf.tanh(y0 * y2) * vf.log(2.0 + y1)])


def _inverse(a):
    from asset_asrl_amd import vf
    y0, y1, y2, y3 = a.tolist()
    return vf.stack([vf.arcsin(0.9 * y0 * y1) * y2 + vf.arccos(0.45 * (y0 + y1)),
                     vf.arctan(y0 * y2 + 2.0 * y1) + vf.arctan2(y2, y3) * y0])


def _powers(a):
    y0, y1, y2 = a.tolist()
    return _stack([y0 ** 3 * y1 + y1 ** 5 - y2 ** 7 * y0,
                   y0 ** -2 * y2 + (y1 * y2) ** -3 + (y0 + y1) ** 1.5,
                   (y0 * y2) ** -0.5 * y1 + (y1 + 0.5 * y2) ** 2.5,
                   a.cubed_norm() * y0 + a.inverse_norm() * y1 + a.normalized_power3()[0] * y1 + a.normalized_power5()[2] * y0])


def _recip(a):
    from asset_asrl_amd import vf
    y0, y1, y2 = a.tolist()
    den = 1.0 + y0 * y0 + 0.5 * y1 * y1                                           # divides five times: lower_reciprocals rewrites them
    return vf.stack([y0 / den + y1 * y2 / den,
                     vf.sin(y2) / den + 1.0 / den,
                     (y0 - y2) / den * y1 + y2 / (2.0 + y0 * y1)])                # ... and a denominator that divides once and stays


def _piecewise(a):
    from asset_asrl_amd import vf
    y0, y1, y2 = a.tolist()
    u = vf.exp(0.5 * y0 * y1)                                                     # shared by the two branches of the last select
    return vf.stack([vf.abs(y0 - 0.2) * y1 + vf.sign(y1) * y2 * y0,
                     vf.ifelse((y0 > 0.1) & (y1 <= 0.3), y0 * y0 * y2,
                               vf.ifelse((y2 < -0.2) | (y0 >= 0.6), vf.sin(y1) * y2, y1 * y2 + y0)),
                     vf.ifelse(y2 > 0.0, u * y0, u + y1)])


def _guarded(a):
    from asset_asrl_amd import vf
    y0, y1, y2 = a.tolist()
    return vf.stack([vf.ifelse(y0 > 0.0, vf.sqrt(y0) * y1, y1 * y2),
                     vf.ifelse(y1 > 0.5, vf.log(y1 - 0.5), 0.0) + y0 * y2,
                     vf.ifelse((y2 > 0.0) | (y2 < 0.0), y0 / y2, y0)])


def _composed(a):
    from asset_asrl_amd import vf
    y0, y1, y2, y3, y4 = a.tolist()
    inner = vf.stack([vf.ifelse(y0 > 0.0, vf.sqrt(y0) * y1, y1 * y2) + y3 * y4,   # R^5 -> R^2, a guarded sqrt inside
                      vf.sin(y0 * y2) + y1 * y3 - 0.5 * y4])
    R = vf.Arguments(2)
    r0, r1 = R.tolist()
    s = vf.exp(0.3 * r0 * r1)
    outer = vf.stack([r0 * r1 + s * vf.cos(r1), r1 * r1 * r0 + s / (2.0 + r0 * r0), vf.sin(r0 + 0.5 * r1) * s])
    c = outer(inner)                                                              # cuts at the inner function's outputs
    w = (y0 * y1 + y2 * y2 + vf.cos(y3 * y4)).cut()                               # ... and an explicit one
    return vf.stack([c[0] + w * w * c[2], c[1] * w + c[2]])


def _bigbody(a):
    from asset_asrl_amd import vf
    y0, y1, y2 = a.tolist()
    f0, f1 = 0.0, 0.0
    for k in range(1, BIG_TERMS + 1):
        c = 0.125 * k
        f0 = f0 + vf.sin(c * y0 + y1 * y2) * vf.exp(-c * y1) + vf.tanh(c * y2 * y0) / (1.0 + c * y1 * y1)
        f1 = f1 + (1.0 + y0 * y0 + c * y1 * y1) ** 1.5 * vf.cos(c * y2) + vf.arctan(c * y0 * y1) * vf.log(2.0 + c + y2) \
            + vf.ifelse(y0 > c - 1.0, vf.sqrt(y0 - c + 1.0) * y1, c * y2)
    return vf.stack([f0, f1])


def _stack(fs):
    from asset_asrl_amd import vf
    return vf.stack(fs)


CASES = {
    "trig": Case(_trig, 3, 3, [(-1.2, 1.2)] * 3),
    "hyper": Case(_hyper, 3, 2, [(-1.0, 1.0)] * 3),
    "inverse": Case(_inverse, 4, 2, [(-1.0, 1.0), (-1.0, 1.0), ("pm", 0.3, 1.5), ("pm", 0.3, 1.5)]),
    "powers": Case(_powers, 3, 4, [(0.5, 1.5)] * 3),
    "recip": Case(_recip, 3, 3, [(-1.0, 1.0)] * 3),
    "piecewise": Case(_piecewise, 3, 3, [(-1.0, 1.0)] * 3),
    "guarded": Case(_guarded, 3, 3, [(-1.0, 1.0), (-0.5, 1.5), ("pm", 0.05, 1.0)]),
    "composed": Case(_composed, 5, 2, [(-1.0, 1.0)] * 5),
    "bigbody": Case(_bigbody, 3, 2, [(-1.0, 1.0)] * 3),
}


def build(name: str):
    """The function of a case over fresh arguments."""
    from asset_asrl_amd import vf
    return CASES[name].build(vf.Arguments(CASES[name].N))


@contextlib.contextmanager
def flat_chain_rule():
    """Inside: compositions are differentiated as ONE flattened expression (codegen.BLOCK_CHAIN_RULE off)."""
    from asset_asrl_amd.vf import codegen
    old = codegen.BLOCK_CHAIN_RULE
    codegen.BLOCK_CHAIN_RULE = False
    try:
        yield
    finally:
        codegen.BLOCK_CHAIN_RULE = old


def build_flat(name: str):
    """(function, derivatives) of a case in the flattened form."""
    from asset_asrl_amd.vf import codegen
    with flat_chain_rule():
        func = build(name)
        return func, codegen.differentiate_function(name + "_flat", func)


DEVICE_FORMS = [(name, False) for name in CASES] + [("composed", True)]


def device_name(name: str, flat: bool = False) -> str:
    return "vfops_" + name + ("_flat" if flat else "")


def prebuild_device_functions(jit):
    """Every device function of tests/test_gpu_vf_ops.py through ``jit.ensure_function`` (the build step compiles and caches them)."""
    from asset_asrl_amd import vf
    for name, flat in DEVICE_FORMS:
        with (flat_chain_rule() if flat else contextlib.nullcontext()):
            jit.ensure_function(build(name), device_name(name, flat))
    jit.ensure_function(trig3(vf.Arguments(3)), "vfops_trig3")


# --------------------------------------------------------------------------- csrc/asset_math.h: the argument sets

def trig3(a):
    """stack(sin x0, cos x1, tan x2), applied with x0 = x1 = x2: the value body of the device functor calls asset_sin, asset_cos and
    asset_tan (three arguments, so nothing is paired into a sincos there); the diagonal of its Jacobian is cos, -sin and 1 + tan^2."""
    from asset_asrl_amd import vf
    return vf.stack([vf.sin(a[0]), vf.cos(a[1]), vf.tan(a[2])])


AM_EXACT_RANGE = 2.0 ** 19 * (np.pi / 2)     # csrc/asset_math.h: the products of the reduction are exact below this
AM_ABS, AM_TAN_ULP = 2.0e-16, 4.0            # the header's own claim for sin / cos; tan = one quotient of two results good to 2 ulp
