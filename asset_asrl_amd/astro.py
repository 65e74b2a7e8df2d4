"""Astrodynamics functions built on the ``vf`` DSL.

``KeplerPropagator(mu)``: the two-body state ``[R, V]`` after a time ``dt`` as ONE expression, usable wherever a VectorFunction is --
a plain function on the device, a term of an ODE, an event function, a control law -- the reference's ``Astro.Kepler.KeplerPropagator``
(/root/reference/src/Astro/KeplerPropagator.h).  Written from the textbook universal-variable formulation (Bate, Mueller & White,
section 4.4; Vallado, algorithm 8), with ``vf.ScalarRootFinder`` for the universal anomaly: every derivative of the result comes from
the implicit-function rule of the root node (vf/ir.py) and the ordinary rules of everything around it.
"""
from __future__ import annotations

import math

from . import vf


def stumpff(psi, conictol: float):
    """(c2, c3) of the scalar function psi: the elliptic forms above `conictol`, the hyperbolic ones below ``-conictol``, the limits
    1/2 and 1/6 in between -- two nested ``ifelse`` each."""
    sq = vf.sqrt(psi)
    c2e, c3e = (1.0 - vf.cos(sq)) / psi, (sq - vf.sin(sq)) / (sq * psi)
    sh = vf.sqrt(-1.0 * psi)
    c2h, c3h = (1.0 - vf.cosh(sh)) / psi, (vf.sinh(sh) - sh) / (sh * (-1.0 * psi))
    c2 = vf.ifelse(psi > conictol, c2e, vf.ifelse(psi < -conictol, c2h, 0.5))
    c3 = vf.ifelse(psi > conictol, c3e, vf.ifelse(psi < -conictol, c3h, 1.0 / 6.0))
    return c2, c3


def _kepler_terms(chi, alpha, sigma, r, conictol):
    """What the residual, its derivative and the Lagrange coefficients share, over scalar functions of one common input size."""
    chi2 = chi * chi
    psi = alpha * chi2
    c2, c3 = stumpff(psi, conictol)
    rho = chi2 * c2 + sigma * chi * (1.0 - psi * c3) + r * (1.0 - psi * c2)       # = -dF/dchi = |R_f|
    return chi2, psi, c2, c3, rho


def KeplerPropagator(mu: float, conictol: float = 1.0e-11, roottol: float = 1.0e-12, iters: int = 19) -> vf.VectorFunction:
    """``[R, V, dt] -> [R_f, V_f]`` (7 inputs, 6 outputs) of the two-body problem with gravitational parameter `mu`; the defaults
    are the reference's (KeplerPropagator.h:291-293).

    With ``r = |R|``, ``sigma = R.V / sqrt(mu)``, ``alpha = 2/r - |V|^2/mu`` and ``psi = alpha chi^2`` the universal anomaly ``chi``
    solves ``F(chi) = sqrt(mu) dt - chi^3 c3(psi) - sigma chi^2 c2(psi) - r chi (1 - psi c3(psi)) = 0``; Newton's iteration steps
    with the closed form ``F_chi = -(chi^2 c2 + sigma chi (1 - psi c3) + r (1 - psi c2))`` from the guess ``sqrt(mu) dt alpha``
    (``alpha >= 0``) or the logarithmic hyperbolic guess.  Then ``f = 1 - chi^2 c2 / r``, ``g = dt - chi^3 c3 / sqrt(mu)``,
    ``fdot = chi (psi c3 - 1) sqrt(mu) / (rho r)``, ``gdot = 1 - chi^2 c2 / rho`` with ``rho = -F_chi``, and
    ``R_f = f R + g V``, ``V_f = fdot R + gdot V``.

    Limits, all the reference's: the iteration is plain Newton with at most `iters` passes and returns its last iterate where it has
    not converged, without a sign of it.  The logarithmic guess is poor on hyperbolic arcs close to the parabola (``alpha`` a little below
    zero: ``sqrt(-1/alpha)`` is huge): for ``alpha`` of order -1e-12 it lies millions of units from the root and 19 passes do not reach
    it; raise `iters` for such arcs, or split them.  A few long elliptic and hyperbolic arcs with ``|alpha|`` of order 0.1 to 1 need more
    than 19 passes too (7 of 209 random draws of the test fixture).  Within ``|psi| < conictol`` the constants stand for the Stumpff
    functions, a relative error of about ``|psi| / 12``; just outside that band their closed forms cancel (``(1 - cos sqrt(psi)) / psi``), so
    arcs with a small ``|psi|`` lose digits in the value and more in the derivatives."""
    mu = float(mu)
    if not (math.isfinite(mu) and mu > 0.0):
        raise ValueError(f"KeplerPropagator: mu = {mu!r} is not a finite positive number")
    sqmu = math.sqrt(mu)
    # ---- the equation, over [chi, alpha, sigma, r, sqrt(mu) dt]
    t = vf.Arguments(5)
    chi, alpha, sigma, r, smdt = t.tolist()
    chi2, psi, c2, c3, rho = _kepler_terms(chi, alpha, sigma, r, conictol)
    fx = smdt - chi2 * chi * c3 - sigma * chi2 * c2 - r * chi * (1.0 - psi * c3)
    root = vf.ScalarRootFinder(fx, -1.0 * rho, iters, roottol)
    # ---- its arguments, over [R, V, dt]
    a = vf.Arguments(7)
    R, V, dt = a.head(3), a.segment(3, 3), a[6]
    rn = R.norm()
    rv = R.dot(V)
    al = 2.0 / rn - V.squared_norm() / mu
    sg = rv / sqmu
    sdt = sqmu * dt
    # the hyperbolic guess: sign(dt) sqrt(-a) log(-2 mu alpha dt / (R.V + sign(dt) sqrt(-mu a) (1 - r alpha))),  a = 1 / alpha
    sgn = vf.sign(dt)
    am = -1.0 / al
    hyp = sgn * vf.sqrt(am) * vf.log((-2.0 * mu) * al * dt / (rv + sgn * vf.sqrt(mu * am) * (1.0 - rn * al)))
    guess = vf.ifelse(al >= 0.0, sdt * al, hyp)
    x = root.eval(vf.stack([guess, al, sg, rn, sdt]))
    # ---- the Lagrange coefficients at the root
    x2, ps, d2, d3, rh = _kepler_terms(x, al, sg, rn, conictol)
    f = 1.0 - x2 * d2 / rn
    g = dt - x2 * x * d3 / sqmu
    fd = x * (ps * d3 - 1.0) * sqmu / (rh * rn)
    gd = 1.0 - x2 * d2 / rh
    return vf.stack([f * R + g * V, fd * R + gd * V])
