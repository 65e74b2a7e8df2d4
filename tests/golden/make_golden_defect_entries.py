"""Generate tests/golden/defect_entries/<shape>.npz: every entry of the defect blocks (fx, jx, gx = sum_k lam_k grad d_k,
hx = sum_k lam_k grad^2 d_k) of a few segments of EVERY shape the device has a kernel form for, as 50-digit values, each with a
running error bound E of its own (run once; commit the .npz files).

What is computed is the value formula of tests/golden/make_golden.py (``defect_value``, the ODE restatements, the collocation
tables of lgl_tables.json -- imported, not restated), differentiated exactly by second-order forward AD in 50-digit arithmetic.
The AD scalar here, ``DE``, is a sibling of make_golden's ``D2``: beside v, g[i], h[i][j] it carries, for each of them, a
first-order running error bound in units of u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.3):

    sum      r = a +- b     e_r = e_a + e_b + |r|          (no |r| where one operand is exactly 0: that sum is exact)
    product  r = a b        e_r = |a| e_b + |b| e_a + |r|  (term by term in the product-rule sums of g and h; no |r| for a
                                                            constant factor that is a power of two: that product is exact)
    unary    r = phi(a)     e_r = |phi'(a)| e_a + c_phi |r|,  c_phi = 1 for sqrt and the reciprocal, 2 for sin, cos, tan, exp
    inputs and double constants are exact (e = 0)

so u E bounds, to first order, the rounding error of a straightforward float64 evaluation of that entry by THIS recursion; other
algorithms (generated derivative code, FMA contraction, the device's M_i products and rank-2 time rows) are covered by the
measured constants kappa of tests/defect_checker.py.  An entry whose formula has no rounded term has E = 0: a structural zero,
or a value (such as the -1 of a Trapezoidal defect) that every float64 evaluation gets exactly.  The values are 50-digit mpf; the
error bounds are carried in float64 (their own rounding, 2^-53 per operation, is far inside the upward rounding to float32 they
are stored with).

Shapes: the 36 library shapes with a device kernel, and the run-time compiled families that reach kernels no library shape
reaches (coupled12 / driven14 in LGL7, shape_1_0_0 / shape_2_13_0 / shape_5_3_2 in LGL5), restated here from the formulas in the
docstrings of tests/helpers.py.  Segments: six per narrow shape -- three plain ones (those of the old golden vector where the
shape has one), one of 1e-4 of the width, one with reversed time (h < 0), one whose multipliers span 1e-6 ... 1e3 in magnitude
with two of them exactly 0.0 (one where the defect has only two or three rows: the ends of the span stay) -- and two for the wide shapes (synthetic32, coupled12,
driven14): a plain one and one with all three edges at once.

Usage:  python tests/golden/make_golden_defect_entries.py --jobs 8 [shape ...]
        python tests/golden/make_golden_defect_entries.py --constants      (measure the oracle, write kappa into the metadata)
"""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import defect_value, ref_table, segment_input, synth  # noqa: E402,F401

mp.mp.dps = 50
OUT = os.path.join(HERE, "defect_entries")
U = 2.0 ** -53
_ZERO = mp.mpf(0)
_tofloat = np.frompyfunc(float, 1, 1)


def _absf(a):
    """|a| of an object array of mpf as float64"""
    return np.abs(_tofloat(a).astype(float))


def _pow2(c: float) -> bool:
    return c != 0.0 and abs(math.frexp(c)[0]) == 0.5


# --------------------------------------------------------------------------- scalar with a running error
class S:
    """mpf value + running error (float, units of u) -- the derivative factors of the unary functions are formed with it"""

    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = v, e

    def __mul__(self, o):
        if isinstance(o, S):
            r = self.v * o.v
            return S(r, abs(float(self.v)) * o.e + abs(float(o.v)) * self.e + abs(float(r)))
        r = self.v * o
        return S(r, abs(float(o)) * self.e + (0.0 if _pow2(float(o)) else abs(float(r))))

    def __add__(self, o):
        if isinstance(o, S):
            r = self.v + o.v
            return S(r, self.e + o.e + (abs(float(r)) if self.v != 0 and o.v != 0 else 0.0))
        r = self.v + o
        return S(r, self.e + (abs(float(r)) if self.v != 0 and o != 0 else 0.0))

    def __neg__(self):
        return S(-self.v, self.e)

    def recip(self):
        r = 1 / self.v
        return S(r, float(r * r) * self.e + abs(float(r)))

    def fn(self, val, dval, c):
        return S(val, abs(float(dval)) * self.e + c * abs(float(val)))


# --------------------------------------------------------------------------- AD scalar with running errors
class DE:
    """value + gradient + Hessian w.r.t. N inputs (mpf, as make_golden.D2), each entry with its running error (float64)."""

    __slots__ = ("v", "g", "h", "ev", "eg", "eh", "_ag", "_ah")
    __array_ufunc__ = None      # (a numpy scalar on the left hands the operation to __rmul__ / __radd__)

    def __init__(self, v, g, h, ev, eg, eh, ag=None, ah=None):
        self.v, self.g, self.h, self.ev, self.eg, self.eh = v, g, h, ev, eg, eh
        self._ag, self._ah = ag, ah

    @property
    def ag(self):
        if self._ag is None:
            self._ag = _absf(self.g)
        return self._ag

    @property
    def ah(self):
        if self._ah is None:
            self._ah = _absf(self.h)
        return self._ah

    @staticmethod
    def const(c, n):
        return DE(mp.mpf(c), np.full(n, _ZERO, dtype=object), np.full((n, n), _ZERO, dtype=object), 0.0, np.zeros(n), np.zeros((n, n)))

    @staticmethod
    def var(val, i, n):
        d = DE.const(val, n)
        d.g[i] = mp.mpf(1)
        return d

    def _n(self):
        return self.g.shape[0]

    # ---- array helpers: (values, |values|, errors) in, (values, errors) out
    @staticmethod
    def _addarr(x, ax, ex, y, ay, ey):
        """ax, ay: |x|, |y| -- or anything that is non-zero exactly where they are; -> (r, e_r, |r|)"""
        r = x + y
        ar = _absf(r)
        return r, ex + ey + np.where((ax != 0) & (ay != 0), ar, 0.0), ar

    def _scale(self, s: S):
        """(s g, s h) with errors: a computed scalar times the arrays"""
        a = abs(float(s.v))
        g = self.g * s.v
        eg = a * self.eg + s.e * self.ag
        eg = eg + np.where(self.ag != 0, _absf(g), 0.0)
        h = self.h * s.v
        eh = a * self.eh + s.e * self.ah
        eh = eh + np.where(self.ah != 0, _absf(h), 0.0)
        return g, eg, h, eh

    @staticmethod
    def _outer(a, b):
        """outer(a.g, b.g) with errors"""
        og = np.outer(a.g, b.g)
        aog = np.outer(a.ag, b.ag)
        return og, aog, np.outer(a.ag, b.eg) + np.outer(a.eg, b.ag) + aog

    def _un(self, r: S, d1: S, d2: S):
        """phi(self): value r, phi' = d1, phi'' = d2 (each with its own running error)"""
        g, eg, h1, eh1 = self._scale(d1)
        og, aog, eog = DE._outer(self, self)
        a2 = abs(float(d2.v))
        h2 = og * d2.v
        eh2 = a2 * eog + d2.e * aog + np.where(aog != 0, _absf(h2), 0.0)
        h, eh, ah = DE._addarr(h1, self.ah, eh1, h2, aog, eh2)
        return DE(r.v, g, h, r.e, eg, eh, None, ah)

    def _s(self):
        return S(self.v, self.ev)

    def __add__(self, o):
        if not isinstance(o, DE):
            c = mp.mpf(o)
            r = self.v + c
            return DE(r, self.g, self.h, self.ev + (abs(float(r)) if self.v != 0 and c != 0 else 0.0), self.eg, self.eh, self._ag, self._ah)
        s = self._s() + o._s()
        g, eg, ag = DE._addarr(self.g, self.ag, self.eg, o.g, o.ag, o.eg)
        h, eh, ah = DE._addarr(self.h, self.ah, self.eh, o.h, o.ah, o.eh)
        return DE(s.v, g, h, s.e, eg, eh, ag, ah)

    __radd__ = __add__

    def __neg__(self):
        return DE(-self.v, -self.g, -self.h, self.ev, self.eg, self.eh, self._ag, self._ah)

    def __sub__(self, o):
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if not isinstance(o, DE):
            c = mp.mpf(o)
            a, exact = abs(float(c)), _pow2(float(c))
            v, g, h = self.v * c, self.g * c, self.h * c
            if exact:
                return DE(v, g, h, a * self.ev, a * self.eg, a * self.eh)
            return DE(v, g, h, a * self.ev + abs(float(v)), a * self.eg + _absf(g), a * self.eh + _absf(h))
        sa, sb = self._s(), o._s()
        s = sa * sb
        g1, eg1, h1, eh1 = self._scale(sb)
        g2, eg2, h2, eh2 = o._scale(sa)
        g, eg, ag = DE._addarr(g1, self.ag, eg1, g2, o.ag, eg2)
        h, eh, ah = DE._addarr(h1, self.ah, eh1, h2, o.ah, eh2)
        og, aog, eog = DE._outer(self, o)
        h, eh, ah = DE._addarr(h, ah, eh, og, aog, eog)
        h, eh, ah = DE._addarr(h, ah, eh, og.T, aog.T, eog.T)
        return DE(s.v, g, h, s.e, eg, eh, ag, ah)

    __rmul__ = __mul__

    def recip(self):
        a = self._s()
        r = a.recip()
        r2 = r * r
        return self._un(r, -r2, (r2 * r) * 2)

    def __truediv__(self, o):
        if not isinstance(o, DE):
            return self * (1 / mp.mpf(o))
        return self * o.recip()

    def __rtruediv__(self, o):
        return self.recip() * o

    def __pow__(self, k):
        if not isinstance(k, int):
            raise TypeError("DE ** k: integer powers only (as the ODE restatements use)")
        if k == 0:
            return DE.const(1, self._n())
        r = self
        for _ in range(abs(k) - 1):
            r = r * self
        return r if k > 0 else r.recip()


class ME:
    """math namespace for DE"""

    @staticmethod
    def sin(a):
        x = a._s()
        s, c = mp.sin(a.v), mp.cos(a.v)
        sv, cv = x.fn(s, c, 2.0), x.fn(c, s, 2.0)
        return a._un(sv, cv, -sv)

    @staticmethod
    def cos(a):
        x = a._s()
        s, c = mp.sin(a.v), mp.cos(a.v)
        sv, cv = x.fn(s, c, 2.0), x.fn(c, s, 2.0)
        return a._un(cv, -sv, -cv)

    @staticmethod
    def tan(a):
        t = mp.tan(a.v)
        tv = a._s().fn(t, 1 + t * t, 2.0)
        d = tv * tv + mp.mpf(1)
        return a._un(tv, d, (tv * d) * 2)

    @staticmethod
    def exp(a):
        e = mp.exp(a.v)
        ev = a._s().fn(e, e, 2.0)
        return a._un(ev, ev, ev)

    @staticmethod
    def sqrt(a):
        x = a._s()
        r = mp.sqrt(a.v)
        rv = x.fn(r, 1 / (2 * r), 1.0)
        return a._un(rv, (rv * 2).recip(), -((rv * x) * 4).recip())


# --------------------------------------------------------------------------- the run-time compiled families (tests/helpers.py)
def ode_coupled(n):
    def f(y, M):
        x, t, u, p0, p1 = y[:n], y[n], y[n + 1:n + 4], y[n + 4], y[n + 5]
        ct = M.cos(t)
        return [-0.5 * x[k] + M.sin(x[(k + 1) % n]) * x[(k + 5) % n] * u[k % 3] + p0 * ct + p1 * x[k] * x[(k + 7) % n] for k in range(n)]
    return f


def ode_driven(n):
    def f(y, M):
        x, t, u = y[:n], y[n], y[n + 1:n + 4]
        ct = M.cos(t)
        return [-0.5 * x[k] + M.sin(x[(k + 1) % n]) * x[(k + 5) % n] * u[k % 3] + 0.3 * ct * x[(k + 3) % n]
                + 0.1 * u[(k + 1) % 3] * u[(k + 1) % 3] for k in range(n)]
    return f


def ode_shape(n, m, p):
    def f(y, M):
        x, t, u, par = y[:n], y[n], y[n + 1:n + 1 + m], y[n + 1 + m:n + 1 + m + p]
        ct = M.cos(t)
        out = []
        for k in range(n):
            v = M.sin(x[(k + 1) % n]) * x[(k + 2) % n]
            if m > 0:
                v = v * u[k % m]
            v = v - 0.5 * x[k] + 0.3 * ct * x[(k + 3) % n]
            if m > 0:
                v = v + 0.1 * u[(k + 1) % m] * u[(k + 1) % m]
            if p > 0:
                v = v + par[0] * x[k] * x[(k + 1) % n] + par[p - 1] * ct
            out.append(v)
        return out
    return f


JIT_ODES = {"coupled12": ((12, 3, 2), ode_coupled(12)), "driven14": ((14, 3, 0), ode_driven(14)),
            "shape_1_0_0": ((1, 0, 0), ode_shape(1, 0, 0)), "shape_2_13_0": ((2, 13, 0), ode_shape(2, 13, 0)),
            "shape_5_3_2": ((5, 3, 2), ode_shape(5, 3, 2))}
WIDE = ("synthetic32", "coupled12", "driven14")


def sizes_of(name):
    return JIT_ODES[name][0] if name in JIT_ODES else synth.ODE_SIZES[name]


class _registered:
    """make_golden.defect_value / segment_input look an ODE up in make_golden.ODES and synth.ODE_SIZES: the run-time compiled
    families are entered there for the duration of a call and taken out again."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.added = self.name in JIT_ODES
        if self.added:
            synth.ODE_SIZES[self.name], mg.ODES[self.name] = JIT_ODES[self.name]

    def __exit__(self, *exc):
        if self.added:
            del synth.ODE_SIZES[self.name], mg.ODES[self.name]


# --------------------------------------------------------------------------- shapes and segments
def shapes():
    """[(ode, mode, blocked)]: the 36 library shapes with a device kernel, then the run-time compiled ones."""
    out = []
    for ode in ("brachistochrone", "reentry", "twobody_lt", "betts_lowthrust", "synthetic32"):
        for mode in ("Trapezoidal", "LGL3", "LGL5", "LGL7"):
            for blocked in (False, True):
                if blocked and synth.ODE_SIZES[ode][1] == 0:
                    continue
                out.append((ode, mode, blocked))
    out += [("coupled12", "LGL7", False), ("driven14", "LGL7", False), ("shape_1_0_0", "LGL5", False),
            ("shape_2_13_0", "LGL5", False), ("shape_2_13_0", "LGL5", True), ("shape_5_3_2", "LGL5", False),
            ("shape_5_3_2", "LGL5", True)]
    return out


def shape_name(ode, mode, blocked):
    return f"{ode}_{mode}{'_blocked' if blocked else ''}"


PLAIN, NARROW, REVERSED, WIDELAM = 1, 2, 4, 8


def segment_plan(ode, mode, blocked):
    """(mesh segments, seed, [(segment of the mesh, edge flags)]).  A shape with an old golden vector keeps that vector's mesh, seed
    and segments as its plain ones, so the two fixtures can be compared."""
    idx = shapes().index((ode, mode, blocked))
    old = [c for c in mg.CASES if (c[0], c[1], c[2]) == (ode, mode, blocked)]
    nm, segs, seed = (old[0][3], list(old[0][4]), old[0][5]) if old else (12, [0, 5, 11], 200 + idx)
    if ode in WIDE:
        plain = segs[:1]
        rest = [s for s in range(nm) if s not in plain]
        return nm, seed, [(plain[0], PLAIN), (rest[len(rest) // 2], NARROW | REVERSED | WIDELAM)]
    rest = [s for s in range(nm) if s not in segs]
    plain = (segs + rest[:2])[:3]
    rest = [s for s in rest if s not in plain]
    e = [rest[len(rest) // 4], rest[len(rest) // 2], rest[(3 * len(rest)) // 4]]
    return nm, seed, [(s, PLAIN) for s in plain] + [(e[0], NARROW), (e[1], REVERSED), (e[2], WIDELAM)]


def segment_inputs(ode, mode, blocked, k):
    """(z[IR], lam[OR]) of fixture segment k: float64, what every code under test is given"""
    nm, seed, plan = segment_plan(ode, mode, blocked)
    seg, flags = plan[k]
    xv, uv, pv = sizes_of(ode)
    cs = synth.MODE_CS[mode]
    with _registered(ode):
        traj = synth.make_traj(ode, mode, nm, seed=seed, sizes=sizes_of(ode) if ode in JIT_ODES else None)
        z = segment_input(ode, mode, blocked, traj, seg).copy()
    q = xv + 1 + (0 if blocked else uv)
    tix = [j * q + xv for j in range(cs)]
    t = z[tix].copy()
    if flags & NARROW:
        t = t[0] + 1e-4 * (t - t[0])
    if flags & REVERSED:
        t = t[-1] - (t - t[0])
    z[tix] = t
    OR = (cs - 1) * xv
    lam = synth.make_multipliers(OR, seed=seed + 100 + seg)
    if flags & WIDELAM:
        rng = np.random.default_rng(seed + 500 + seg)
        lam = np.where(rng.uniform(size=OR) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6.0, 3.0, OR)
        lam[0], lam[-1] = 1e-6, -1e3                                   # the span is there whatever the draw
        zero = rng.choice(np.arange(1, OR - 1), size=min(2, OR - 2), replace=False) if OR > 2 else np.array([0])
        lam[zero] = 0.0
    return z, lam


def _up32(e):
    """float64 -> float32, rounded upward (after a relative 2^-20 for the float64 carry of the bounds)"""
    e = np.asarray(e, dtype=np.float64) * (1.0 + 2.0 ** -20)
    f = e.astype(np.float32)
    low = f.astype(np.float64) < e
    f[low] = np.nextafter(f[low], np.float32(np.inf))
    assert np.all(f.astype(np.float64) >= e) and np.all((f == 0) == (e == 0))
    return f


def compute_segment(ode, mode, blocked, k):
    """One fixture segment: dict of float64 values and float32 bounds (hx as its lower triangle, row-major: (i, j <= i))."""
    z, lam = segment_inputs(ode, mode, blocked, k)
    IR, OR = z.size, lam.size
    with _registered(ode):
        d = defect_value(ode, mode, blocked, [DE.var(mp.mpf(float(v)), i, IR) for i, v in enumerate(z)], ME)
    assert len(d) == OR
    return blocks_of(d, z, lam)


def blocks_of(d, z, lam):
    """The fixture record of one application of a vector function: ``d`` = its outputs as DE over the inputs ``z``, contracted with
    the multipliers ``lam`` by the same rules (lambda is exact)."""
    IR, OR = z.size, lam.size
    il = np.tril_indices(IR)
    g, eg, ag = np.full(IR, _ZERO, dtype=object), np.zeros(IR), np.zeros(IR)
    h, eh, ah = np.full((IR, IR), _ZERO, dtype=object), np.zeros((IR, IR)), np.zeros((IR, IR))
    for kk in range(OR):
        l = mp.mpf(float(lam[kk]))
        al, exact = abs(float(lam[kk])), _pow2(float(lam[kk]))
        tg, th = d[kk].g * l, d[kk].h * l
        atg, ath = _absf(tg), _absf(th)
        etg = al * d[kk].eg + (0.0 if exact else atg)
        eth = al * d[kk].eh + (0.0 if exact else ath)
        g, eg, ag = DE._addarr(g, ag, eg, tg, atg, etg)
        h, eh, ah = DE._addarr(h, ah, eh, th, ath, eth)
    f64 = lambda a: _tofloat(a).astype(float)
    return dict(x=z, lam=lam,
                fx=np.array([float(e.v) for e in d]), fxE=_up32([e.ev for e in d]),
                jx=np.array([f64(e.g) for e in d]), jxE=_up32(np.array([e.eg for e in d])),
                gx=f64(g), gxE=_up32(eg), hx=f64(h)[il], hxE=_up32(np.maximum(eh, eh.T)[il]))


def _task(args):
    return args, compute_segment(*args)


def _cost(ode, mode, blocked):
    """rough relative cost of a segment, to start the long ones first"""
    xv, uv, pv = sizes_of(ode)
    cs = synth.MODE_CS[mode]
    ir = cs * (xv + 1 + (0 if blocked else uv)) + pv + (uv if blocked else 0)
    w = {"betts_lowthrust": 40.0, "reentry": 6.0, "twobody_lt": 3.0}.get(ode, 1.0) * max(xv, 4) / 4
    return ir * ir * (2 * cs - 1) * w


def commit_id():
    try:
        return subprocess.check_output(["git", "-C", HERE, "rev-parse", "HEAD"], text=True).strip()
    except Exception:
        return "unknown"


def path_of(ode, mode, blocked):
    return os.path.join(OUT, shape_name(ode, mode, blocked) + ".npz")


def write_shape(key, segs, constants=None):
    ode, mode, blocked = key
    nm, seed, plan = segment_plan(*key)
    meta = dict(generator="tests/golden/make_golden_defect_entries.py", commit=commit_id(), dps=mp.mp.dps, ode=ode, mode=mode,
                blocked=bool(blocked), sizes=list(sizes_of(ode)), mesh_segments=nm, seed=seed,
                segments=[int(s) for s, _ in plan], flags=[int(f) for _, f in plan],
                multiplier_seeds=[seed + 100 + int(s) for s, _ in plan], constants=constants)
    arr = {k: np.stack([s[k] for s in segs]) for k in segs[0]}
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(path_of(*key), meta=json.dumps(meta), **arr)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4, help="worker processes")
    ap.add_argument("--constants", action="store_true", help="measure the oracle against the fixtures, write kappa into every file")
    ap.add_argument("only", nargs="*", help="shape names (default: all)")
    a = ap.parse_args(argv)
    if a.constants:
        return write_constants()
    keys = [k for k in shapes() if not a.only or shape_name(*k) in a.only]
    tasks = [(k + (i,)) for k in keys for i in range(len(segment_plan(*k)[2]))]
    tasks.sort(key=lambda t: -_cost(*t[:3]))
    import multiprocessing
    done = {k: {} for k in keys}
    with multiprocessing.get_context("fork").Pool(a.jobs) as pool:
        for (ode, mode, blocked, i), seg in pool.imap_unordered(_task, tasks):
            key = (ode, mode, blocked)
            done[key][i] = seg
            if len(done[key]) == len(segment_plan(*key)[2]):
                write_shape(key, [done[key][j] for j in range(len(done[key]))])
                print("wrote", shape_name(*key), os.path.getsize(path_of(*key)), flush=True)
                done[key] = {}
    return 0


def write_constants():
    """The four kappa of tests/defect_checker.py, measured on the oracle's two providers (never on the device), into every file."""
    sys.path.insert(0, os.path.dirname(HERE))
    import defect_checker as dc
    constants = dc.measure_constants()
    for key in shapes():
        with np.load(path_of(*key)) as f:
            arr = {k: f[k] for k in f.files}
        meta = json.loads(str(arr.pop("meta")))
        meta["constants"] = constants
        np.savez_compressed(path_of(*key), meta=json.dumps(meta), **arr)
    print(json.dumps(constants, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
