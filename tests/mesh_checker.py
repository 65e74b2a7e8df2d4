"""Error bounds for the de Boor mesh-error estimate (csrc/mesh_kernels.h, oracle/mesh.cpp), and the loader of its 50-digit fixture
tests/golden/mesh_error.npz (written by tests/golden/make_golden_mesh.py).  Pure numpy; nothing here touches the code under test.

The estimate of block i and state k is built from   y_i = sum_j [ x_j xw_j F + f_j dxw_j F h ] / h^Order   (xw, dxw: the leading
power weights of the scheme's Hermite interpolant, F = Order! for the LGL schemes, 1 for Trapezoidal), then
    e_i = |y_i - y_(i-1)| / |h_i + h_(i-1)| + |y_(i+1) - y_i| / |h_i + h_(i+1)|        (twice the one difference at either end),
    mesh_errors_i = e_i |h_i|^(Order+1) ErrorWeight,        mesh_dist_i = e_i^(1/(Order+1)).
y_i divides O(1) node data by h^Order and the e_i difference the results: the estimate is ill-conditioned by construction, and a
fixed relative tolerance cannot be tight on random data and honest on smooth data.  The bound here follows the conditioning.  With
u = 2^-53, S_i the sum of the absolute values of the 2 cs terms of y_i, and Phi_i = sum_j |f(row_j)|_inf |dxw_j F h / h^Order|:

    |y_i - exact| <= delta_i = 16 u S_i + eps_f Phi_i
        16: at most 4 roundings in a term's product chain (xw F, its product with x, the reciprocal power, h), 2 cs <= 8 roundings in
        the accumulation of the 2 cs terms, 4 ulp for pow and the reciprocal together;
        eps_f: the relative error of the float64 right-hand side, measured per ODE against 50-digit arithmetic when the fixture is
        generated (its meta data holds the measured values and the factor 8 they are multiplied by: the device functor is generated
        code with its own operation order and FMA contraction).
    |e_i - exact| <= tau_i + 8 u e_i,   tau_i = the sum over the neighbour differences e_i uses of (delta_i + delta_nb) / |h_i + h_nb|
    mesh_errors: tau_i |h_i|^(Order+1) ErrorWeight + 8 u |ref|
    mesh_dist:   within [max(e - tau, 0)^(1/(Order+1)) (1 - 8u), (e + tau)^(1/(Order+1)) (1 + 8u)]  -- not linearised: on smooth fine
                 meshes tau exceeds e
    tsnd:        4 u
tau is linear in (S, Phi): the fixture stores the two neighbour combinations ``tau_s`` [xv, nb] and ``tau_phi`` [nb] and
``tau = 16 u tau_s + eps_f tau_phi``."""
from __future__ import annotations

import json
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(_HERE, "golden", "mesh_error.npz")
U = 2.0 ** -53
ROUNDINGS = 16.0
MODE_CS = {"Trapezoidal": 2, "LGL3": 2, "LGL5": 3, "LGL7": 4}
LD = np.longdouble


def scheme(mode: str):
    """(cs, Order, ErrorWeight, F, xw[cs], dxw[cs]) -- from tests/golden/lgl_tables.json; Trapezoidal: the literals of the estimator."""
    if mode == "Trapezoidal":
        return 2, 2, 1.0 / 12.0, 1.0, np.array([0.0, 0.0]), np.array([-1.0, 1.0])
    cs = MODE_CS[mode]
    t = json.load(open(os.path.join(_HERE, "golden", "lgl_tables.json")))["tables"][str(cs)]
    order = int(t["Order"])
    assert order == t["Order"]
    return (cs, order, float(t["ErrorWeight"]), float(math.factorial(order)),
            np.array(t["Cardinal_XPower_Weights"], dtype=float)[:, 0], np.array(t["Cardinal_DXPower_Weights"], dtype=float)[:, 0])


def block_rows(traj, mode: str, blocked: bool, xv: int, uv: int):
    """rows[nb, cs, N]: the node rows of every block; BlockConstant: the block's last row carries the first row's controls."""
    traj = np.asarray(traj, dtype=float)
    cs = MODE_CS[mode]
    K = cs - 1
    nb = (traj.shape[0] - 1) // K
    assert nb >= 2 and nb * K + 1 == traj.shape[0]
    rows = traj[np.arange(nb)[:, None] * K + np.arange(cs)[None, :]].copy()
    if blocked and uv > 0:
        rows[:, -1, xv + 1:xv + 1 + uv] = rows[:, 0, xv + 1:xv + 1 + uv]
    return rows


def block_rhs(rows, rhs, xv: int):
    """f[nb, cs, xv] of block_rows' rows through ``rhs(rows2d) -> f2d``."""
    nb, cs, N = rows.shape
    return np.asarray(rhs(rows.reshape(nb * cs, N)), dtype=float).reshape(nb, cs, xv)


def _terms(rows, f, mode: str, xv: int):
    """(h[nb], x-terms[nb, cs, xv], f-terms[nb, cs, xv], |f-weights|[nb, cs]) in longdouble."""
    cs, order, _, F, xw, dxw = scheme(mode)
    t = rows[:, :, xv].astype(LD)
    h = t[:, -1] - t[:, 0]
    hp = h ** order
    wx = (xw.astype(LD) * LD(F))[None, :] / hp[:, None]
    wf = (dxw.astype(LD) * LD(F))[None, :] * (h / hp)[:, None]
    return h, rows[:, :, :xv].astype(LD) * wx[:, :, None], f.astype(LD) * wf[:, :, None], np.abs(wf)


def neighbours(d, h):
    """The combination of per-block quantities d[nb, ...] that e_i makes of |y| differences: d_i + d_nb over |h_i + h_nb| for each
    neighbour difference used, doubled at the two ends."""
    d = np.asarray(d)
    pair = (d[:-1] + d[1:]) / np.abs(h[:-1] + h[1:]).reshape((-1,) + (1,) * (d.ndim - 1))
    out = np.empty_like(d)
    out[1:-1] = pair[:-1] + pair[1:]
    out[0], out[-1] = 2.0 * pair[0], 2.0 * pair[-1]
    return out


def tolerance_data(traj, mode: str, blocked: bool, xv: int, uv: int, rhs):
    """(tau_s[xv, nb], tau_phi[nb]) as float64: tau = 16 u tau_s + eps_f tau_phi (module docstring)."""
    rows = block_rows(traj, mode, blocked, xv, uv)
    f = block_rhs(rows, rhs, xv)
    h, tx, tf, wf = _terms(rows, f, mode, xv)
    S = np.abs(tx).sum(axis=1) + np.abs(tf).sum(axis=1)                     # [nb, xv]
    fn = np.abs(f).max(axis=2).astype(LD) if xv else np.zeros(f.shape[:2], dtype=LD)
    Phi = (fn * wf).sum(axis=1)                                             # [nb]
    return neighbours(S, h).T.astype(float), neighbours(Phi, h).astype(float)


def tau_of(tau_s, tau_phi, eps_f: float):
    return ROUNDINGS * U * np.asarray(tau_s) + float(eps_f) * np.asarray(tau_phi)[None, :]


def block_widths(traj, mode: str, xv: int):
    K = MODE_CS[mode] - 1
    tb = np.asarray(traj, dtype=float)[::K, xv]
    return np.diff(tb)


def estimate(traj, mode: str, blocked: bool, xv: int, uv: int, rhs):
    """(tsnd[nb+1], e[xv, nb+1], mesh_errors[xv, nb+1], mesh_dist[xv, nb+1]) of the formulas above, every sum in longdouble, rounded
    to float64 at the end.  NaN in the data goes where the formulas take it."""
    cs, order, ew, _, _, _ = scheme(mode)
    rows = block_rows(traj, mode, blocked, xv, uv)
    f = block_rhs(rows, rhs, xv)
    h, tx, tf, _ = _terms(rows, f, mode, xv)
    y = (tx + tf).sum(axis=1)
    with np.errstate(invalid="ignore"):
        pair = np.abs(y[:-1] - y[1:]) / np.abs(h[:-1] + h[1:])[:, None]
        e = np.empty_like(y)
        e[1:-1] = pair[:-1] + pair[1:]
        e[0], e[-1] = 2.0 * pair[0], 2.0 * pair[-1]
        err = e * (np.abs(h) ** (order + 1) * LD(ew))[:, None]
        dist = e ** (LD(1) / LD(order + 1))
    t = np.asarray(traj, dtype=float)[:, xv].astype(LD)
    tsnd = np.append((rows[:, 0, xv].astype(LD) - t[0]) / (t[-1] - t[0]), LD(1))
    last = lambda a: np.concatenate([a, a[-1:]], axis=0).T.astype(float)
    return tsnd.astype(float), last(e), last(err), last(dist)


def compare(got, ref, tau, h, mode: str, factor: float = 1.0, what: str = ""):
    """got = (tsnd, mesh_errors[xv, nb+1], mesh_dist[xv, nb+1]), ref = (tsnd, e[xv, nb+1], mesh_errors, mesh_dist), tau[xv, nb] (the
    last column takes the bound of the one it repeats), h[nb].  Asserts the module's bounds with `factor` times tau (2 where the
    reference is a float64 code itself) and returns the worst |got - ref| / bound of (tsnd, mesh_errors, mesh_dist).  A NaN must sit
    exactly where the reference has one."""
    _, order, ew, _, _, _ = scheme(mode)
    gt, gerr, gdist = (np.asarray(a, dtype=float) for a in got)
    rt, re, rerr, rdist = (np.asarray(a, dtype=float) for a in ref)
    assert gt.shape == rt.shape and gerr.shape == rerr.shape == gdist.shape == rdist.shape == re.shape, what
    tau = factor * np.concatenate([tau, tau[:, -1:]], axis=1)
    hh = np.abs(np.append(h, h[-1])).astype(LD)
    scale = (hh ** (order + 1) * LD(ew)).astype(float)[None, :]
    p = 1.0 / (order + 1)
    worst_t = float(np.abs(gt - rt).max() / (4.0 * U))
    assert worst_t <= 1.0, f"{what}: tsnd off by {worst_t * 4:.2f} u"
    nan = np.isnan(rerr)
    assert np.array_equal(np.isnan(gerr), nan) and np.array_equal(np.isnan(gdist), np.isnan(rdist)), f"{what}: NaN pattern differs"
    ok = ~nan
    berr = tau * scale + 8.0 * U * np.abs(rerr)
    lo = np.maximum(re - tau, 0.0) ** p * (1.0 - 8.0 * U)
    hi = (re + tau) ** p * (1.0 + 8.0 * U)
    with np.errstate(invalid="ignore", divide="ignore"):
        rerr_ratio = np.where(ok, np.abs(gerr - rerr) / berr, 0.0)
        up = np.where(gdist > rdist, (gdist - rdist) / (hi - rdist), 0.0)
        dn = np.where(gdist < rdist, (rdist - gdist) / (rdist - lo), 0.0)
        rdist_ratio = np.where(ok, np.maximum(up, dn), 0.0)
        inside = (gdist >= lo) & (gdist <= hi)
    # (a zero bound -- identical inputs give 0/0 -- passes only on exact equality)
    rerr_ratio = np.where(ok & (berr == 0.0), np.where(gerr == rerr, 0.0, np.inf), rerr_ratio)
    worst_e, worst_d = float(np.nanmax(rerr_ratio, initial=0.0)), float(np.nanmax(rdist_ratio, initial=0.0))
    bad = np.argwhere(ok & ~(np.abs(gerr - rerr) <= berr))
    assert bad.size == 0, (f"{what}: mesh_errors outside the bound at {len(bad)} entries, worst ratio {worst_e:.3g}; first (state, block) "
                           f"{tuple(bad[0])}: got {gerr[tuple(bad[0])]!r} ref {rerr[tuple(bad[0])]!r} bound {berr[tuple(bad[0])]:.3e}")
    bad = np.argwhere(ok & ~inside)
    assert bad.size == 0, (f"{what}: mesh_dist outside its interval at {len(bad)} entries, worst ratio {worst_d:.3g}; first (state, block) "
                           f"{tuple(bad[0])}: got {gdist[tuple(bad[0])]!r} not in [{lo[tuple(bad[0])]!r}, {hi[tuple(bad[0])]!r}]")
    return worst_t, worst_e, worst_d


def e_from_errors(err, h, mode: str):
    """e of a float64 code that returns mesh_errors only: mesh_errors / (|h|^(Order+1) ErrorWeight), in longdouble (its one extra
    rounding is far inside the 8 u of the mesh_dist interval)."""
    _, order, ew, _, _, _ = scheme(mode)
    hh = np.abs(np.append(h, h[-1])).astype(LD)
    return (np.asarray(err).astype(LD) / (hh ** (order + 1) * LD(ew))[None, :]).astype(float)


def compare_float64_codes(got, ref, traj, mode, blocked, xv, uv, rhs, eps_f, what="", factor=2.0):
    """Two float64 evaluations of the estimate (the device against the oracle): each is within tau of the exact value, so they are
    within 2 tau of each other (`factor`).  got / ref = (tsnd, mesh_errors, mesh_dist)."""
    h = block_widths(traj, mode, xv)
    tau = tau_of(*tolerance_data(traj, mode, blocked, xv, uv, rhs), eps_f)
    rt, rerr, rdist = ref
    return compare(got, (rt, e_from_errors(rerr, h, mode), rerr, rdist), tau, h, mode, factor=factor, what=what)


# ------------------------------------------------------------------------------------------------ the fixture
_CACHE = None


def fixture():
    """(meta, cases): meta the generator's record (eps_f per ODE, its factor, the case list), cases[name] a dict with the case's
    meta data and arrays -- 'traj' (the time-reversed cases: the stored trajectory reversed), 'tsnd', 'e', 'mesh_errors', 'mesh_dist',
    'tau_s', 'tau_phi'."""
    global _CACHE
    if _CACHE is None:
        z = np.load(FIXTURE)
        meta = json.loads(str(z["meta"]))
        cases = {}
        for c in meta["cases"]:
            for rev in (False, True):
                d = dict(c, reversed=rev)
                key = c["name"] + (".rev." if rev else ".fwd.")
                d["traj"] = z[c["name"] + ".traj"][::-1].copy() if rev else z[c["name"] + ".traj"]
                for a in ("tsnd", "e", "mesh_errors", "mesh_dist", "tau_s", "tau_phi"):
                    d[a] = z[key + a]
                d["zero_e"] = c["zero_e"][int(rev)]
                cases[c["name"] + ("-reversed" if rev else "")] = d
        _CACHE = (meta, cases)
    return _CACHE


def case_names():
    return list(fixture()[1]) if os.path.exists(FIXTURE) else []


def eps_f(ode: str) -> float:
    """The float64 right-hand side's relative error to use for `ode`: factor x the value measured at generation."""
    meta = fixture()[0]
    return meta["eps_f_factor"] * meta["eps_f_measured"][ode]


def compare_with_fixture(case, got, what=""):
    """got = (tsnd, mesh_errors, mesh_dist) of the case's trajectory against its 50-digit values."""
    h = block_widths(case["traj"], case["mode"], case["sizes"][0])
    tau = tau_of(case["tau_s"], case["tau_phi"], eps_f(case["ode"]))
    return compare(got, (case["tsnd"], case["e"], case["mesh_errors"], case["mesh_dist"]), tau, h, case["mode"], what=what)


def device_ode(case):
    """What asset_asrl_amd takes for the case's ODE: a library name, or a run-time compiled user ODE."""
    ode = case["ode"]
    if ode == "integrator":
        from interp_checker import make_integrator_ode
        return make_integrator_ode()
    if ode == "vanderpol":
        from helpers import make_vanderpol
        return make_vanderpol()
    if ode.startswith("shape_"):
        from helpers import make_shape
        return make_shape(*case["sizes"])
    return ode
