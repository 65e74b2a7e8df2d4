"""Generate tests/golden/traj_table/<case>.npz: every entry of the trajectory table's two outputs (the Hermite interpolant of a
trajectory and its time derivative, csrc/interp_kernels.h behind asset_hip_traj_table_* and LGLInterpTable) at a set of query times,
as 50-digit values, each with a running error bound E of its own (run once; commit the .npz files).

What is computed: per query time tau the block e -- the first whose end is not before tau in the direction of time, the first / last
block for a tau outside the data; comparing two doubles is exact -- and, with tb0 / tb1 the block's end times, h = tb1 - tb0 and
s = (tau - tb0) / h,

    x(tau)  = sum_i x_i phi_i(s) + f_i h psi_i(s)          x'(tau) = sum_i x_i phi_i'(s) / h + f_i psi_i'(s)
    u(tau)  = sum_i u_i ups_i(s)                            u'(tau) = sum_i u_i ups_i'(s) / h         (controls and parameters)
    t(tau)  = tb0 + h s                                     t'(tau) = 1
    BlockConstant: u(tau) = u of the block's first row, u'(tau) = 0

over the CS node rows of the block, f_i the ODE right-hand side at node row i.  Nothing is restated here: the right-hand sides are the
generic-scalar ODEs of make_golden.py, make_golden_mesh.py (vanderpol) and make_golden_defect_entries.py (the run-time compiled
families) -- all but ``manyparams``, the family this fixture adds (tests/helpers.py: make_manyparams) --, the power weights are read
from lgl_tables.json, and the scalar with a running error is make_golden_defect_entries.S (the right-hand sides run over its AD
sibling DE with no inputs: DE's value part is S, and ME forms its unary functions with S).

E, in units of u = 2^-53, is the first-order running error of the algorithm the head of csrc/interp_kernels.h documents -- NOT that of
plain Horner:

    h = tb1 - tb0                e_h = |h|                     one rounding
    s = (tau - tb0) / h          e_s = 3 |s|                   the difference, h, the quotient
    1 / h                        e = e_h / h^2 + |1 / h|
    a basis value p(s), p'(s)    e_p = |p| + |p'| e_s          the exact polynomial at the rounded s, rounded once: nothing for the
                                 e_p' = |p'| + |p''| e_s       size of the coefficients (2e3 in LGL7, 1.4e4 in the derivative).  That
                                                               is what the double-double Horner buys and what this fixture holds.
    h psi, phi' / h, ups' / h    products (S * S)
    the sums over the nodes      v = (v + x_i phi_i) + f_i (h psi_i), i = 0 .. CS - 1, a product and a sum each (the kernel's fused
                                 multiply-adds round once where this counts twice); x_i exact, f_i with the running error of its
                                 restatement
    t = tb0 + h s                a product and a sum

An entry with no rounded term has E = 0 and must be reproduced exactly: t' = 1.0, BlockConstant controls and parameters (the block's
first row) and their derivative 0.0 -- and t itself at tau = t0, where s = 0 and tb0 + h 0 is tb0.

Cases (CASES below): each the smallest mesh that reaches its edge.  Block widths are ragged over a spread of 1e4 with the narrowest
block (h = 1e-4) beside the widest (h = 1), so the derivative entries of the narrow block take the whole 1 / h.  States are random
(synth.make_traj).  Queries of every case, shuffled so that neighbouring lanes search different blocks: every node time, the doubles
next to every block boundary on both sides, t0 and tf, random interior times (drawn per block, four of them in the narrowest), and two
points outside each end (s = -0.3, -1e-9 of the first block, s = 1 + 1e-9, 1.2 of the last).

Usage:  python tests/golden/make_golden_traj_table.py [--jobs 8] [case ...]   (bit for bit the committed files; the record of the
                                                                               measured constants of a file that exists is kept)
        python tests/golden/make_golden_traj_table.py --constants             (measure kappa on the float64 model of
                                                                               tests/traj_table_checker.py, write it into every file)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_defect_entries as gde  # noqa: E402
from make_golden import synth  # noqa: E402
from make_golden_defect_entries import DE, JIT_ODES, ME, S, ode_shape  # noqa: E402,F401
from make_golden_mesh import ode_vanderpol  # noqa: E402
from make_golden_vf import write_npz  # noqa: E402

mp.mp.dps = 50
OUT = os.path.join(HERE, "traj_table")
MODE_CS = synth.MODE_CS
MODES = ("Trapezoidal", "LGL3", "LGL5", "LGL7")
_TABLES = json.load(open(os.path.join(HERE, "lgl_tables.json")))["tables"]
SIZE_CAP_FILE = os.path.join(HERE, "defect_entries", "synthetic32_LGL7.npz")


# --------------------------------------------------------------------------- the run-time compiled family this fixture adds
def ode_manyparams(n, p):
    """tests/helpers.py: make_manyparams -- x_k' = -x_k/2 + sin(x_{k+1}) x_{k+2} p_k + p_{p/2} x_k x_{k+1} + p_{p-1} cos t"""
    def f(y, M):
        x, t, par = y[:n], y[n], y[n + 1:n + 1 + p]
        ct = M.cos(t)
        return [-0.5 * x[k] + M.sin(x[(k + 1) % n]) * x[(k + 2) % n] * par[k] + par[p // 2] * x[k] * x[(k + 1) % n] + par[p - 1] * ct
                for k in range(n)]
    return f


# name -> ((xv, uv, pv), generic-scalar right-hand side)
ODES = {name: (synth.ODE_SIZES[name], mg.ODES[name]) for name in ("brachistochrone", "reentry", "twobody_lt", "betts_lowthrust", "synthetic32")}
ODES["coupled12"] = JIT_ODES["coupled12"]
ODES["vanderpol"] = ((2, 1, 1), ode_vanderpol)
ODES["manyparams_3_90"] = ((3, 0, 90), ode_manyparams(3, 90))
LIBRARY = tuple(synth.ODE_SIZES)


# --------------------------------------------------------------------------- cases
def _case(name, ode, mode, nb, blocked=False, reverse=False, nrand=36, t0=0.25, widest=1.0, spread=1.0e4):
    return dict(name=name, ode=ode, mode=mode, nb=nb, blocked=blocked, reverse=reverse, nrand=nrand, t0=t0, widest=widest, spread=spread)


def cases():
    out = []
    for mode in MODES:                                              # every mode, forward and time-reversed
        out.append(_case(f"reentry_{mode}", "reentry", mode, 5))
        out.append(_case(f"reentry_{mode}_reversed", "reentry", mode, 5, reverse=True))
    for mode in MODES:                                              # with and without BlockConstant
        out.append(_case(f"twobody_lt_{mode}", "twobody_lt", mode, 5))
        out.append(_case(f"twobody_lt_{mode}_blocked", "twobody_lt", mode, 5, blocked=True))
    out.append(_case("betts_lowthrust_LGL5", "betts_lowthrust", "LGL5", 5))
    out.append(_case("vanderpol_LGL7_blocked", "vanderpol", "LGL7", 5, blocked=True))
    # the widest library rows; 129 queries in all, for the GPU tests of 127, 128 and 129 queries (the other wide cases: 8 random ones)
    out.append(_case("synthetic32_LGL7", "synthetic32", "LGL7", 2, nrand=110))
    out.append(_case("coupled12_LGL7", "coupled12", "LGL7", 2, nrand=8))
    for mode in ("LGL3", "LGL7"):                                   # one block and two
        out.append(_case(f"reentry_{mode}_nb1", "reentry", mode, 1))
        out.append(_case(f"reentry_{mode}_nb2", "reentry", mode, 2))
    # node counts either side of a stage-1 workgroup of 64 rows
    out.append(_case("brachistochrone_Trapezoidal_nodes64", "brachistochrone", "Trapezoidal", 63))
    out.append(_case("brachistochrone_Trapezoidal_nodes65", "brachistochrone", "Trapezoidal", 64))
    out.append(_case("brachistochrone_LGL5_nodes65", "brachistochrone", "LGL5", 32))
    out.append(_case("brachistochrone_LGL7_nodes64", "brachistochrone", "LGL7", 21))
    out.append(_case("brachistochrone_LGL7_nodes67", "brachistochrone", "LGL7", 22))
    # times near 1e3 and h ~ 1e-3 (3e-4 ... 3e-3): tau - tb0 cancels six digits
    out.append(_case("reentry_LGL5_offset1e3", "reentry", "LGL5", 5, t0=1.0e3, widest=3.0e-3, spread=10.0))
    for mode in ("Trapezoidal", "LGL3"):                            # stage 1 without the LDS staging: (N|1) + (n|1) = 95 + 3 > 96
        out.append(_case(f"manyparams_3_90_{mode}", "manyparams_3_90", mode, 2, nrand=8))
    for i, c in enumerate(out):
        c["seed"] = 300 + i
    return out


def case_by_name(name):
    return next(c for c in cases() if c["name"] == name)


def path_of(name):
    return os.path.join(OUT, name + ".npz")


# --------------------------------------------------------------------------- trajectory and queries
def tc_of(cs):
    return np.array(_TABLES[str(cs)]["CardinalSpacings"], dtype=float)


def make_traj(c, seed):
    """Random states on a ragged mesh: widths in [widest / spread, widest], the narrowest beside the widest."""
    (xv, uv, pv), _ = ODES[c["ode"]]
    cs = MODE_CS[c["mode"]]
    K, nb = cs - 1, c["nb"]
    traj = synth.make_traj(c["ode"], c["mode"], nb, seed=seed, sizes=None if c["ode"] in LIBRARY else (xv, uv, pv))
    rng = np.random.default_rng(seed + 101)
    w = c["spread"] ** (-rng.uniform(0.0, 1.0, nb))
    if nb >= 2:
        a = int(rng.integers(0, nb - 1))
        w[a], w[a + 1] = 1.0 / c["spread"], 1.0
    else:
        w[0] = 1.0 / c["spread"]
    edges = c["t0"] + np.concatenate([[0.0], np.cumsum(w * c["widest"])])
    t, tc = np.empty(K * nb + 1), tc_of(cs)
    for j in range(K):
        t[j:-1:K] = edges[:-1] + tc[j] * (edges[1:] - edges[:-1])
    t[-1] = edges[-1]
    assert np.all(np.diff(t) > 0)
    traj[:, xv] = t
    return traj[::-1].copy() if c["reverse"] else traj


def make_times(c, traj, seed):
    xv = ODES[c["ode"]][0][0]
    K = MODE_CS[c["mode"]] - 1
    t = traj[:, xv]
    tb = t[::K]
    nb = tb.size - 1
    rng = np.random.default_rng(seed + 7)
    eb = rng.integers(0, nb, c["nrand"])
    eb[:4] = int(np.argmin(np.abs(np.diff(tb))))
    ss = rng.uniform(0.02, 0.98, c["nrand"])
    h0, h1 = tb[1] - tb[0], tb[-1] - tb[-2]
    out = np.array([tb[0] - 0.3 * h0, tb[0] - 1.0e-9 * h0, tb[-2] + (1.0 + 1.0e-9) * h1, tb[-2] + 1.2 * h1])
    d = 1.0 if tb[-1] > tb[0] else -1.0
    assert np.all(d * out[:2] < d * tb[0]) and np.all(d * out[2:] > d * tb[-1])
    q = np.concatenate([t, np.nextafter(tb, -np.inf), np.nextafter(tb, np.inf), [tb[0], tb[-1]],
                        tb[eb] + ss * (tb[eb + 1] - tb[eb]), out])
    return q[rng.permutation(q.size)]


def find_block(tb, tau):
    """(block, outside) of one time: the first block whose end is not before tau in the direction of time"""
    d = 1.0 if tb[-1] > tb[0] else -1.0
    nb = len(tb) - 1
    outside = d * tau < d * tb[0] or d * tau > d * tb[-1]
    for e in range(nb):
        if d * tau <= d * tb[e + 1]:
            return e, outside
    return nb - 1, outside


# --------------------------------------------------------------------------- the 50-digit table
def weights_mp(cs):
    t = _TABLES[str(cs)]
    f = lambda key: [[mp.mpf(float(v)) for v in row] for row in t[key]]
    return f("Cardinal_XPower_Weights"), f("Cardinal_DXPower_Weights"), f("Cardinal_UPolyPower_Weights")


def poly_mp(w, s):
    """(p, p', p'')(s) of the polynomial with coefficients w, highest power first"""
    p = d1 = d2 = mp.mpf(0)
    for c in w:
        d2 = d2 * s + 2 * d1
        d1 = d1 * s + p
        p = p * s + c
    return p, d1, d2


def rhs_S(ode, row):
    """f(row) as S: 50-digit value and the running error of the restatement"""
    out = ODES[ode][1]([DE.const(mp.mpf(float(v)), 0) for v in row], ME)
    return [S(o.v, float(o.ev)) if isinstance(o, DE) else S(mp.mpf(o), 0.0) for o in out]


def _basis(w, s, es):
    p, d1, d2 = poly_mp(w, s)
    return S(p, abs(float(p)) + abs(float(d1)) * es), S(d1, abs(float(d1)) + abs(float(d2)) * es)


def _acc(a, term):
    return term if a is None else a + term


def compute_case(c, seed=None):
    seed = c["seed"] if seed is None else seed
    (xv, uv, pv), _ = ODES[c["ode"]]
    cs = MODE_CS[c["mode"]]
    K, N = cs - 1, xv + 1 + uv + pv
    blocked = c["blocked"]
    traj = make_traj(c, seed)
    times = make_times(c, traj, seed)
    tb = [float(v) for v in traj[::K, xv]]
    Xw, DXw, Uw = weights_mp(cs)
    F = [rhs_S(c["ode"], row) for row in traj]
    nq = times.size
    val, der = np.zeros((nq, N)), np.zeros((nq, N))
    valE, derE = np.zeros((nq, N)), np.zeros((nq, N))
    block, outside = np.zeros(nq, dtype=np.int32), 0
    for q, tau in enumerate(times):
        tau = float(tau)
        e, out = find_block(tb, tau)
        block[q] = e
        outside += int(out)
        tb0, tb1 = mp.mpf(tb[e]), mp.mpf(tb[e + 1])
        h = tb1 - tb0
        s = (mp.mpf(tau) - tb0) / h
        es = 3.0 * abs(float(s))
        Sh = S(h, abs(float(h)))
        Sih = Sh.recip()
        Ss = S(s, es)
        phi, dphi, hpsi, dpsi, ups, dups = [], [], [], [], [], []
        for i in range(cs):
            p, dp = _basis(Xw[i], s, es)
            phi.append(p), dphi.append(dp * Sih)
            p, dp = _basis(DXw[i], s, es)
            hpsi.append(p * Sh), dpsi.append(dp)
            p, dp = _basis(Uw[i], s, es)
            ups.append(p), dups.append(dp * Sih)
        rows = traj[e * K:e * K + cs]
        for col in range(N):
            if col == xv:
                v, dv = Sh * Ss + tb0, S(mp.mpf(1), 0.0)
            elif col > xv and blocked:
                v, dv = S(mp.mpf(float(rows[0, col])), 0.0), S(mp.mpf(0), 0.0)
            else:
                v = dv = None
                for i in range(cs):
                    x = mp.mpf(float(rows[i, col]))
                    if col < xv:
                        f = F[e * K + i][col]
                        v = _acc(_acc(v, phi[i] * x), f * hpsi[i])
                        dv = _acc(_acc(dv, dphi[i] * x), f * dpsi[i])
                    else:
                        v, dv = _acc(v, ups[i] * x), _acc(dv, dups[i] * x)
            val[q, col], der[q, col], valE[q, col], derE[q, col] = float(v.v), float(dv.v), v.e, dv.e
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(der))
    return dict(traj=traj, times=times, block=block, outside=np.int64(outside), val=val, der=der,
                valE=gde._up32(valE), derE=gde._up32(derE))


def existing_constants(name):
    try:
        with np.load(path_of(name)) as f:
            return json.loads(str(f["meta"])).get("constants")
    except OSError:
        return None


def meta_of(c, constants):
    """The metadata record of a case, as the JSON text the file holds.  ``redrawn``: trajectory seeds given up because an entry's
    first-order E could not model a cancellation (none so far: every case keeps the seed of its place in the list)."""
    (xv, uv, pv), _ = ODES[c["ode"]]
    meta = dict(generator="tests/golden/make_golden_traj_table.py", dps=mp.mp.dps, sizes=[xv, uv, pv], redrawn=0,
                trajectory_seed=c["seed"], constants=constants, **c)
    return json.dumps(meta, sort_keys=True)


def write_case(c, arr, constants):
    os.makedirs(OUT, exist_ok=True)
    write_npz(path_of(c["name"]), dict(arr, meta=meta_of(c, constants)))


def _task(c):
    return c, compute_case(c)


def write_constants():
    import traj_table_checker as tc
    constants = tc.measure_constants()
    for c in cases():
        with np.load(path_of(c["name"])) as f:
            arr = {k: f[k] for k in f.files}
        meta = json.loads(str(arr.pop("meta")))
        meta["constants"] = constants
        write_npz(path_of(c["name"]), dict(arr, meta=json.dumps(meta, sort_keys=True)))
    print(json.dumps(constants, indent=1))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4, help="worker processes")
    ap.add_argument("--constants", action="store_true", help="measure the float64 model against the fixtures, write kappa into every file")
    ap.add_argument("only", nargs="*", help="case names (default: all)")
    a = ap.parse_args(argv)
    if a.constants:
        return write_constants()
    todo = [c for c in cases() if not a.only or c["name"] in a.only]
    cap = os.path.getsize(SIZE_CAP_FILE)
    import multiprocessing
    with multiprocessing.get_context("fork").Pool(a.jobs) as pool:
        for c, arr in pool.imap_unordered(_task, todo):
            write_case(c, arr, existing_constants(c["name"]))
            size = os.path.getsize(path_of(c["name"]))
            print("wrote", c["name"], arr["times"].size, "queries", size, "bytes", flush=True)
            assert size < cap, (c["name"], size, cap)
    return 0


if __name__ == "__main__":
    sys.exit(main())
