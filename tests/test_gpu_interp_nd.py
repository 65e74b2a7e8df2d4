"""``vf.InterpTable2D`` / ``vf.InterpTable3D`` on the device: plain functions on the four tables of the 50-digit fixture
tests/golden/interp_nd/tables.npz through the function kernel, one application per stored point, within the fixture's bounds; an ODE on a
2-D cubic and a 3-D linear table through the defect kernels against its polynomial twin; the same ODE through the batched propagation
and its STM against the float64 restatement; a table in an event function and in a control law.  Every module is pre-built
(tests/interp_nd_cases.py: prebuild); the tests compile what they do not find.

Measured on an MI355X: the function kernel uses at most 0.27 of a fixture bound (the mixed function, m = 65; the single tables 0.26);
table ODE against twin, worst rel_err 7.1e-15 (Trapezoidal, 5 segments); propagation 2.4e-5 of the state bound and 0.048 of the STM
bound; event 0.050; control law 2.5e-5 (states) and 6.6e-5 (controls)."""
import numpy as np
import pytest

import controller_cases
import controller_checker as cck
import event_checker as eck
import integ_checker as gck
import interp_nd_cases as cases
import interp_nd_checker as ck
import propagate_checker as pck
from asset_asrl_amd import jit
from asset_asrl_amd.evaluator import (CON, CON_ADJGRAD, JAC, JAC_ADJGRAD, JAC_ADJGRAD_HESS, DefectEvaluator,
                                      unpack_kkt_block)
from asset_asrl_amd.pathfuncs import FunctionEvaluator
from helpers import Workload, rel_err
from test_gpu_propagate import _Problems

pytestmark = pytest.mark.gpu
U = ck.U
KINDS = (JAC_ADJGRAD_HESS, CON, CON_ADJGRAD, JAC, JAC_ADJGRAD)
WITH_L = (CON_ADJGRAD, JAC_ADJGRAD, JAC_ADJGRAD_HESS)
LD = np.longdouble


# ---- 1. the function kernel against the fixture
def _run_function(name, X, L, m, N, n):
    """{kind: (f[m, n], g[m, N] or None, J[m, n, N] or None, H[m, N, N] or None)} of one application per row of X"""
    vindex = np.arange(m * N, dtype=np.int32).reshape(m, N)
    cindex = np.arange(m * n, dtype=np.int32).reshape(m, n)
    ev = FunctionEvaluator(cases.function(name), cases.device_name(name), vindex, cindex, m * N, m * n)
    assert (ev.IR, ev.OR) == (N, n)
    out = {}
    for what in KINDS:
        fx, agx, kkt = ev.eval(what, X.ravel().copy(), L.ravel().copy() if what in WITH_L else None)
        f = np.asarray(fx).reshape(m, n)
        g = np.asarray(agx).reshape(m, N) if what in WITH_L else None
        J = H = None
        if what >= JAC:
            blocks = [unpack_kkt_block(b, N, n) for b in np.asarray(kkt).reshape(m, -1)]
            J = np.array([b[1] for b in blocks])
            if what == JAC_ADJGRAD_HESS:
                H = np.array([b[0] for b in blocks])
                assert np.array_equal(H, np.swapaxes(H, 1, 2))
        out[what] = (f, g, J, H)
    ev.close()
    return out


def _close(got, ref_ld, bound, what):
    """|got - ref| <= bound entry by entry, compared in long double; a bound of 0 asks for the value itself"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref_ld).astype(np.float64)
    bad = err > bound
    if np.any(bad):
        k = np.unravel_index(int(np.argmax(np.where(bad, err - bound, -1.0))), err.shape)
        raise AssertionError(f"{what}: entry {k}: |got - ref| = {err[k]:.3e} > bound {bound[k]:.3e}; {int(bad.sum())} of {err.size} entries miss")
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))


def _exact(e, m):
    hi, lo, E = (np.asarray(a[:m]) for a in e)
    return hi.astype(LD) + lo.astype(LD), U * E


@pytest.mark.parametrize("m", [1, 65])
@pytest.mark.parametrize("name", ck.TABLES)
def test_function_kernel_matches_the_fixture(name, m):
    """The table as a plain function, one application per point of the fixture (point 0 alone; a wave plus one -- neighbouring lanes in
    different cells, in and out of range).  Value and Jacobian within the fixture's bounds; the adjoint gradient lam grad and the
    adjoint Hessian lam H are linear in the fixture's entries: the bounds times |lam|, plus one rounding u |lam x| for the product."""
    N = ck.DIM[name]
    P = ck.load()[f"{name}_P"][:m]
    lam = np.random.default_rng(5).uniform(0.25, 2.0, m) * np.where(np.arange(m) % 2, -1.0, 1.0)
    e = ck.entries(name)
    (v, bv), (g, bg), (H, bH) = _exact(e["v"], m), _exact(e["g"], m), _exact(e["H"], m)
    worst = 0.0
    for what, (f, ag, J, Hd) in _run_function(name, P, lam, m, N, 1).items():
        tag = f"{name} x {m}, kind {what}:"
        worst = max(worst, _close(f[:, 0], v, bv, tag + " value"))
        if J is not None:
            worst = max(worst, _close(J[:, 0, :], g, bg, tag + " Jacobian"))
        if ag is not None:
            ref = lam.astype(LD)[:, None] * g
            worst = max(worst, _close(ag, ref, np.abs(lam)[:, None] * bg + U * np.abs(ref).astype(float), tag + " adjoint gradient"))
        if Hd is not None:
            ref = lam.astype(LD)[:, None, None] * H
            worst = max(worst, _close(Hd, ref, np.abs(lam)[:, None, None] * bH + U * np.abs(ref).astype(float), tag + " adjoint Hessian"))
    print(f"{name} x {m}: worst |got - ref| / bound = {worst:.3g}")


@pytest.mark.parametrize("m", [1, 65])
def test_function_mixing_two_tables_and_an_ordinary_term(m):
    """out0 = c2(y0, y1) + 0.5 y4, out1 = c3(y2, y3, y4) - 0.25 y0: application k reads point k of both fixture tables.  Bounds: the
    fixture's entries scaled by the multipliers, and u times the magnitude of every product and sum formed on top of them."""
    a, b = cases.MIX_TERMS
    fx = ck.load()
    Y = np.concatenate([fx["c2_P"][:m], fx["c3_P"][:m]], axis=1)
    lam = np.random.default_rng(6).uniform(0.25, 2.0, (m, 2)) * np.array([1.0, -1.0])
    e2, e3 = ck.entries("c2"), ck.entries("c3")
    (v2, bv2), (g2, bg2), (H2, bH2) = (_exact(e2[k], m) for k in "vgH")
    (v3, bv3), (g3, bg3), (H3, bH3) = (_exact(e3[k], m) for k in "vgH")
    Yl = Y.astype(LD)
    f_ref = np.stack([v2 + a * Yl[:, 4], v3 + b * Yl[:, 0]], axis=1)
    f_bnd = np.stack([bv2 + U * (np.abs(a * Y[:, 4]) + np.abs(f_ref[:, 0]).astype(float)), bv3 + U * (np.abs(b * Y[:, 0]) + np.abs(f_ref[:, 1]).astype(float))], axis=1)
    J_ref, J_bnd = np.zeros((m, 2, 5), dtype=LD), np.zeros((m, 2, 5))
    J_ref[:, 0, 0:2], J_bnd[:, 0, 0:2], J_ref[:, 0, 4] = g2, bg2, a
    J_ref[:, 1, 2:5], J_bnd[:, 1, 2:5], J_ref[:, 1, 0] = g3, bg3, b
    terms = lam.astype(LD)[:, :, None] * J_ref
    g_ref = terms.sum(axis=1)
    g_bnd = (np.abs(lam)[:, :, None] * J_bnd).sum(axis=1) + 2.0 * U * np.abs(terms).astype(float).sum(axis=1)
    H_ref, H_bnd = np.zeros((m, 5, 5), dtype=LD), np.zeros((m, 5, 5))
    H_ref[:, 0:2, 0:2] = lam.astype(LD)[:, 0, None, None] * H2
    H_ref[:, 2:5, 2:5] = lam.astype(LD)[:, 1, None, None] * H3
    H_bnd[:, 0:2, 0:2] = np.abs(lam)[:, 0, None, None] * bH2
    H_bnd[:, 2:5, 2:5] = np.abs(lam)[:, 1, None, None] * bH3
    H_bnd += U * np.abs(H_ref).astype(float)
    worst = 0.0
    for what, (f, ag, J, Hd) in _run_function("mixed", Y, lam, m, 5, 2).items():
        tag = f"mixed x {m}, kind {what}:"
        worst = max(worst, _close(f, f_ref, f_bnd, tag + " value"))
        if J is not None:
            worst = max(worst, _close(J, J_ref, J_bnd, tag + " Jacobian"))
        if ag is not None:
            worst = max(worst, _close(ag, g_ref, g_bnd, tag + " adjoint gradient"))
        if Hd is not None:
            worst = max(worst, _close(Hd, H_ref, H_bnd, tag + " adjoint Hessian"))
    print(f"mixed x {m}: worst |got - ref| / bound = {worst:.3g}")


# ---- 2. in a phase: the table ODE against its polynomial twin
def _phase_workload(mode, blocked, nseg):
    w = Workload("interp_nd", mode, nseg, blocked, sizes=(2, 1, 0), var_offset=1, con_offset=2, extra_vars=2)
    ix = w.indexer
    S = ix.numStates
    xtu = ix.XtVars() if w.blocked else ix.XtUVars()
    st = w.X[1:1 + S * xtu].reshape(S, xtu)
    rng = np.random.default_rng(8)
    st[:, 0] = rng.uniform(-1.9, 1.9, S)                                   # both tables end at +-1.6 in x0 ...
    st[:, 1] = rng.uniform(-1.8, 1.8, S)                                   # ... and the linear one at +-1.5 in x1
    if w.blocked:
        w.X[1 + S * xtu:1 + S * xtu + nseg] *= 1.7                         # the cubic table ends at +-1.5 in u
    else:
        st[:, 3] *= 1.7
    return w


@pytest.mark.parametrize("nseg", [5, 70])
@pytest.mark.parametrize("mode,blocked", cases.ODE_MODES)
def test_table_ode_in_a_phase_against_its_polynomial_twin(mode, blocked, nseg):
    """Both tables are sampled from polynomials they reproduce, so the table ODE and the ODE written with the polynomials are two
    float64 forms of one function: every block agrees as in tests/test_gpu_jit.py's block form against flat form (rel_err < 1e-12;
    tests/test_interp_nd_cpu.py holds the pair to a quarter of that through the plain-C builds)."""
    nt, np_ = jit.ensure_kernel(cases.make_ode(False), mode, blocked), jit.ensure_kernel(cases.make_ode(True), mode, blocked)
    assert nt != np_
    w = _phase_workload(mode, blocked, nseg)
    et = DefectEvaluator(nt, mode, w.blocked, w.vindex, w.cindex, w.n_primal, w.n_equal)
    ep = DefectEvaluator(np_, mode, w.blocked, w.vindex, w.cindex, w.n_primal, w.n_equal)
    worst = 0.0
    for what in (JAC_ADJGRAD_HESS, JAC_ADJGRAD, CON):
        L = w.L if what != CON else None
        a, b = et.eval(what, w.X, L), ep.eval(what, w.X, L)
        for x, y in zip(a, b):
            assert (x is None) == (y is None)
            if x is not None:
                assert np.all(np.isfinite(x)) and np.all(np.isfinite(y))
                worst = max(worst, rel_err(x, y))
                assert rel_err(x, y) < 1e-12
    fx, agx, kkt = et.eval(JAC_ADJGRAD_HESS, w.X, w.L)
    for V in (0, nseg // 2, nseg - 1):
        H, J = unpack_kkt_block(kkt[V], et.IR, et.OR)
        assert rel_err(J.T @ w.L[w.cindex[V]], agx[V]) < 1e-12 and rel_err(H, H.T) == 0.0
    print(f"{mode} blocked={blocked} x {nseg}: worst rel_err table against twin {worst:.3g}")
    et.close()
    ep.close()


# ---- 3. in propagation
def _configure(g, opt):
    g.setStepSizes(opt["def_step"], opt["min_step"], opt["max_step"])
    g.MaxStepChange, g.Adaptive, g.MaxSteps = opt["max_step_change"], opt["adaptive"], opt["max_steps"]
    g.setAbsTols(np.broadcast_to(opt["abs_tol"], (g.xv,)))
    g.setRelTols(np.broadcast_to(opt["rel_tol"], (g.xv,)))
    return g


def test_table_ode_in_batched_propagation_and_its_stm():
    """``ode.integrator(0.1)`` on the table ODE, three arcs, the middle one backwards, against tests/propagate_checker.py's restatement
    run on numpy callbacks built from the checker's tables: the comparison and bounds of tests/test_gpu_propagate.py, _Problems.check."""
    f, fj = cases.ode_callbacks()
    P = _Problems("interp_nd_table", (2, 1, 0), 3, 41, f, fj, lengths=(0.05, 0.2))
    P.tfs[1] = 2.0 * P.rows[1, 2] - P.tfs[1]
    assert P.tfs[1] < P.rows[1, 2] and P.tfs[0] > P.rows[0, 2] and P.tfs[2] > P.rows[2, 2]
    g = _configure(cases.make_ode(False).integrator(0.1), P.opt)
    rows, steps, status = g.integrate_parallel(P.rows, P.tfs, details=True)
    assert (status == 0).all()
    ids = np.arange(3)
    P.check(ids, np.array(rows)[:, :2], steps, what="table ODE x 3")
    res, ssteps, sstatus, _ = g.integrate_stm_parallel(P.rows, P.tfs, details=True)
    assert (sstatus == 0).all() and np.array_equal(ssteps, steps)
    xf, J = np.array([r[0][:2] for r in res]), np.array([r[1] for r in res])
    assert np.array_equal(xf, np.array(rows)[:, :2])
    P.check(ids, xf, ssteps, J, what="table ODE x 3, STM")


# ---- 4. as an event function and in a control law
def test_table_as_an_event_function():
    """g = cubic2(x0, x1) - level on the oscillator, two arcs (one backwards), against tests/event_checker.py's restatement with numpy
    callbacks from the checker's table: a case_from_restatement case at twice the bounds."""
    from test_gpu_propagate_events import _as_got, _integrator
    tab = cases.poly_restated("cubic2")
    eck.SYSTEMS["oscillator"]["events"]["interp_nd"] = (
        lambda y: y.dtype.type(tab.eval((float(y[0]), float(y[1])), 0)[0]) - y.dtype.type(cases.EVENT_LEVEL),
        lambda y: np.asarray(tab.eval((float(y[0]), float(y[1])), 1)[1], dtype=y.dtype))
    try:
        rows = np.array([[1.0 * np.cos(0.2), -1.0 * np.sin(0.2), 0.2], [0.8 * np.cos(1.0), -0.8 * np.sin(1.0), 1.0]])
        tfs = np.array([0.2 + 5.0, 1.0 - 4.0])
        opt = gck.options(def_step=0.05, max_step=0.25)
        case, B = eck.case_from_restatement("table event", "oscillator", ("interp_nd",), (0,), (0,), rows, tfs, opt, 1.0e-6, 8, np.ones((2, 2, 2)))
        assert (case["count"] > 0).all(), case["count"]                    # (the test's own premise: both arcs cross the level)
        g = _integrator("oscillator", opt)
        res, info = g.integrate_parallel(rows, tfs, [(cases.event_function(), 0, 0)], details=True)
        assert (info["status"] == 0).all()
        eck.compare_case(case, _as_got(res, info, 2), B, factor=2.0, what="device, table event:")
    finally:
        del eck.SYSTEMS["oscillator"]["events"]["interp_nd"]


def test_table_as_a_control_law():
    """u = cubic2(x0, t) on the double integrator, two arcs, against the closed loop of tests/controller_checker.py with the law and its
    Jacobian from the checker's table: end states by _Problems.check, the returned controls by the controller suite's rule (16 u |K| plus
    the law's Lipschitz bound times the state bound)."""
    tab = cases.poly_restated("cubic2")
    K = lambda z: np.array([tab.eval((z[0], z[1]), 0)[0]])                 # noqa: E731
    JK = lambda z: np.array([tab.eval((z[0], z[1]), 1)[1]])                # noqa: E731
    f_c, fj_c = cck.closed_loop(cck.pd_f, cck.pd_fj, (2, 1, 1), cases.LAW_VARLOCS, K, JK)
    P = _Problems("pd", (2, 1, 1), 2, 43, f_c, fj_c, lengths=(0.05, 0.3))
    ucon, varlocs = cases.control_law()
    g = _configure(controller_cases.make_ode("pd").integrator(P.opt["def_step"], ucon, varlocs), P.opt)
    end, steps, status = g.integrate_parallel(P.rows, P.tfs, details=True)
    end = np.array(end)
    assert (status == 0).all()
    ids = np.arange(2)
    P.check(ids, end[:, :2], steps, what="table law x 2")
    refs = [P.ref(i) for i in ids]
    S_max = np.maximum(np.abs(np.array([r["S"] for r in refs])[:, :, :2]), np.eye(2)[None])
    B = 2.0 * pck.state_bound(S_max, np.array([r["steps"] for r in refs])[:, 0], P.opt["abs_tol"])
    law = np.array([K(r[cases.LAW_VARLOCS]) for r in end])
    lip = np.array([np.abs(JK(r[cases.LAW_VARLOCS]))[:, 0] for r in end])                        # of the law's arguments, x0 alone is a state
    pck.compare(end[:, 3:4], law, 16.0 * U * np.abs(law) + lip * B[:, 0:1], "table law: the returned controls")
