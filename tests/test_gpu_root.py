"""``vf.ScalarRootFinder`` and ``astro.KeplerPropagator`` on the device: every case of the 50-digit fixture tests/golden/root/root.npz
as a plain function through the function kernel, one application per stored point, within the fixture's bounds (193 points: a partial
wave whose lanes leave the loop on different trips); the propagator against the batched propagation of the two-body ODE; an ODE written
with a root through the defect kernels against its closed-form twin; the same ODE through the batched propagation and its STM; a root in
an event function and in a control law.  Every module is pre-built (tests/root_cases.py: prebuild); the tests compile what they do not
find.

Measured on an MI355X: the function kernel uses at most 0.74 of a fixture bound (given_step, m = 193; the propagator 0.33); the propagator
against the batched propagation 0.0044 of the state bound and 0.13 of the STM bound; root ODE against twin, worst rel_err 3.0e-16; the
propagation of the root ODE 1.2e-5 (states) and 0.0070 (STM); event 0.19; the control law agrees with the closed loop bit for bit."""
import numpy as np
import pytest

import controller_cases
import controller_checker as cck
import event_checker as eck
import integ_checker as gck
import propagate_checker as pck
import root_cases as cases
from asset_asrl_amd import jit
from asset_asrl_amd.evaluator import (CON, CON_ADJGRAD, JAC, JAC_ADJGRAD, JAC_ADJGRAD_HESS, DefectEvaluator,
                                      unpack_kkt_block)
from asset_asrl_amd.pathfuncs import FunctionEvaluator
from helpers import Workload, rel_err
from test_gpu_propagate import _Problems

pytestmark = pytest.mark.gpu
U = cases.U
KINDS = (JAC_ADJGRAD_HESS, CON, CON_ADJGRAD, JAC, JAC_ADJGRAD)
WITH_L = (CON_ADJGRAD, JAC_ADJGRAD, JAC_ADJGRAD_HESS)
LD = np.longdouble


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


# ---- 1. the function kernel against the fixture
@pytest.mark.parametrize("m", [1, 193])
@pytest.mark.parametrize("name", cases.CASES)
def test_function_kernel_matches_the_fixture(name, m):
    """Value and Jacobian within the fixture's bounds; the adjoint Hessian is the fixture's lam^T H for its own lam, bound and all; the
    adjoint gradient J^T lam is linear in the Jacobian's entries: their bounds times |lam|, plus one rounding per product and sum."""
    N, n = cases.SIZES[name]
    fx = cases.load()
    P, lam = fx[f"{name}_P"][:m], fx[f"{name}_lam"][:m]
    (fr, fb), (Jr, Jb), (Hr, Hb) = (tuple(a[:m] for a in cases.entries(name, k)) for k in "fJH")
    terms = lam.astype(LD)[:, :, None] * Jr
    g_ref = terms.sum(axis=1)
    g_bnd = (np.abs(lam)[:, :, None] * Jb).sum(axis=1) + (n + 1) * U * np.abs(terms).astype(float).sum(axis=1)
    worst = 0.0
    for what, (f, ag, J, Hd) in _run_function(name, P, lam, m, N, n).items():
        tag = f"{name} x {m}, kind {what}:"
        worst = max(worst, cases.close(f, fr, fb, tag + " value"))
        if J is not None:
            worst = max(worst, cases.close(J, Jr, Jb, tag + " Jacobian"))
            if cases.HAS_GUESS[name]:
                assert not J[:, :, 0].any()
        if ag is not None:
            worst = max(worst, cases.close(ag, g_ref, g_bnd, tag + " adjoint gradient"))
        if Hd is not None:
            worst = max(worst, cases.close(Hd, Hr, Hb, tag + " adjoint Hessian"))
            if cases.HAS_GUESS[name]:
                assert not Hd[:, 0, :].any()
    print(f"{name} x {m}: worst |got - ref| / bound = {worst:.3g}")


# ---- 2. the propagator: all arcs in one call, and against the batched propagation of the two-body ODE
def _configure(g, opt):
    g.setStepSizes(opt["def_step"], opt["min_step"], opt["max_step"])
    g.MaxStepChange, g.Adaptive, g.MaxSteps = opt["max_step_change"], opt["adaptive"], opt["max_steps"]
    g.setAbsTols(np.broadcast_to(opt["abs_tol"], (g.xv,)))
    g.setRelTols(np.broadcast_to(opt["rel_tol"], (g.xv,)))
    return g


def test_kepler_propagator_against_the_fixture_and_the_batched_propagation():
    """The band points too (values only).  Then the three Kepler arcs: end state and STM of ``integrate_stm_parallel`` of twobody_lt with
    zero thrust against the propagator's value and d/d[R, V] -- two device paths that share no code.  The bound is the propagation's own
    (state_bound; 4 eS + 16 u |S|) PLUS the fixture's bound of the propagator's entry: the propagation's bound is its distance to the
    exact value, and the other side of this comparison is not exact either, it is within its own bound of it -- the triangle inequality,
    as tests/event_checker.py compares two restatements at twice the bounds.  The propagator's term on these three arcs is at most 9.1e-12 (end state) and
    5.5e-10 (Jacobian); measured shares of the sum: 0.0044 and 0.13."""
    from asset_asrl_amd.workloads import TwoBody
    fx = cases.load()
    band = fx["kepler_prop_band_P"]
    mb = band.shape[0]
    out = _run_function("kepler_prop", band, np.ones((mb, 6)), mb, 7, 6)[CON]
    cases.close(out[0], fx["kepler_prop_band_f"].astype(LD), fx["kepler_prop_band_fB"], "band")
    P = fx["kepler_prop_P"][:3]
    f, _, J, _ = _run_function("kepler_prop", P, np.ones((3, 6)), 3, 7, 6)[JAC]
    pf = pck.fixture()[1]
    for k, c in enumerate(("kepler_quarter", "kepler_full", "kepler_back")):
        case = pf[c]
        opt = pck.case_options(case)
        g = _configure(TwoBody().integrator(0.1), opt)
        res, steps, status, _ = g.integrate_stm_parallel(case["rows"], case["tfs"], details=True)
        assert (status == 0).all()
        xf, S = np.array(res[0][0][:6]), np.array(res[0][1])
        B = pck.state_bound(case["S_max"], case["steps64_stm"][:, 0], opt["abs_tol"])[0]
        pck.compare(xf[None], f[k][None], (B + fx["kepler_prop_fB"][k])[None], c + ": propagation against the propagator, end state")
        Sx = S[:, :6]
        bS = pck.stm_bound(case["S_exact"], case["eS"])[0][:, :6]
        pck.compare(Sx[None], J[k][:, :6][None], (bS + fx["kepler_prop_JB"][k][:, :6])[None], c + ": STM against the propagator's Jacobian")


# ---- 3. in a phase: the root ODE against its closed-form twin
@pytest.mark.parametrize("nseg", [5, 70])
@pytest.mark.parametrize("mode,blocked", cases.ODE_MODES)
def test_root_ode_in_a_phase_against_its_closed_form_twin(mode, blocked, nseg):
    """The loop inside the resident, row-wise and adjoint-gradient kernels: every block of every evaluation kind agrees with the ODE
    written with sqrt as in tests/test_gpu_jit.py's block form against flat form (rel_err < 1e-12; tests/test_root_cpu.py holds the
    pair to a quarter of that through the plain-C builds)."""
    nr, nt = jit.ensure_kernel(cases.make_ode(False), mode, blocked), jit.ensure_kernel(cases.make_ode(True), mode, blocked)
    assert nr != nt
    w = Workload("root_ode", mode, nseg, blocked, sizes=(2, 1, 0), var_offset=1, con_offset=2, extra_vars=2)
    er = DefectEvaluator(nr, mode, w.blocked, w.vindex, w.cindex, w.n_primal, w.n_equal)
    et = DefectEvaluator(nt, mode, w.blocked, w.vindex, w.cindex, w.n_primal, w.n_equal)
    worst = 0.0
    for what in KINDS:
        L = w.L if what in WITH_L else None
        a, b = er.eval(what, w.X, L), et.eval(what, w.X, L)
        for x, y in zip(a, b):
            assert (x is None) == (y is None)
            if x is not None:
                assert np.all(np.isfinite(x)) and np.all(np.isfinite(y))
                worst = max(worst, rel_err(x, y))
                assert rel_err(x, y) < 1e-12
    fx, agx, kkt = er.eval(JAC_ADJGRAD_HESS, w.X, w.L)
    for V in (0, nseg // 2, nseg - 1):
        H, J = unpack_kkt_block(kkt[V], er.IR, er.OR)
        assert rel_err(J.T @ w.L[w.cindex[V]], agx[V]) < 1e-12 and rel_err(H, H.T) == 0.0
    print(f"{mode} blocked={blocked} x {nseg}: worst rel_err root against twin {worst:.3g}")
    er.close()
    et.close()


# ---- 4. in propagation
def test_root_ode_in_batched_propagation_and_its_stm():
    """``ode.integrator(0.1)`` on the root ODE, three arcs, the middle one backwards, against tests/propagate_checker.py's restatement
    run on numpy callbacks written from the closed form: the comparison and bounds of tests/test_gpu_propagate.py, _Problems.check."""
    f, fj = cases.ode_callbacks()
    P = _Problems("root_newton", (2, 1, 0), 3, 47, f, fj, lengths=(0.05, 0.2))
    P.tfs[1] = 2.0 * P.rows[1, 2] - P.tfs[1]
    assert P.tfs[1] < P.rows[1, 2] and P.tfs[0] > P.rows[0, 2] and P.tfs[2] > P.rows[2, 2]
    g = _configure(cases.make_ode(False).integrator(0.1), P.opt)
    rows, steps, status = g.integrate_parallel(P.rows, P.tfs, details=True)
    assert (status == 0).all()
    ids = np.arange(3)
    P.check(ids, np.array(rows)[:, :2], steps, what="root ODE x 3")
    res, ssteps, sstatus, _ = g.integrate_stm_parallel(P.rows, P.tfs, details=True)
    assert (sstatus == 0).all() and np.array_equal(ssteps, steps)
    xf, J = np.array([r[0][:2] for r in res]), np.array([r[1] for r in res])
    assert np.array_equal(xf, np.array(rows)[:, :2])
    P.check(ids, xf, ssteps, J, what="root ODE x 3, STM")


# ---- 5. as an event function and in a control law
def test_root_as_an_event_function():
    """g = root(s^2 - (1 + 0.5 x0^2 + 0.3 x1)) - level on the oscillator, two arcs (one backwards), against tests/event_checker.py's
    restatement with numpy callbacks from the closed form: a case_from_restatement case at twice the bounds."""
    from test_gpu_propagate_events import _as_got, _integrator
    eck.SYSTEMS["oscillator"]["events"]["root"] = cases.event_np()
    try:
        rows = np.array([[1.0 * np.cos(0.2), -1.0 * np.sin(0.2), 0.2], [0.8 * np.cos(1.0), -0.8 * np.sin(1.0), 1.0]])
        tfs = np.array([0.2 + 5.0, 1.0 - 4.0])
        opt = gck.options(def_step=0.05, max_step=0.25)
        case, B = eck.case_from_restatement("root event", "oscillator", ("root",), (0,), (0,), rows, tfs, opt, 1.0e-6, 8, np.ones((2, 2, 2)))
        assert (case["count"] > 0).all(), case["count"]                    # (the test's own premise: both arcs cross the level)
        g = _integrator("oscillator", opt)
        res, info = g.integrate_parallel(rows, tfs, [(cases.event_function(), 0, 0)], details=True)
        assert (info["status"] == 0).all()
        eck.compare_case(case, _as_got(res, info, 2), B, factor=2.0, what="device, root event:")
    finally:
        del eck.SYSTEMS["oscillator"]["events"]["root"]


def test_root_as_a_control_law():
    """u = 0.5 - 0.5 root(s^2 - (1 + x0^2 + 0.2 sin t)) on the double integrator, two arcs, against the closed loop of
    tests/controller_checker.py with the law and its Jacobian from the closed form: end states by _Problems.check, the returned controls
    by the controller suite's rule (16 u |K| plus the law's Lipschitz bound times the state bound)."""
    K, JK = cases.law_np()
    f_c, fj_c = cck.closed_loop(cck.pd_f, cck.pd_fj, (2, 1, 1), cases.LAW_VARLOCS, K, JK)
    P = _Problems("pd", (2, 1, 1), 2, 43, f_c, fj_c, lengths=(0.05, 0.3))
    ucon, varlocs = cases.control_law()
    g = _configure(controller_cases.make_ode("pd").integrator(P.opt["def_step"], ucon, varlocs), P.opt)
    end, steps, status = g.integrate_parallel(P.rows, P.tfs, details=True)
    end = np.array(end)
    assert (status == 0).all()
    ids = np.arange(2)
    P.check(ids, end[:, :2], steps, what="root law x 2")
    refs = [P.ref(i) for i in ids]
    S_max = np.maximum(np.abs(np.array([r["S"] for r in refs])[:, :, :2]), np.eye(2)[None])
    B = 2.0 * pck.state_bound(S_max, np.array([r["steps"] for r in refs])[:, 0], P.opt["abs_tol"])
    law = np.array([K(r[cases.LAW_VARLOCS]) for r in end])
    lip = np.array([np.abs(JK(r[cases.LAW_VARLOCS]))[:, 0] for r in end])                        # of the law's arguments, x0 alone is a state
    pck.compare(end[:, 3:4], law, 16.0 * U * np.abs(law) + lip * B[:, 0:1], "root law: the returned controls")
