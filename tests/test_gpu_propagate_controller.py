"""The batched propagation with a controller on the device (csrc/propagate_ctrl_kernels.h through asset_hip_propagate_ctrl /
asset_hip_propagate_ctrl_stm and ``ode.integrator(def_step, ucon, varlocs)``) against the 50-digit fixture
tests/golden/propagate_controller/controller.npz and -- where there is no fixture -- against the float64 restatement of
tests/propagate_checker.py run on the closed loop of tests/controller_checker.py (each side within its bound of the exact state, so the
two are within twice the bound of each other): every fixture case with the controls of every returned row, the bitwise claims (STM call
against batch call, across the lanes of a group, a pass-through law against held controls, the constant controller against held
controls), tangential thrust in a mixed wave, the edges of the launch shape, and the statuses.

Measured on an MI355X, worst |got - ref| / bound per fixture case (end states, samples, STM, d xf / d t0, d xf / d tf, controls):
see the table in DESIGN.md 4.13."""
import functools

import numpy as np
import pytest

import controller_cases as cc
import controller_checker as cck
import integ_checker as gck
import propagate_checker as pck
from test_gpu_propagate import _Problems, _same_bits

pytestmark = pytest.mark.gpu
U = pck.U


def _integrator(law, opt):
    g = cc.integrator(law, opt["def_step"], "DOPRI87")
    g.setStepSizes(opt["def_step"], opt["min_step"], opt["max_step"])
    g.MaxStepChange, g.Adaptive, g.MaxSteps = opt["max_step_change"], opt["adaptive"], opt["max_steps"]
    g.setAbsTols(np.broadcast_to(opt["abs_tol"], (g.xv,)))
    g.setRelTols(np.broadcast_to(opt["rel_tol"], (g.xv,)))
    return g


def _stm(g, rows, tfs):
    """(end rows[m, N], J[m, n, N + 1], steps, status, xf_last) of integrate_stm_parallel(details=True)"""
    res, steps, status, last = g.integrate_stm_parallel(rows, tfs, details=True)
    return np.array([r[0] for r in res]), np.array([r[1] for r in res]), steps, status, last


def _same_rows(a, b, n, uv, what):
    """two sets of full rows bit for bit, but for their controls: the law is evaluated by another kernel (the STM's assembly kernel against
    the batch kernel), where the compiler is free to contract its operations differently -- those are held to the law itself"""
    a, b = np.asarray(a), np.asarray(b)
    _same_bits(a[..., :n + 1], b[..., :n + 1], what + " (states, times)")
    _same_bits(a[..., n + 1 + uv:], b[..., n + 1 + uv:], what + " (parameters)")


def _check_controls(law, got_rows, B, what, factor=1.0):
    """the u entries of returned rows[..., N] against the numpy law at each row: 16 u |K| + the law's Lipschitz bound times the state bound"""
    system = cck.LAWS[law][0]
    n, uv, _ = cck.SIZES[system]
    got_rows = np.asarray(got_rows)
    pck.compare(got_rows[..., n + 1:n + 1 + uv], cck.law_value(law, got_rows), factor * cck.control_bound(law, got_rows, B), what + ": controls")


# ---- 1. the fixture (and the bitwise claims of the STM call on its cases)
@pytest.mark.parametrize("name", cck.case_names())
def test_device_matches_the_50_digit_fixture(oracle, name):
    c = cck.fixture()[1][name]
    law = c["law"]
    n, uv, pv = c["sizes"]
    N, ns, rows, tfs = n + 1 + uv + pv, c["ns"], c["rows"], c["tfs"]
    us = slice(n + 1, n + 1 + uv)
    opt = pck.case_options(c)
    g = _integrator(law, opt)
    end, steps, status = g.integrate_parallel(rows, tfs, details=True)
    end = np.array(end)
    assert (status == 0).all(), status
    assert end.shape == (len(tfs), N) and np.array_equal(end[:, n], tfs) and np.array_equal(end[:, n + 1 + uv:], rows[:, n + 1 + uv:])
    srows, J, steps_s, status_s, last = _stm(g, rows, tfs)
    assert (status_s == 0).all() and np.array_equal(steps_s, steps)
    _same_rows(srows, end, n, uv, "integrate_stm_parallel's rows against integrate_parallel's")
    _same_bits(last, end[:, :n], "the last lane of a group against lane 0")
    plain = g.integrate_stm_parallel(rows, tfs)                                       # (asset_hip_propagate_ctrl_stm itself)
    _same_bits(np.array([r[0] for r in plain]), srows, "the plain STM entry's rows against the diagnostic one's")
    _same_bits(np.array([r[1] for r in plain]), J, "the plain STM entry point against the diagnostic one")
    assert np.all(J[:, :, us] == 0.0) and not np.signbit(J[:, :, us]).any(), "the STM's u columns are exactly 0.0"
    S = np.concatenate([J[:, :, :n], J[:, :, n + 1:N]], axis=2)
    f_c = cck.closed_loop_of(oracle, law)[0]
    if opt["adaptive"]:
        B = pck.state_bound(c["S_max"], c["steps64_end"][:, 0], opt["abs_tol"])
        pck.compare(end[:, :n], c["x_exact"][:, -1], B, f"{name}: end states")
        gck.compare_step_totals(steps, c["steps64_end"], name)
        pck.compare(S, c["S_exact"], pck.stm_bound(c["S_exact"], c["eS"]), f"{name}: STM")
        b0, bf = pck.time_column_bounds(c["S_exact"], c["eS"], c["f0"], c["Jxf_abs"], B, c["dtf_exact"])
        pck.compare(J[:, :, n], c["dt0_exact"], b0, f"{name}: d xf / d t0")
        pck.compare(J[:, :, N], c["dtf_exact"], bf, f"{name}: d xf / d tf")
    else:
        B = 8.0 * c["d64"] + 16.0 * U * np.abs(c["xld"]).astype(float)
        pck.compare(end[:, :n], c["xld"], B, f"{name}: end states against the longdouble restatement")
        np.testing.assert_array_equal(steps, c["steps64_end"])
        pck.compare(S, c["Sld"], 8.0 * c["dS64"] + 16.0 * U * np.abs(c["Sld"]).astype(float), f"{name}: STM against the longdouble restatement")
        d0, df = pck.time_columns(f_c, rows, tfs, c["xld"].astype(float), c["Sld"])
        b0, bf = pck.time_column_bounds(c["Sld"].astype(float), 2.0 * c["dS64"].max(axis=(1, 2)), c["f0"], c["Jxf_abs"], B, c["dtf_exact"])
        pck.compare(J[:, :, n], d0, b0, f"{name}: d xf / d t0")
        pck.compare(J[:, :, N], df, bf, f"{name}: d xf / d tf")
    _check_controls(law, end, B, f"{name}: end rows")
    _check_controls(law, srows, B, f"{name}: the STM call's rows")
    if ns > 1:
        trajs, dsteps, dstatus = g.integrate_dense_parallel(rows, tfs, ns, details=True)
        T = np.array(trajs)
        assert (dstatus == 0).all() and T.shape == (len(tfs), ns, N)
        for i in range(len(tfs)):
            np.testing.assert_array_equal(T[i, :, n], pck.sample_times(rows[i, n], tfs[i], ns))
        assert np.array_equal(T[:, :, n + 1 + uv:], np.repeat(rows[:, None, n + 1 + uv:], ns, axis=1))
        _same_bits(T[:, 0, :n], rows[:, :n], "sample 0 is x0")
        Bd = np.repeat(pck.state_bound(c["S_max"], c["steps64"][:, 0], opt["abs_tol"])[:, None, :], ns, axis=1)
        pck.compare(T[:, :, :n], c["x_exact"], Bd, f"{name}: samples")
        gck.compare_step_totals(dsteps, c["steps64"], name + " dense")
        Bd[:, 0, :] = 0.0                                                             # (sample 0 is x0 itself: rounding of the law alone)
        _check_controls(law, T, Bd, f"{name}: every sample, sample 0 included")
        assert not np.any(T[:, :, us] == 7.0), "the rows' own controls are not returned"
    print(f"{name}: steps {steps.sum(axis=0)} against the restatement's {c['steps64_end'].sum(axis=0)}")


# ---- 2. bitwise: a pass-through law against held controls
def test_a_pass_through_law_is_the_held_control_propagation_bit_for_bit():
    """u = row[4] = mu on vanderpol against the held-control call whose rows carry u = mu: the same right-hand side on the same data"""
    from helpers import make_vanderpol
    rng = np.random.default_rng(12)
    rows = np.column_stack([rng.uniform(-1, 1, (70, 2)), rng.uniform(0, 1, 70), np.full(70, 9.0), rng.uniform(0.5, 1.5, 70)])
    tfs = rows[:, 2] + rng.uniform(0.1, 0.5, 70) * rng.choice([-1.0, 1.0], 70)
    held = rows.copy()
    held[:, 3] = held[:, 4]
    g, h = cc.integrator("vdp_pass", 0.05), make_vanderpol().integrator(0.05)
    a, asteps, astatus = g.integrate_parallel(rows, tfs, details=True)
    b, bsteps, bstatus = h.integrate_parallel(held, tfs, details=True)
    assert (astatus == 0).all() and (bstatus == 0).all() and np.array_equal(asteps, bsteps)
    _same_bits(np.array(a), np.array(b), "end rows: states, times, u = mu, parameters")
    da, db = np.array(g.integrate_dense_parallel(rows, tfs, 4)), np.array(h.integrate_dense_parallel(held, tfs, 4))
    _same_bits(da, db, "dense rows")


# ---- 6. the constant controller
def test_the_constant_controller_is_the_held_control_call_bit_for_bit():
    from helpers import make_vanderpol
    rng = np.random.default_rng(13)
    rows = np.column_stack([rng.uniform(-1, 1, (9, 2)), rng.uniform(0, 1, 9), np.full(9, 9.0), rng.uniform(0.5, 1.5, 9)])
    tfs = rows[:, 2] + 0.4
    held = rows.copy()
    held[:, 3] = 0.3
    g, h = make_vanderpol().integrator(0.05, 0.3), make_vanderpol().integrator(0.05)
    _same_bits(np.array(g.integrate_parallel(rows, tfs)), np.array(h.integrate_parallel(held, tfs)), "end rows")
    _same_bits(np.array(g.integrate_dense_parallel(rows, tfs, 3)), np.array(h.integrate_dense_parallel(held, tfs, 3)), "dense rows")
    sa, sb = g.integrate_stm_parallel(rows, tfs), h.integrate_stm_parallel(held, tfs)
    _same_bits(np.array([r[0] for r in sa]), np.array([r[0] for r in sb]), "STM call's rows")
    _same_bits(np.array([r[1] for r in sa]), np.array([r[1] for r in sb]), "STM")
    _same_bits(np.array(make_vanderpol().integrator("DOPRI87", 0.05, [0.3]).integrate(rows[0], tfs[0])), np.array(h.integrate(held[0], tfs[0])), "integrate")


# ---- 3. / 4. problems without a fixture: the float64 restatement of the closed loop at twice its bound
@functools.lru_cache(maxsize=None)
def _problems(oracle, law, m, seed, lengths=(0.05, 0.2), mixed=False):
    system = cck.LAWS[law][0]
    f_c, fj_c = cck.closed_loop_of(oracle, law)
    return _Problems(system, cck.SIZES[system], m, seed, f_c, fj_c, lengths=lengths, mixed=mixed)


def _check_rows(P, law, ids, rows_out, steps, J=None, what=""):
    """states (and the STM) of problems `ids` against the restatement at twice the bound, the controls of the returned rows, the rest
    of the rows"""
    n, uv, _ = cck.SIZES[cck.LAWS[law][0]]
    rows_out = np.asarray(rows_out)
    P.check(ids, rows_out[:, :n], steps, J, what=what)
    st64 = np.array([P.ref(i)["steps"] for i in ids])
    S_max = np.maximum(np.abs(np.array([P.ref(i)["S"] for i in ids])[:, :, :n]), np.eye(n)[None])
    _check_controls(law, rows_out, 2.0 * pck.state_bound(S_max, st64[:, 0], P.opt["abs_tol"]), what, factor=1.0)
    assert np.array_equal(rows_out[:, n], P.tfs[ids]) and np.array_equal(rows_out[:, n + 1 + uv:], P.rows[ids][:, n + 1 + uv:])
    if J is not None:
        assert np.all(J[:, :, n + 1:n + 1 + uv] == 0.0), what + ": the STM's u columns are exactly 0.0"


def test_tangential_thrust_in_a_mixed_wave_with_a_zero_length_arc(oracle):
    """ode.integrator(def_step, Args(3).normalized() * 0.01, [3, 4, 5]) on twobody_lt: 65 problems, both directions, one of length 0"""
    P = _problems(oracle, "tangential", 65, 31, lengths=(0.05, 0.5), mixed=True)
    z = 17
    tfs = P.tfs.copy()
    tfs[z] = P.rows[z, 6]
    assert (tfs > P.rows[:, 6]).any() and (tfs < P.rows[:, 6]).any()
    g = _integrator("tangential", P.opt)
    out, steps, status = g.integrate_parallel(P.rows, tfs, details=True)
    out = np.array(out)
    assert (status == 0).all() and tuple(steps[z]) == (0, 0)
    _same_bits(out[z, :7], P.rows[z, :7], "tf == t0 returns the state and the time")
    pck.compare(out[z, 7:], cck.law_value("tangential", P.rows[z]), np.full(3, 16.0 * U * 0.01), "tf == t0: the controls are the law at the row")
    ids = np.array([i for i in range(0, 65, 4) if i != z])                             # (0, 4, .., 64)
    _check_rows(P, "tangential", ids, out[ids], steps[ids], what="tangential thrust, mixed wave")
    sids = np.array([0, 16, 18, 64])
    srows, J, ssteps, sstatus, last = _stm(g, P.rows[[16, 17, 18, 0, 64]], tfs[[16, 17, 18, 0, 64]])
    assert (sstatus == 0).all() and tuple(ssteps[1]) == (0, 0)
    _same_rows(srows, out[[16, 17, 18, 0, 64]], 6, 3, "STM call's rows against the batch call's")
    _same_bits(last, srows[:, :6], "the last lane of a group against lane 0")
    assert np.array_equal(J[1, :, :6], np.eye(6)) and np.all(J[1, :, 7:10] == 0.0)
    f0 = cck.closed_loop_of(oracle, "tangential")[0](P.rows[z])
    tol = np.full(6, 64.0 * U * np.abs(f0).max())                                      # generated right-hand side against the oracle's
    pck.compare(J[1, :, 10], f0, tol, "tf == t0: d xf / d tf is f(x0) under the law")
    pck.compare(J[1, :, 6], -f0, tol, "tf == t0: d xf / d t0 is -f(x0) under the law")
    order = [3, 0, 2, 4]                                                               # (problems 0, 16, 18, 64 of the call above)
    _check_rows(P, "tangential", sids, srows[order], ssteps[order], J[order], what="tangential thrust, STM")
    dense, dsteps, dstatus = g.integrate_dense_parallel(P.rows[z - 1:z + 2], tfs[z - 1:z + 2], 4, details=True)
    dense = np.array(dense)
    assert (dstatus == 0).all() and tuple(dsteps[1]) == (0, 0)
    _same_bits(dense[1], np.repeat(out[z][None], 4, axis=0), "tf == t0, dense: every sample is the end row, controls included")
    _same_bits(dense[:, 0, :6], P.rows[z - 1:z + 2, :6], "sample 0 is x0")
    pck.compare(dense[:, 0, 7:], cck.law_value("tangential", P.rows[z - 1:z + 2]), np.full((3, 3), 16.0 * U * 0.01), "sample 0: the law at the row")


@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_batch_kernel_workgroup_edges(oracle, m):
    P = _problems(oracle, "pd", 65, 32, lengths=(0.05, 0.3))
    g = _integrator("pd", P.opt)
    out, steps, status = g.integrate_parallel(P.rows[:m], P.tfs[:m], details=True)
    out = np.array(out)
    assert (status == 0).all() and out.shape == (m, 5)
    ids = np.arange(m) if m == 1 else np.array([0, 1, 31, 32, 62] + ([63] if m > 63 else []) + ([64] if m > 64 else []))
    _check_rows(P, "pd", ids, out[ids], steps[ids], what=f"pd x {m}")
    if m == 65:
        r64 = np.array(g.integrate_parallel(P.rows[:64], P.tfs[:64]))
        _same_bits(out[:64], r64, "a problem's result does not depend on the batch around it")


@pytest.mark.parametrize("m", [31, 32, 33])
def test_batch_kernel_with_halved_lanes(oracle, m):
    """shape_11_4_0: 13 stage vectors of 11 states for 64 lanes do not fit the LDS budget, a workgroup runs 32 lanes"""
    from asset_asrl_amd import _lib
    assert _lib.propagate_plan(11, 4, 0, m, False)["lanes"] == 32
    P = _problems(oracle, "shape_11_4_0", 33, 33, lengths=(0.05, 0.12))
    g = _integrator("shape_11_4_0", P.opt)
    out, steps, status = g.integrate_parallel(P.rows[:m], P.tfs[:m], details=True)
    out = np.array(out)
    assert (status == 0).all()
    ids = np.array([0, 30] + ([31] if m > 31 else []) + ([32] if m > 32 else []))
    _check_rows(P, "shape_11_4_0", ids, out[ids], steps[ids], what=f"shape_11_4_0 x {m}")


STM_EDGES = [("shape_5_3_2", 3, 8, 1), ("shape_5_3_2", 9, 8, 1), ("shape_8_3_1", 3, 16, 1), ("shape_8_3_1", 5, 16, 1), ("shape_11_4_0", 3, 16, 1),
             ("coupled16", 3, 16, 2)]


@pytest.mark.parametrize("law,m,group,passes", STM_EDGES, ids=[f"{a}-{b}" for a, b, _, _ in STM_EDGES])
def test_stm_kernel_lane_group_edges(oracle, law, m, group, passes):
    """shape_5_3_2: C' = 7 in groups of 8 (one lane idle), 9 problems overflow a wave of 8 groups; shape_8_3_1: C' = 9 in groups of 16, 5
    problems overflow a wave; shape_11_4_0: C' = 11; coupled16: C' = 18, groups of 16 lanes walk the columns in two passes"""
    from asset_asrl_amd import _lib
    n, uv, pv = cck.SIZES[cck.LAWS[law][0]]
    plan = _lib.propagate_plan(n, 0, pv, m, True)
    assert (plan["group"], plan["passes"], plan["columns"]) == (group, passes, n + pv)
    P = _problems(oracle, law, 9 if law == "shape_5_3_2" else (5 if law == "shape_8_3_1" else 3), 40 + n, lengths=(0.05, 0.12))
    g = _integrator(law, P.opt)
    srows, J, steps, status, last = _stm(g, P.rows[:m], P.tfs[:m])
    assert (status == 0).all()
    out, bsteps, bstatus = g.integrate_parallel(P.rows[:m], P.tfs[:m], details=True)
    _same_rows(srows, np.array(out), n, uv, "integrate_stm_parallel's rows against integrate_parallel's")
    _same_bits(last, srows[:, :n], "the last lane of a group against lane 0")
    assert np.array_equal(steps, bsteps)
    ids = np.arange(m) if m <= 3 else np.array([0, m - 2, m - 1])
    _check_rows(P, law, ids, srows[ids], steps[ids], J[ids], what=f"{law} x {m}")
    # the time columns are the closed forms on the device's own S and xf, the law's controls in f: rounding alone (tests/test_gpu_propagate.py)
    N = n + 1 + uv + pv
    Sdev = np.concatenate([J[:, :, :n], J[:, :, n + 1:N]], axis=2)
    d0, df = pck.time_columns(P.f, P.rows[:m], P.tfs[:m], srows[:, :n], Sdev, dtype=float)
    f0 = np.array([P.f(r) for r in P.rows[:m]])
    fscale = 64.0 * U * np.maximum(np.abs(f0).max(axis=1), np.abs(df).max(axis=1))
    b0 = (np.abs(J[:, :, :n]) * (16.0 * U * np.abs(f0) + fscale[:, None])[:, None, :]).sum(axis=2)
    pck.compare(J[:, :, n], d0, b0, f"{law}: d xf / d t0 is -S_x f(x0) of the device's own S")
    pck.compare(J[:, :, N], df, np.repeat(fscale[:, None], n, axis=1), f"{law}: d xf / d tf is f(xf) of the device's own xf")


# ---- 5. statuses
def test_statuses_do_not_disturb_the_neighbours(oracle):
    """a NaN initial state, a law that is NaN for one problem (sqrt of a negative parameter), and the step cap"""
    from asset_asrl_amd.integrator import IntegrationError
    P = _problems(oracle, "pd_nan", 10, 35, lengths=(0.03, 0.05))
    opt = gck.options(max_steps=12)
    rows, tfs = P.rows.copy(), P.tfs.copy()
    rows[3, 1] = np.nan
    rows[7, 4] = -1.0
    tfs[5] = rows[5, 2] + 20.0
    with np.errstate(all="ignore"):
        ref = [pck.propagate(P.f, P.fj, rows[i], tfs[i], 1, opt) for i in range(10)]
    want = [0, 0, 0, 2, 0, 1, 0, 2, 0, 0]
    assert [r["status"] for r in ref] == want                                          # (the test's own premise)
    good = np.array([0, 1, 2, 4, 6, 8, 9])
    g = _integrator("pd_nan", opt)
    clean = np.array(g.integrate_parallel(rows[good], tfs[good]))
    out, steps, status = g.integrate_parallel(rows, tfs, details=True)                 # (details: statuses, no exception)
    out = np.array(out)
    assert status.tolist() == want
    assert np.isnan(out[[3, 5, 7], :2]).all() and np.isnan(out[[3, 5, 7], 3]).all() and steps[5].sum() == 12 and steps[3].sum() == 0
    _same_bits(out[good], clean, "the other problems of the batch")
    dense, dsteps, dstatus = g.integrate_dense_parallel(rows, tfs, 5, details=True)
    dense = np.array(dense)
    assert dstatus.tolist() == want and np.isnan(dense[5, -1, [0, 1, 3]]).all() and np.isnan(dense[[3, 7], 1:][:, :, [0, 1, 3]]).all()
    _same_bits(dense[5, 0, :2], rows[5, :2], "sample 0 of a problem that fails later is x0")
    assert np.isfinite(dense[5, 0, 3]) and np.isnan(dense[3, 0, 3]) and np.isnan(dense[7, 0, 3])
    assert np.isfinite(dense[good]).all()
    srows, J, ssteps, sstatus, _ = _stm(g, rows, tfs)
    assert sstatus.tolist() == want and np.isnan(srows[[3, 5, 7]][:, [0, 1, 3]]).all() and np.isnan(J[[3, 5, 7]]).all()
    _same_rows(srows[good], clean, 2, 1, "STM call: the other problems of the batch")
    assert np.isfinite(J[good]).all()
    for call in (lambda: g.integrate_parallel(rows, tfs), lambda: g.integrate_dense_parallel(rows, tfs, 5), lambda: g.integrate_stm_parallel(rows, tfs)):
        with pytest.raises(IntegrationError, match="3 of 10 propagations failed; first: problem 3, status 2"):
            call()
