"""Batched propagation with events AND the state-transition matrix on the device (csrc/propagate_event_stm_kernels.h through
asset_hip_propagate_events_stm and ``integrate_events_stm*``).  The state side -- rows, end times, counts, stored occurrences, steps --
is pinned bit for bit to ``integrate_parallel(events)``, and where nothing stops the propagation the Jacobian bit for bit to
``integrate_stm_parallel``: two calls the 50-digit fixtures already hold.  The derivative of a propagation that stops is held to the
closed-form variational flows of tests/event_stm_checker.py at the times the device returned, and where there is no closed form to the
float64 restatement at twice the bounds.  Lane-group edges, the caps, a failed problem, tf == t0, the optional outputs of the C entry
and the public return shapes.  Every module is pre-built (tests/event_stm_cases.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import event_checker as eck
import event_stm_cases as cases
import event_stm_checker as sck
import integ_checker as gck
import propagate_checker as pck
from asset_asrl_amd import _lib

pytestmark = pytest.mark.gpu
U = eck.U
PI = float(np.pi)


def _integrator(system, opt, event_tol=1.0e-6, iters=10, locs=8):
    g = cases.make_ode(system).integrator("DOPRI87", opt["def_step"])
    g.setStepSizes(opt["def_step"], opt["min_step"], opt["max_step"])
    g.MaxStepChange, g.Adaptive, g.MaxSteps = opt["max_step_change"], opt["adaptive"], opt["max_steps"]
    g.setAbsTols(np.broadcast_to(opt["abs_tol"], (g.xv,)))
    g.setRelTols(np.broadcast_to(opt["rel_tol"], (g.xv,)))
    g.EventTol, g.MaxEventIters, g.MaxEventLocs = event_tol, iters, locs
    return g


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


STATE_SIDE = ("t_end", "ev_rows", "ev_resid")
INT_SIDE = ("steps", "status", "stopped", "ev_count", "ev_conv")


def _same_state_side(res, info, res_ev, info_ev, what, event_jacs=False):
    """rows, eventlocs and every array of the events call, bit for bit"""
    assert len(res) == len(res_ev)
    _same_bits(np.array([r[0] for r in res]), np.array([r[0] for r in res_ev]), f"{what}: end rows")
    for k in STATE_SIDE:
        _same_bits(info[k], info_ev[k], f"{what}: {k}")
    for k in INT_SIDE:
        assert np.array_equal(info[k], info_ev[k]), (what, k)
    for r, r_ev in zip(res, res_ev):
        assert len(r[2]) == len(r_ev[1])
        for lj, lj_ev in zip(r[2], r_ev[1]):
            assert len(lj) == len(lj_ev)
            for a, b in zip(lj, lj_ev):
                _same_bits(a[0] if event_jacs else a, b, f"{what}: a located row")


# ---- 1. never stopping: bit for bit the STM call and the events call
def _bitwise_problems(system):
    """the problems of tests/test_gpu_propagate_events.py: the fixture rows forward and backward, one thrusting arc"""
    c = eck.fixture()[1]["vdp_x1" if system == "vanderpol" else "kepler_apsides"]
    rows, tfs = c["rows"].copy(), c["tfs"].copy()
    rows, tfs = np.concatenate([rows, rows]), np.concatenate([tfs, 2.0 * rows[:, eck.SYSTEMS[system]["n"]] - tfs])
    if system == "twobody_lt":
        rows[1, 7:10] = (0.3, -0.2, 0.5)
    return rows, tfs, eck.case_options(c)


@pytest.mark.parametrize("system,fires,never", [("vanderpol", "x1", "pos"), ("twobody_lt", "rv", "pos")])
def test_never_stopping_is_bitwise_the_stm_call_and_the_events_call(system, fires, never):
    rows, tfs, opt = _bitwise_problems(system)
    g = _integrator(system, opt)
    stm, steps, status, _ = g.integrate_stm_parallel(rows, tfs, details=True)
    assert (status == 0).all()
    for ev, want in ((fires, True), (never, False)):
        events = cases.events_of(system, (ev,), (0,), (0,))
        res_ev, info_ev = g.integrate_parallel(rows, tfs, events, details=True)
        res, info = g.integrate_events_stm_parallel(rows, tfs, events, details=True)
        assert (info["ev_count"].sum() > 0) == want and (info["stopped"] == -1).all()
        _same_bits(np.array([r[0] for r in res]), np.array([r[0] for r in stm]), f"{system}, '{ev}': rows against integrate_stm_parallel")
        _same_bits(np.array([r[1] for r in res]), np.array([r[1] for r in stm]), f"{system}, '{ev}': J against integrate_stm_parallel")
        _same_bits(info["jac"], np.array([r[1] for r in stm]), "info['jac']")
        assert np.array_equal(info["steps"], steps) and np.array_equal(info["status"], status)
        _same_state_side(res, info, res_ev, info_ev, f"{system}, '{ev}'")


# ---- 2. stopping: the state side bit for bit
STOPPING = [n for n in eck.case_names() if (eck.fixture()[1][n]["stopped"] >= 0).any()]


def _case_run(case, stm, **kw):
    g = _integrator(case["system"], eck.case_options(case), case["event_tol"], 10, case["max_locs"])
    ev = cases.events_of(case["system"], case["events"], case["direction"], case["stop"])
    if stm:
        return g.integrate_events_stm_parallel(case["rows"], case["tfs"], ev, details=True, **kw)
    return g.integrate_parallel(case["rows"], case["tfs"], ev, details=True)


@pytest.mark.parametrize("name", STOPPING)
def test_stopping_cases_have_the_state_side_of_the_events_call(name):
    assert {"osc_up_stop1", "osc_down_stop3", "fall_impact"} <= set(STOPPING)
    case = eck.fixture()[1][name]
    res_ev, info_ev = _case_run(case, False)
    res, info = _case_run(case, True)
    assert (info["status"] == 0).all() and (info["stopped"] >= 0).all()
    _same_state_side(res, info, res_ev, info_ev, name)
    assert np.isfinite(info["jac"]).all()


# ---- 3. stopping: the derivative
@functools.lru_cache(maxsize=None)
def _closed_bounds(name):
    case = eck.fixture()[1][name]
    return sck.eS_closed(case)[0], eck.state_bounds(case, case["accepted64"])


@pytest.mark.parametrize("name", [n for n in eck.case_names() if eck.fixture()[1][n]["system"] in sck.CLOSED])
def test_jacobians_meet_the_closed_form_variational_flows_at_the_returned_times(name):
    case = eck.fixture()[1][name]
    n = eck.SYSTEMS[case["system"]]["n"]
    eS, B = _closed_bounds(name)
    res, info = _case_run(case, True, event_jacs=True)
    assert (info["status"] == 0).all()
    worst, located = 0.0, 0
    for i, (row, J, locs) in enumerate(res):
        worst = max(worst, sck.compare_item_closed(case["system"], case["rows"][i], row[n], row[:n], J, eS[i], B[i], f"{name} problem {i}, end"))
        for j, lj in enumerate(locs):
            assert len(lj) == min(info["ev_count"][i, j], case["max_locs"])
            for k, (lrow, Jl) in enumerate(lj):
                located += 1
                _same_bits(Jl, info["ev_jac"][i, j, k], "J_loc is the slot of info['ev_jac']")
                worst = max(worst, sck.compare_item_closed(case["system"], case["rows"][i], lrow[n], lrow[:n], Jl, eS[i], B[i],
                                                           f"{name} problem {i}, event {j} occurrence {k}"))
    assert located > 0
    used = np.arange(case["max_locs"])[None, None, :] < info["ev_count"][:, :, None]
    assert np.isnan(info["ev_jac"][~used]).all() and np.isfinite(info["ev_jac"][used]).all()
    print(f"{name}: {located} located occurrences, worst ratio {worst:.3g}, eS {eS}")


def _fj_of(f, J):
    return lambda y: (f(y), J(y))


def _check_against_restatement(case, res, info, f, Jfun, what, sysd=None):
    """every item of every problem against the float64 restatement, at twice the bounds (tests/event_stm_checker.py)"""
    n = (sysd or eck.SYSTEMS[case["system"]])["n"]
    ref = sck.restate_case(case, J=Jfun, sysd=sysd)
    opt = eck.case_options(case)
    worst = 0.0
    for i, (r, (row, J, locs)) in enumerate(zip(ref, res)):
        assert r["status"] == 0 and info["status"][i] == 0
        assert list(info["ev_count"][i]) == r["count"] and info["stopped"][i] == r["stopped"], (what, i)
        eS, dS = sck.eS_estimated(f, _fj_of(f, Jfun), case["rows"][i], r["t_end"], opt)
        S_max = np.maximum(np.abs(np.asarray(r["S"], dtype=float)[:, :n]), np.eye(n))
        B = pck.state_bound(S_max[None], np.array([r["steps"][0] + 1]), opt["abs_tol"])[0]
        items = sck.items_of(r)
        eS = max(eS, sck.eS_items(f, _fj_of(f, Jfun), case["rows"][i], items, opt))
        got = [(row[n], J)] + [(lrow[n], Jl) for lj in locs for lrow, Jl in lj]
        assert len(got) == len(items), (what, i)
        for k, (a, b) in enumerate(zip(items, got)):
            print(f"{what} problem {i} item {k}: t_device - t_restated = {float(b[0]) - float(a[0]):.3e}")
            shift = sck.time_shift(f, _fj_of(f, Jfun), case["rows"][i], a[0], b[0], opt)
            worst = max(worst, sck.compare_item_restated(f, Jfun, case["rows"][i], n, a, b, eS, dS.max(), B, f"{what} problem {i} item {k}", shift))
    print(f"{what}: worst ratio {worst:.3g}")
    return ref


def test_twobody_stop_2_against_the_restatement():
    case = eck.fixture()[1]["kepler_backward"]
    assert case["events"] == ["rv"] and case["stop"] == [2]
    res_ev, info_ev = _case_run(case, False)
    res, info = _case_run(case, True, event_jacs=True)
    _same_state_side(res, info, res_ev, info_ev, "kepler_backward", event_jacs=True)
    f = eck.SYSTEMS["twobody_lt"]["f"]
    _check_against_restatement(case, res, info, f, sck.jacobian_of("twobody_lt"), "twobody_lt, rv, stop 2")


# ---- 4. lane-group edges
def _kepler_row(offset, e=0.3):
    """the state of the orbit a = 1 (period 2 pi) at `offset` past its periapsis, which it passes at t = 0; no thrust"""
    peri = np.array([1.0 - e, 0.0, 0.0, 0.0, np.sqrt((1.0 + e) / (1.0 - e)), 0.0, 0.0, 0.0, 0.0, 0.0])
    x = eck.exact_flow("twobody_lt", peri, offset).astype(float)
    return np.concatenate([x, [offset, 0.0, 0.0, 0.0]])


def test_lane_groups_of_16_four_problems_per_workgroup():
    """twobody_lt, C = 9 in groups of 16: five problems, so the last workgroup holds one.  Event 0 is r.v in any direction and never
    stops, event 1 is r.v upward (a periapsis passage) and stops at its first occurrence."""
    plan = _lib.propagate_plan(6, 3, 0, 5, True)
    assert (plan["group"], plan["lanes"], plan["problems_per_wg"], plan["passes"], plan["grid"]) == (16, 64, 4, 1, 2)
    rows = np.array([_kepler_row(-0.02), _kepler_row(0.3), _kepler_row(0.2), _kepler_row(0.25, 0.2), _kepler_row(1.0, 0.1)])
    tfs = rows[:, 6] + np.array([3.0, 1.5, 8.0, -5.0, 2.5])
    rows[1, 7:10] = (0.2, -0.1, 0.3)                                                   # (a thrusting arc among them)
    opt = gck.options(def_step=0.1, min_step=1.0e-5, max_step=0.75)
    case = dict(name="lane groups of 16", system="twobody_lt", events=["rv", "rv"], direction=[0, 1], stop=[0, 1], rows=rows, tfs=tfs,
                options={k: opt[k] for k in ("def_step", "min_step", "max_step", "max_step_change", "adaptive", "max_steps", "abs_tol", "rel_tol")},
                event_tol=1.0e-6, max_locs=8)
    res_ev, info_ev = _case_run(case, False)
    res, info = _case_run(case, True, event_jacs=True)
    _same_state_side(res, info, res_ev, info_ev, "lane groups of 16", event_jacs=True)
    f = eck.SYSTEMS["twobody_lt"]["f"]
    ref = _check_against_restatement(case, res, info, f, sck.jacobian_of("twobody_lt"), "lane groups of 16")
    # the test's own premise, on the restatement
    assert ref[0]["stopped"] == 1 and ref[0]["steps"][0] == 1, "stops in its first accepted step"
    assert ref[1]["count"] == [0, 0] and ref[1]["stopped"] == -1, "never fires"
    assert sum(len(lj) for lj in ref[2]["locs"]) >= 3, "locates several occurrences"
    assert tfs[3] < rows[3, 6] and sum(ref[3]["count"]) >= 1, "backward, with an occurrence"
    assert info["steps"][0, 0] == 1


@functools.lru_cache(maxsize=None)
def _shape_case():
    """three arcs of shape_11_4_2 about the level x0 = 0.25 (tests/test_gpu_propagate_events.py: _shape_problems), stop at the first"""
    rng = np.random.default_rng(5)
    rows, tfs = [], []
    for i in range(3):
        row = np.concatenate([rng.uniform(-0.6, 0.6, 11), [0.1 * i], rng.uniform(-1, 1, 4), rng.uniform(-0.5, 0.5, 2)])
        row[0] = eck.SHAPE_LEVEL + (0.03 if i % 2 else -0.03)
        rows.append(row)
        tfs.append(row[11] + (1.5 if i % 3 else -1.5))
    opt = gck.options(def_step=0.05, max_step=0.25)
    return dict(name="shape", system="shape_11_4_2", events=["x0c"], direction=[0], stop=[1], rows=np.array(rows), tfs=np.array(tfs),
                options={k: opt[k] for k in ("def_step", "min_step", "max_step", "max_step_change", "adaptive", "max_steps", "abs_tol", "rel_tol")},
                event_tol=1.0e-6, max_locs=8)


def test_lane_group_of_32_one_problem_per_workgroup():
    """shape_11_4_2: C = 17 takes a group of 32 lanes, the whole 32-lane workgroup; x0 - 0.25 with stop = 1 against the restatement"""
    plan = _lib.propagate_plan(11, 4, 2, 3, True)
    assert (plan["columns"], plan["group"], plan["lanes"], plan["problems_per_wg"], plan["passes"], plan["grid"]) == (17, 32, 32, 1, 1, 3)
    case = _shape_case()
    res_ev, info_ev = _case_run(case, False)
    res, info = _case_run(case, True, event_jacs=True)
    _same_state_side(res, info, res_ev, info_ev, "shape_11_4_2", event_jacs=True)
    f = eck.SYSTEMS["shape_11_4_2"]["f"]
    ref = _check_against_restatement(case, res, info, f, sck.jacobian_of("shape_11_4_2"), "shape_11_4_2, x0c, stop 1")
    assert sorted(r["stopped"] for r in ref) == [-1, 0, 0], "two of the three stop"


def test_four_column_passes_of_groups_of_8(oracle):
    """synthetic32: groups of 8 lanes walk 32 columns in 4 passes; S and ev_S columns of every pass against the restatement"""
    plan = _lib.propagate_plan(32, 0, 0, 2, True)
    assert (plan["group"], plan["lanes"], plan["passes"], plan["problems_per_wg"], plan["grid"]) == (8, 8, 4, 1, 2)
    from asset_asrl_amd import synth
    f, fj = pck.oracle_f(oracle, "synthetic32"), pck.oracle_fj(oracle, "synthetic32")
    rows = synth.make_traj("synthetic32", "LGL3", 2, seed=82, T=1.0)[:2].copy()
    rows[:, 0] = (-0.01, -0.03)                                                        # x0 rises through the level 0 early in the arc
    tfs = rows[:, 32] + 0.1
    opt = gck.options()
    sysd = dict(n=32, uv=0, pv=0, f=f, events={"x0c": (lambda y: y[0] - y.dtype.type(cases.SYNTH_LEVEL), None)})
    case = dict(name="synthetic32", system="synthetic32", events=["x0c"], direction=[0], stop=[1], rows=rows, tfs=tfs,
                options={k: opt[k] for k in ("def_step", "min_step", "max_step", "max_step_change", "adaptive", "max_steps", "abs_tol", "rel_tol")},
                event_tol=1.0e-6, max_locs=8)
    res_ev, info_ev = _case_run(case, False)
    res, info = _case_run(case, True, event_jacs=True)
    _same_state_side(res, info, res_ev, info_ev, "synthetic32", event_jacs=True)
    ref = _check_against_restatement(case, res, info, f, lambda y: fj(y)[1], "synthetic32, four passes", sysd=sysd)
    assert [r["stopped"] for r in ref] == [0, 0] and [r["count"] for r in ref] == [[1], [1]]
    assert np.isfinite(info["ev_jac"][:, 0, 0]).all() and np.isnan(info["ev_jac"][:, 0, 1:]).all()


# ---- 5. caps
def _osc_case(rows, tfs, direction=(0,), stop=(0,), event_tol=1.0e-6, locs=8, **o):
    opt = gck.options(**dict(dict(def_step=0.1, min_step=1.0e-5, max_step=1.0), **o))
    return dict(name="oscillator", system="oscillator", events=["x0"], direction=list(direction), stop=list(stop), rows=np.array(rows, dtype=float),
                tfs=np.array(tfs, dtype=float), event_tol=event_tol, max_locs=locs,
                options={k: opt[k] for k in ("def_step", "min_step", "max_step", "max_step_change", "adaptive", "max_steps", "abs_tol", "rel_tol")})


def test_occurrences_beyond_max_event_locs_are_counted_and_their_slots_absent():
    case = _osc_case([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [16.0, 3.0], locs=2)          # crossings at pi / 2 + k pi: five, and one
    res_ev, info_ev = _case_run(case, False)
    res, info = _case_run(case, True, event_jacs=True)
    _same_state_side(res, info, res_ev, info_ev, "MaxEventLocs = 2", event_jacs=True)
    assert info["ev_count"].ravel().tolist() == [5, 1] and (info["stopped"] == -1).all() and (info["status"] == 0).all()
    assert [len(r[2][0]) for r in res] == [2, 1] and info["ev_jac"].shape == (2, 1, 2, 2, 4)
    assert all(np.isfinite(Jl).all() for r in res for _, Jl in r[2][0]) and np.isnan(info["ev_jac"][1, 0, 1]).all()
    eS = sck.eS_closed(case)[0]
    B = pck.state_bound(np.ones((2, 2, 2)), info["steps"][:, 0] + 1, 1.0e-12)          # (|d x(t) / d x0| <= 1: a rotation)
    for i, (row, J, locs) in enumerate(res):
        for lrow, Jl in [(row, J)] + locs[0]:
            sck.compare_item_closed("oscillator", case["rows"][i], lrow[2], lrow[:2], Jl, eS[i], B[i], f"MaxEventLocs = 2, problem {i}")


def test_an_occurrence_that_uses_up_its_evaluations_keeps_the_trial_points_matrix():
    case = _osc_case([[1.0, 0.0, 0.0], [2.0, 0.0, 0.0]], [6.0, 6.0], event_tol=1.0e-14)
    g = _integrator("oscillator", eck.case_options(case), event_tol=1.0e-14, iters=1)
    ev = cases.events_of("oscillator", ("x0",), (0,), (0,))
    res_ev, info_ev = g.integrate_parallel(case["rows"], case["tfs"], ev, details=True)
    res, info = g.integrate_events_stm_parallel(case["rows"], case["tfs"], ev, event_jacs=True, details=True)
    _same_state_side(res, info, res_ev, info_ev, "MaxEventIters = 1", event_jacs=True)
    assert info["ev_count"].ravel().tolist() == [2, 2] and (info["ev_conv"][:, 0, :2] == 0).all()
    assert all(r[2] == [[]] for r in res), "dropped from eventlocs"
    # the stored state is one theta h step from the bracket's start, whatever theta was: its matrix is the variational flow at the
    # time that was stored
    eS = sck.eS_closed(case)[0]
    B = pck.state_bound(np.ones((2, 2, 2)), info["steps"][:, 0] + 1, 1.0e-12)
    for i in range(2):
        for k in range(2):
            stored = info["ev_rows"][i, 0, k]
            sck.compare_item_closed("oscillator", case["rows"][i], stored[2], stored[:2], info["ev_jac"][i, 0, k], eS[i], B[i],
                                    f"MaxEventIters = 1, problem {i} occurrence {k}")


# ---- 6. status and optional outputs
def test_a_problem_that_runs_out_of_steps_keeps_its_occurrences_and_leaves_the_others_alone():
    case = _osc_case([[1.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.5, 0.0, 0.0]], [3.0, 60.0, 3.0], max_steps=40)
    ref = eck.restate_case(case)
    assert [r["status"] for r in ref] == [0, 1, 0] and ref[1]["count"][0] >= 2           # (the test's own premise)
    res, info = _case_run(case, True, event_jacs=True)
    assert info["status"].tolist() == [0, 1, 0] and info["steps"][1].sum() == 40
    row, J, locs = res[1]
    assert np.isnan(row[:2]).all() and np.isnan(J).all() and np.isnan(info["ev_jac"][1]).all()
    used = min(int(info["ev_count"][1, 0]), 8)
    assert used >= 2 and np.isfinite(info["ev_rows"][1, 0, :used]).all() and (info["ev_conv"][1, 0, :used] == 1).all()
    assert len(locs[0]) == used
    res_ev, info_ev = _case_run(case, False)
    _same_state_side(res, info, res_ev, info_ev, "a failed problem", event_jacs=True)
    alone = dict(case, rows=case["rows"][[0, 2]], tfs=case["tfs"][[0, 2]])
    res2, info2 = _case_run(alone, True, event_jacs=True)
    _same_bits(np.array([r[1] for r in res2]), np.array([res[0][1], res[2][1]]), "J of the other two problems")
    _same_bits(info2["ev_jac"], info["ev_jac"][[0, 2]], "ev_jac of the other two problems")
    from asset_asrl_amd.integrator import IntegrationError
    with pytest.raises(IntegrationError, match="1 of 3 propagations failed; first: problem 1, status 1"):
        _integrator("oscillator", eck.case_options(case)).integrate_events_stm_parallel(case["rows"], case["tfs"],
                                                                                        cases.events_of("oscillator", ("x0",), (0,), (0,)))


def test_a_problem_that_does_not_move():
    case = eck.fixture()[1]["fall_impact"]
    rows, tfs = case["rows"][:3].copy(), case["tfs"][:3].copy()
    tfs[1] = rows[1, 2]
    res, info = _case_run(dict(case, rows=rows, tfs=tfs), True, event_jacs=True)
    row, J, locs = res[1]
    _same_bits(row, rows[1], "tf == t0 returns the row")
    assert tuple(info["steps"][1]) == (0, 0) and info["ev_count"][1, 0] == 0 and info["stopped"][1] == -1 and locs == [[]]
    assert np.array_equal(J[:, :2], np.eye(2)) and np.all(J[:, 3] == 0.0), "S: the identity in its x columns, zero elsewhere"
    f0 = np.array([rows[1, 1], -rows[1, 3]])
    assert np.array_equal(J[:, 4], f0) and np.array_equal(J[:, 2], -f0), "the time columns: f(x0) and -f(x0)"
    assert np.isnan(info["ev_jac"][1]).all() and np.isnan(info["ev_rows"][1]).all()
    assert info["stopped"][0] == 0 and info["stopped"][2] == 0, "its neighbours stop as they do without it"


def test_optional_outputs_of_the_c_entry_change_no_bit():
    from asset_asrl_amd import jit
    case = eck.fixture()[1]["osc_down_stop3"]
    module = jit.ensure_event_stm_module(cases.make_ode("oscillator"), [cases.event_function("oscillator", "x0")], compile_only=False)
    rows, tfs = np.ascontiguousarray(case["rows"]), np.ascontiguousarray(case["tfs"])
    m, n, N, ne, K = rows.shape[0], 2, 3, 1, 4
    o = eck.case_options(case)
    tols = np.concatenate([np.broadcast_to(o["abs_tol"], (n,)), np.broadcast_to(o["rel_tol"], (n,))]).astype(float)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    opt = _lib.IntegOptions(o["def_step"], o["min_step"], o["max_step"], o["max_step_change"], int(o["adaptive"]), o["max_steps"],
                            tols[:n].ctypes.data_as(dp), tols[n:].ctypes.data_as(dp))
    d, s = np.array([-1], dtype=np.int32), np.array([3], dtype=np.int32)

    def call(optional):
        out = dict(xf=np.full((m, n), -7.0), jac=np.full((m, n, N + 1), -7.0), t_end=np.full(m, -7.0), stopped=np.full(m, -7, dtype=np.int32),
                   ev_count=np.full((m, ne), -7, dtype=np.int32), ev_rows=np.full((m, ne, K, n + 1), -7.0), ev_resid=np.full((m, ne, K), -7.0),
                   ev_conv=np.full((m, ne, K), -7, dtype=np.int32), ev_jac=np.full((m, ne, K, n, N + 1), -7.0),
                   steps=np.full((m, 2), -7, dtype=np.int32), status=np.full(m, -7, dtype=np.int32))
        a = {k: (v.ctypes.data_as(dp if v.dtype == np.float64 else ip) if optional or k not in ("ev_jac", "steps", "status") else None)
             for k, v in out.items()}
        rc = _lib.lib().asset_hip_propagate_events_stm(module.encode(), rows.ctypes.data_as(dp), m, tfs.ctypes.data_as(dp), C.byref(opt), ne,
                                                       d.ctypes.data_as(ip), s.ctypes.data_as(ip), 1.0e-6, 10, K, a["xf"], a["jac"], a["t_end"],
                                                       a["stopped"], a["ev_count"], a["ev_rows"], a["ev_resid"], a["ev_conv"], a["ev_jac"],
                                                       a["steps"], a["status"], 0)
        assert rc == 0, _lib.lib().asset_hip_last_error().decode()
        return out
    full, bare = call(True), call(False)
    for k in ("xf", "jac", "t_end", "ev_rows", "ev_resid"):
        _same_bits(bare[k], full[k], k)
    for k in ("stopped", "ev_count", "ev_conv"):
        assert np.array_equal(bare[k], full[k]), k
    assert all((bare[k] == -7).all() for k in ("ev_jac", "steps", "status")) and not (full["ev_jac"] == -7).any()
    assert (full["status"] == 0).all() and (full["stopped"] == 0).all() and (full["ev_count"] == 3).all()


# ---- 7. public return shapes
def test_public_return_shapes():
    c = eck.fixture()[1]["vdp_x1"]
    rows, tfs = c["rows"], c["tfs"]
    g = _integrator("vanderpol", eck.case_options(c))
    ev = cases.events_of("vanderpol", ("x1",), (0,), (0,))
    n, N, m = 2, 5, rows.shape[0]

    def check_row(r, i):
        assert r.shape == (N,) and np.array_equal(r[n + 1:], rows[i, n + 1:]), "the control and parameter columns are the input row's"

    def check_triple(t, i, jacs):
        row, J, locs = t
        check_row(row, i)
        assert J.shape == (n, N + 1) and len(locs) == 1 and len(locs[0]) > 0
        for e in locs[0]:
            if jacs:
                assert isinstance(e, tuple) and len(e) == 2 and e[1].shape == (n, N + 1)
                check_row(e[0], i)
            else:
                check_row(e, i)
    for jacs in (False, True):
        res = g.integrate_events_stm_parallel(rows, tfs, ev, event_jacs=jacs)
        assert isinstance(res, list) and len(res) == m
        for i, t in enumerate(res):
            assert isinstance(t, tuple) and len(t) == 3
            check_triple(t, i, jacs)
        res2, info = g.integrate_events_stm_parallel(rows, tfs, ev, threads=4, event_jacs=jacs, details=True)
        assert set(info) == {"steps", "status", "stopped", "t_end", "ev_count", "ev_rows", "ev_resid", "ev_conv", "jac"} | ({"ev_jac"} if jacs else set())
        assert info["jac"].shape == (m, n, N + 1) and (not jacs or info["ev_jac"].shape == (m, 1, 8, n, N + 1))
        _same_bits(np.array([t[0] for t in res2]), np.array([t[0] for t in res]), "details changes no row")
        one = g.integrate_events_stm(rows[1], tfs[1], ev, event_jacs=jacs)
        assert isinstance(one, tuple) and len(one) == 3
        check_triple(one, 1, jacs)
        _same_bits(one[0], res[1][0], "the single call is the batch of one")
        _same_bits(one[1], res[1][1], "the single call's J")
        row, J, locs, inf = g.integrate_events_stm(rows[1], tfs[1], ev, event_jacs=jacs, details=True)
        check_triple((row, J, locs), 1, jacs)
        assert inf["jac"].shape == (n, N + 1) and inf["steps"].shape == (2,) and int(inf["status"]) == 0
