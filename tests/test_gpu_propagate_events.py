"""Batched propagation with events on the device (csrc/propagate_event_kernels.h through asset_hip_propagate_events and
``ode.integrator``): every case of the 50-digit fixture tests/golden/propagate_events/events.npz within the bounds of
tests/event_checker.py; bitwise equality of end states and step counts with the call without events; the workgroup edges of a shape
whose plan has 32 lanes; one wave that mixes everything a lane can do; several events in one step; the cap on stored occurrences;
occurrences that are not located within MaxEventIters.  Where there is no fixture the reference is the float64 restatement, at twice the
bounds (each side is within its bound of the exact value).  Every event module is pre-built (tests/event_cases.py)."""
import functools

import numpy as np
import pytest

import event_cases
import event_checker as eck
import integ_checker as gck

pytestmark = pytest.mark.gpu
U = eck.U
PI = float(np.pi)


def _integrator(system, opt, event_tol=1.0e-6, iters=10, locs=8):
    g = event_cases.make_ode(system).integrator("DOPRI87", opt["def_step"])
    g.setStepSizes(opt["def_step"], opt["min_step"], opt["max_step"])
    g.MaxStepChange, g.Adaptive, g.MaxSteps = opt["max_step_change"], opt["adaptive"], opt["max_steps"]
    g.setAbsTols(np.broadcast_to(opt["abs_tol"], (g.xv,)))
    g.setRelTols(np.broadcast_to(opt["rel_tol"], (g.xv,)))
    g.EventTol, g.MaxEventIters, g.MaxEventLocs = event_tol, iters, locs
    return g


def _run_case(case, rows=None, tfs=None, iters=10):
    g = _integrator(case["system"], eck.case_options(case), case["event_tol"], iters, case["max_locs"])
    ev = event_cases.events_of(case["system"], case["events"], case["direction"], case["stop"])
    return g.integrate_parallel(case["rows"] if rows is None else rows, case["tfs"] if tfs is None else tfs, ev, details=True)


def _as_got(res, info, n):
    return [dict(x=row[:n], t_end=row[n], stopped=info["stopped"][i], count=info["ev_count"][i],
                 locs=[[dict(x=r[:n], t=r[n]) for r in lj] for lj in locs]) for i, (row, locs) in enumerate(res)]


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def _check_shapes(case, res, info):
    rows, n = case["rows"], eck.SYSTEMS[case["system"]]["n"]
    m, ne, K = rows.shape[0], len(case["events"]), case["max_locs"]
    assert len(res) == m and info["ev_rows"].shape == (m, ne, K, n + 1) and info["ev_conv"].shape == (m, ne, K)
    for i, (row, locs) in enumerate(res):
        assert np.array_equal(row[n + 1:], rows[i, n + 1:]) and len(locs) == ne
        for j in range(ne):
            used = min(int(info["ev_count"][i, j]), K)
            assert np.isnan(info["ev_rows"][i, j, used:]).all() and np.isnan(info["ev_resid"][i, j, used:]).all()
            assert (info["ev_conv"][i, j, used:] == 0).all() and np.isfinite(info["ev_rows"][i, j, :used]).all()
            for r in locs[j]:
                assert np.array_equal(r[n + 1:], rows[i, n + 1:])


# ---- the fixture
@pytest.mark.parametrize("name", eck.case_names())
def test_device_matches_the_50_digit_fixture(name):
    case = eck.fixture()[1][name]
    n = eck.SYSTEMS[case["system"]]["n"]
    res, info = _run_case(case)
    assert (info["status"] == 0).all(), info["status"]
    _check_shapes(case, res, info)
    used = np.arange(case["max_locs"])[None, None, :] < info["ev_count"][:, :, None]
    assert (info["ev_conv"][used] == 1).all() and (np.abs(info["ev_resid"][used]) < 1.0).all()
    B = eck.state_bounds(case, case["accepted64"])
    eck.compare_case(case, _as_got(res, info, n), B, what="device:")
    acc, ref = int(info["steps"][:, 0].sum()), int(case["accepted64"].sum())
    print(f"{name}: accepted steps {acc} against the restatement's {ref}")
    assert abs(acc - ref) <= max(2, ref // 10)
    # the plain return: the same rows, and an exception-free call
    plain = _integrator(case["system"], eck.case_options(case), case["event_tol"], 10, case["max_locs"]).integrate_parallel(
        case["rows"], case["tfs"], events=event_cases.events_of(case["system"], case["events"], case["direction"], case["stop"]))
    _same_bits(np.array([r[0] for r in plain]), np.array([r[0] for r in res]), "the plain return against details=True")


# ---- locating does not disturb the propagation
def _bitwise_problems(system):
    c = eck.fixture()[1]["vdp_x1" if system == "vanderpol" else "kepler_apsides"]
    rows, tfs = c["rows"].copy(), c["tfs"].copy()
    rows, tfs = np.concatenate([rows, rows]), np.concatenate([tfs, 2.0 * rows[:, eck.SYSTEMS[system]["n"]] - tfs])   # (and backward)
    if system == "twobody_lt":
        rows[1, 7:10] = (0.3, -0.2, 0.5)                                               # a thrusting arc too
    return rows, tfs, eck.case_options(c)


@pytest.mark.parametrize("system,fires,never", [("vanderpol", "x1", "pos"), ("twobody_lt", "rv", "pos")])
def test_end_states_and_steps_are_bitwise_those_of_the_call_without_events(system, fires, never):
    """a run-time ODE and a library ODE (whose functor is regenerated for the event module)"""
    rows, tfs, opt = _bitwise_problems(system)
    g = _integrator(system, opt)
    end, steps, status = g.integrate_parallel(rows, tfs, details=True)
    assert (status == 0).all()
    n = g.xv
    for ev, want in ((never, False), (fires, True)):
        res, info = g.integrate_parallel(rows, tfs, event_cases.events_of(system, (ev,), (0,), (0,)), details=True)
        assert (info["status"] == 0).all() and (info["stopped"] == -1).all()
        assert (info["ev_count"].sum() > 0) == want, (ev, info["ev_count"].ravel())
        _same_bits(np.array([r[0] for r in res]), np.array(end), f"{system}: end rows with the event '{ev}' (stop = 0)")
        assert np.array_equal(info["steps"], steps), (system, ev)
        assert all(len(r[1][0]) == info["ev_count"][i, 0] for i, r in enumerate(res))
    assert n == eck.SYSTEMS[system]["n"]


# ---- workgroup edges of a shape whose plan has 32 lanes
def _complex_step_jacobian(f):
    def fj(y):
        y = np.asarray(y, dtype=float)
        J = np.zeros((f(y).size, y.size))
        for i in range(y.size):
            z = y.astype(complex)
            z[i] += 1.0e-30j
            J[:, i] = f(z).imag / 1.0e-30
        return f(y), J
    return fj


@functools.lru_cache(maxsize=None)
def _shape_problems():
    """eight arcs of shape_11_4_2 about the level x0 = 0.25, forward and backward; five of them cross it.  (case, B) of the restatement."""
    import propagate_checker as pck
    from asset_asrl_amd import _lib
    assert _lib.propagate_plan(11, 4, 2, 65, False)["lanes"] == 32                      # 13 . 11 . 8 . 64 bytes exceed 48 KB
    rng = np.random.default_rng(5)
    rows, tfs = [], []
    for i in range(8):
        row = np.concatenate([rng.uniform(-0.6, 0.6, 11), [0.1 * i], rng.uniform(-1, 1, 4), rng.uniform(-0.5, 0.5, 2)])
        row[0] = eck.SHAPE_LEVEL + (0.03 if i % 2 else -0.03)
        rows.append(row)
        tfs.append(row[11] + (1.5 if i % 3 else -1.5))
    rows, tfs = np.array(rows), np.array(tfs)
    opt = gck.options(def_step=0.05, max_step=0.25)
    f = eck.SYSTEMS["shape_11_4_2"]["f"]
    fj = _complex_step_jacobian(f)
    S = np.array([pck.propagate(f, fj, r, t, 1, opt, stm=True)["S"][:, :11] for r, t in zip(rows, tfs)])
    S_max = np.maximum(np.abs(S), np.eye(11)[None])                                    # (tests/test_gpu_propagate.py: _Problems.check)
    case, B = eck.case_from_restatement("shape edges", "shape_11_4_2", ("x0c",), (0,), (0,), rows, tfs, opt, 1.0e-6, 8, S_max)
    assert case["count"].ravel().tolist() == [1, 1, 0, 0, 0, 1, 1, 1]                   # (the test's own premise)
    return case, B


@pytest.mark.parametrize("m", [1, 31, 32, 33, 65])
def test_workgroup_edges_of_a_32_lane_plan(m):
    case, B = _shape_problems()
    ids = np.arange(m) % 8
    sub = dict(case, **{k: case[k][ids] for k in eck.ARRAYS if k in case and k != "gddot"})
    res, info = _run_case(sub)
    assert (info["status"] == 0).all()
    _check_shapes(sub, res, info)
    eck.compare_case(sub, _as_got(res, info, 11), B[ids], factor=2.0, what=f"device, m = {m}:")
    for i in range(8, m):                                                              # the same problem in another lane or workgroup
        _same_bits(res[i][0], res[i % 8][0], f"problem {i} against problem {i % 8}")


# ---- one wave that mixes everything
def test_one_wave_of_64_mixed_lanes():
    osc = lambda A, t0: [A * np.cos(t0), -A * np.sin(t0), t0]
    rows, tfs, kind = [], [], []
    for i in range(64):
        A = 0.5 + 0.05 * i
        k = ("none", "first", "late", "backward", "zero", "late", "first", "none")[i % 8]
        t0 = {"none": 0.1 * (i % 5), "first": PI / 2 - 0.01 - 0.001 * i, "late": PI / 2 + 0.05 + 0.01 * i, "backward": 0.02 * i, "zero": 1.0}[k]
        H = {"none": 0.5, "first": 5.0, "late": 6.0, "backward": -3.0, "zero": 0.0}[k]
        rows.append(osc(A, t0)), tfs.append(t0 + H), kind.append(k)
    rows, tfs = np.array(rows), np.array(tfs)
    NAN, CAP = 21, 42
    rows[NAN, 1] = np.nan
    rows[CAP], tfs[CAP] = [0.0, 0.0, 0.0], 100.0                                       # g = 0 for good: no event, a step of 1 at the most
    kind[NAN], kind[CAP] = "nan", "cap"
    opt = gck.options(def_step=0.1, min_step=1.0e-5, max_step=1.0, max_steps=40)
    good = np.array([i for i in range(64) if kind[i] not in ("nan", "cap")])
    case, B = eck.case_from_restatement("mixed wave", "oscillator", ("x0",), (0,), (1,), rows[good], tfs[good], opt, 1.0e-6, 8,
                                        np.ones((good.size, 2, 2)))                     # (|d x(t) / d x0| <= 1: a rotation)
    st = {k: case["stopped"][[kind[i] == k for i in good]] for k in ("none", "first", "late", "backward", "zero")}
    assert (st["none"] == -1).all() and (st["zero"] == -1).all() and all((st[k] == 0).all() for k in ("first", "late", "backward"))
    g = _integrator("oscillator", opt)
    ev = event_cases.events_of("oscillator", ("x0",), (0,), (1,))
    res, info = g.integrate_parallel(rows, tfs, ev, details=True)
    assert info["status"].tolist() == [2 if k == "nan" else (1 if k == "cap" else 0) for k in kind]
    assert np.isnan(res[NAN][0][:2]).all() and np.isnan(res[CAP][0][:2]).all()
    assert info["steps"][NAN].sum() == 0 and info["steps"][CAP].sum() == 40 and (info["ev_count"][[NAN, CAP]] == 0).all()
    first = [i for i in good if kind[i] == "first"]
    assert (info["steps"][first].sum(axis=1) == 1).all(), "the lanes that stop in their first step"
    zero = [i for i in good if kind[i] == "zero"]
    assert (info["steps"][zero] == 0).all() and (info["t_end"][zero] == tfs[zero]).all()
    _same_bits(np.array([res[i][0] for i in zero]), rows[zero], "tf == t0: the row itself")
    got = _as_got(res, info, 2)
    eck.compare_case(case, [got[i] for i in good], B, factor=2.0, what="device, every good lane:")
    for i in (NAN - 1, NAN + 1, CAP - 1, CAP + 1):                                     # the neighbours of the failed lanes, run alone
        alone, ainfo = g.integrate_parallel(rows[i:i + 1], tfs[i:i + 1], ev, details=True)
        _same_bits(alone[0][0], res[i][0], f"lane {i} alone")
        _same_bits(ainfo["ev_rows"][0], info["ev_rows"][i], f"lane {i} alone: its events")
        assert np.array_equal(ainfo["steps"][0], info["steps"][i]) and ainfo["stopped"][0] == info["stopped"][i]
    from asset_asrl_amd.integrator import IntegrationError
    with pytest.raises(IntegrationError, match="2 of 64 propagations failed"):
        g.integrate_parallel(rows, tfs, ev)


# ---- several events in one step
@pytest.mark.parametrize("direction,stop,stopped,counts", [((0, 0, 0), (1, 1, 0), 0, (1, 1, 0)), ((0, 0, 0), (0, 1, 0), 1, (1, 1, 0)),
                                                           ((-1, 1, 0), (0, 0, 0), -1, (1, 0, 1)), ((1, -1, -1), (0, 0, 0), -1, (0, 1, 0))])
def test_three_events_two_of_them_in_one_step(direction, stop, stopped, counts):
    """x0 = cos t, fixed steps of 0.4: x0 - 0.01 crosses at 1.5608 and x0 at 1.5708, both inside the step (1.2, 1.6); x1 = -sin t at pi.
    Fixed steps: the device and the restatement walk the same discrete map, so they differ by rounding (64 u) and by what the
    termination rule allows each root finder -- dt of tests/event_checker.py with B = 64 u on each side."""
    names = ("x0", "x0m", "x1")
    opt = gck.options(def_step=0.5, min_step=1.0e-5, max_step=1.0, adaptive=False)
    rows, tfs = np.array([[1.0, 0.0, 0.0]]), np.array([4.0])
    ref = eck.propagate_events(eck.SYSTEMS["oscillator"]["f"], [eck.SYSTEMS["oscillator"]["events"][e][0] for e in names], rows[0], 4.0,
                               direction, stop, opt)
    assert tuple(ref["count"]) == counts and ref["stopped"] == stopped                   # (the test's own premise)
    if stopped >= 0:
        assert ref["steps"] == (4, 0) and abs(ref["t_end"] - 1.6) < 1e-12
    res, info = _integrator("oscillator", opt).integrate_parallel(rows, tfs, event_cases.events_of("oscillator", names, direction, stop),
                                                                  details=True)
    assert info["status"][0] == 0 and tuple(info["ev_count"][0]) == counts and info["stopped"][0] == stopped
    assert tuple(info["steps"][0]) == ref["steps"]
    Bx = 64.0 * U * np.ones(2)
    for j in range(3):
        assert len(res[0][1][j]) == counts[j] == len(ref["locs"][j])
        for got, loc in zip(res[0][1][j], ref["locs"][j]):
            y = np.array([float(v) for v in loc["x"]] + [float(loc["t"])])
            fv, dg = eck.SYSTEMS["oscillator"]["f"](y), eck.SYSTEMS["oscillator"]["events"][names[j]][1](y)
            dt = eck.event_time_bound(1.0e-6, np.abs(dg), Bx, abs(dg @ fv))
            assert abs(got[2] - float(loc["t"])) <= 2.0 * dt, (j, got[2], loc["t"], dt)
            assert (np.abs(got[:2] - y[:2]) <= 2.0 * eck.event_state_bound(Bx, np.abs(fv), dt)).all(), (j, got, y)
    assert abs(res[0][0][2] - ref["t_end"]) <= 8.0 * U * 4.0
    assert (np.abs(res[0][0][:2] - np.asarray(ref["x"], dtype=float)) <= Bx).all()


# ---- the cap on stored occurrences
def test_occurrences_beyond_max_event_locs_are_counted_not_stored():
    opt = gck.options(def_step=0.1, min_step=1.0e-5, max_step=1.0)
    g = _integrator("oscillator", opt, locs=2)
    rows, tfs = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), np.array([16.0, 3.0])       # crossings at pi / 2 + k pi: five, and one
    res, info = g.integrate_parallel(rows, tfs, event_cases.events_of("oscillator", ("x0",), (0,), (0,)), details=True)
    assert info["ev_count"].ravel().tolist() == [5, 1] and (info["stopped"] == -1).all() and (info["status"] == 0).all()
    assert [len(r[1][0]) for r in res] == [2, 1] and info["ev_rows"].shape == (2, 1, 2, 3)
    assert np.allclose([r[2] for r in res[0][1][0]], [PI / 2, 3 * PI / 2], atol=1e-5, rtol=0) and abs(res[1][1][0][0][2] - PI / 2) < 1e-5
    assert np.isnan(info["ev_rows"][1, 0, 1]).all() and np.isnan(info["ev_resid"][1, 0, 1]) and info["ev_conv"][1, 0].tolist() == [1, 0]
    # a stop count at the cap: the third occurrence is stored and stops the propagation
    g2 = _integrator("oscillator", opt, locs=3)
    res2, info2 = g2.integrate_parallel(rows[:1], tfs[:1], event_cases.events_of("oscillator", ("x0",), (0,), (3,)), details=True)
    assert info2["ev_count"][0, 0] == 3 and info2["stopped"][0] == 0 and 5 * PI / 2 < res2[0][0][2] < 5 * PI / 2 + 1.0
    with pytest.raises(ValueError, match="MaxEventLocs"):
        g.integrate_parallel(rows, tfs, event_cases.events_of("oscillator", ("x0",), (0,), (3,)))


# ---- occurrences that are not located
def test_an_occurrence_that_uses_up_its_evaluations_is_flagged_and_dropped():
    opt = gck.options(def_step=0.1, min_step=1.0e-5, max_step=1.0)
    g = _integrator("oscillator", opt, event_tol=1.0e-14, iters=1)
    rows, tfs = np.array([[1.0, 0.0, 0.0], [2.0, 0.0, 0.0]]), np.array([6.0, 6.0])
    ev = event_cases.events_of("oscillator", ("x0",), (0,), (0,))
    res, info = g.integrate_parallel(rows, tfs, ev, details=True)
    assert info["ev_count"].ravel().tolist() == [2, 2] and (info["status"] == 0).all()
    assert (info["ev_conv"][:, 0, :2] == 0).all() and all(r[1] == [[]] for r in res), "absent from the returned lists"
    stored = info["ev_rows"][:, 0, :2]
    assert np.isfinite(stored).all() and np.isfinite(info["ev_resid"][:, 0, :2]).all(), "present under details=True"
    assert (np.abs(info["ev_resid"][:, 0, :2]) >= 1.0e-14).all()
    assert np.allclose(stored[:, :, 2], [[PI / 2, 3 * PI / 2]] * 2, atol=0.05, rtol=0)     # one secant step from a bracket of about 0.3
    plain = g.integrate_parallel(rows, tfs, ev)
    assert all(r[1] == [[]] for r in plain)
    # the propagation itself is not disturbed
    g10 = _integrator("oscillator", opt)
    res10, info10 = g10.integrate_parallel(rows, tfs, ev, details=True)
    _same_bits(np.array([r[0] for r in res10]), np.array([r[0] for r in res]), "end rows with one and with ten evaluations")
    assert (info10["ev_conv"][:, 0, :2] == 1).all()
