"""The device integrator-based mesh-error estimator (csrc/integ_kernels.h through asset_hip_mesh_error_integrator, asset_asrl_amd/mesh.py
and Phase.get_meshinfo_integrator) against the 50-digit fixture tests/golden/mesh_integ/mesh_error_integ.npz and -- where there is no fixture --
against the float64 restatement of tests/integ_checker.py (each side within its bound of the exact end state, so the two are within
twice the bound of each other): every fixture case, workgroup edges, a multi-workgroup mesh, the reduced-lane path of the 32-state
ODE, AutoScaling, a NaN state, the step cap, the input errors, and the adaptive mesh loop end to end on the cart-pole."""
import time

import numpy as np
import pytest

import integ_checker as gck
import interp_checker as ick
import mesh_checker as mck
from asset_asrl_amd import _lib, jit, mesh
from test_adaptive_mesh_known_answer import REFERENCE_OBJECTIVE, REFERENCE_TOLERANCE, shim  # noqa: F401  (the harness, as it is)
from test_integ_cpu import INPUT_ERRORS, _call, _opts

pytestmark = pytest.mark.gpu

_ODES = {}


def _device_name(case):
    key = (case["ode"], case["mode"], case["blocked"])
    if key not in _ODES:
        ode = mck.device_ode(case)
        _ODES[key] = ode if isinstance(ode, str) else jit.ensure_kernel(ode, case["mode"], case["blocked"])
    return _ODES[key]


def _options(xv, opt):
    o = mesh.IntegratorOptions(xv)
    o.setStepSizes(opt["def_step"], opt["min_step"], opt["max_step"])
    o.MaxStepChange, o.Adaptive, o.MaxSteps = opt["max_step_change"], opt["adaptive"], opt["max_steps"]
    o.setAbsTols(np.broadcast_to(opt["abs_tol"], (xv,)))
    o.setRelTols(np.broadcast_to(opt["rel_tol"], (xv,)))
    return o


def _short_traj(ode, mode, nb, seed, dt, sizes=None):
    """random node rows on a ragged mesh with node intervals |H| <= 0.2 (tests/golden/make_golden_mesh_integ.py)"""
    traj = ick.ragged_traj(ode, mode, nb, seed=seed, T=dt * nb, sizes=sizes, spread=2.0)
    xv = (sizes or {"reentry": (5, 2, 0), "synthetic32": (32, 0, 0)}[ode])[0]
    assert np.abs(np.diff(traj[:, xv])).max() <= 0.2
    return traj


@pytest.mark.parametrize("name", gck.case_names())
def test_device_matches_the_50_digit_fixture(name):
    c = gck.fixture()[1][name]
    xv, uv, _ = c["sizes"]
    opt = gck.case_options(c)
    out = mesh.mesh_error_integrator(_device_name(c), c["mode"], c["traj"], c["blocked"], _options(xv, opt), details=True)
    xend, steps, status = out[5:]
    assert (status == 0).all(), status
    if opt["adaptive"]:
        ref, B = c["x_exact"], gck.state_bound(c["x_exact"], c["steps64"][:, 0], opt["abs_tol"])
        gck.compare_step_totals(steps, c["steps64"], name)
    else:
        ref, B = c["xld"], 8.0 * c["d64"] + 16.0 * gck.U * np.abs(c["x_exact"])
        np.testing.assert_array_equal(steps, c["steps64"])                          # numsteps + 1, 0 (tests/test_integ_cpu.py)
    wx = gck.compare_states(xend, ref, B, name)
    wt, we, wd = gck.compare_estimate(out[:5], c["traj"], c["mode"], xv, ref, B, name)
    print(f"{name}: worst |got - ref| / bound: xend {wx:.3f}, tsnd {wt:.3f}, mesh_errors {we:.3f}, mesh_dist {wd:.3f}; steps "
          f"{steps.sum(axis=0)} against the restatement's {c['steps64'].sum(axis=0)}")


def _against_restatement(oracle, ode, dev, mode, traj, sizes, what, blocked=False, sample=None, rhs=None, opt=None):
    xv, uv, _ = sizes
    opt = opt or gck.options()
    out = mesh.mesh_error_integrator(dev, mode, traj, blocked, _options(xv, opt), details=True)
    xend, steps, status = out[5:]
    assert (status == 0).all()
    ids = np.arange(traj.shape[0] - 1) if sample is None else sample
    x64, steps64, st64 = gck.reintegrate(rhs or ick.oracle_rhs(oracle, ode), traj, mode, blocked, xv, uv, opt, intervals=ids)
    assert (st64 == 0).all()
    B = 2.0 * gck.state_bound(x64, steps64[:, 0], opt["abs_tol"])
    wx = gck.compare_states(xend[ids], x64, B, what)
    gck.compare_step_totals(steps[ids], steps64, what)
    if sample is None:
        wt, we, wd = gck.compare_estimate(out[:5], traj, mode, xv, x64, B, what)
    else:
        gck.check_column_maxima(*out[1:5], what)
        wt = float(np.abs(out[0] - np.append((traj[:-1:gck.MODE_CS[mode] - 1, xv] - traj[0, xv]) / (traj[-1, xv] - traj[0, xv]), 1.0)).max() / (4 * gck.U))
        assert wt <= 1.0
        we = wd = float("nan")
    print(f"{what}: worst |device - restatement| / (2 bound): xend {wx:.3f}, tsnd {wt:.3f}, mesh_errors {we:.3f}, mesh_dist {wd:.3f}; steps "
          f"{steps[ids].sum(axis=0)} against {steps64.sum(axis=0)}")
    return out


@pytest.mark.parametrize("mode,nb,dt", [("Trapezoidal", 63, 0.08), ("Trapezoidal", 64, 0.08), ("Trapezoidal", 65, 0.08), ("LGL7", 21, 0.2),
                                        ("LGL7", 22, 0.2)])
def test_workgroup_edges_against_the_restatement(oracle, mode, nb, dt):
    """64 intervals per workgroup: the last one a lane short, full, one lane into the next (Trapezoidal: intervals = blocks); LGL7: 63 and
    66 intervals, the second workgroup starting inside a block."""
    traj = _short_traj("reentry", mode, nb, 700 + nb, dt)
    _against_restatement(oracle, "reentry", "reentry", mode, traj, (5, 2, 0), f"reentry {mode} x{nb}")


def test_a_multi_workgroup_mesh_on_a_strided_sample(oracle):
    nb = 3000
    traj = _short_traj("reentry", "LGL5", nb, 71, 0.16)
    sample = np.arange(200) * 30 + (np.arange(200) % 7)                               # both intervals of a block, every lane position
    _against_restatement(oracle, "reentry", "reentry", "LGL5", traj, (5, 2, 0), "reentry LGL5 x3000 (200 of 6000 intervals)", sample=sample)


def test_the_32_state_ode_runs_with_fewer_lanes(oracle):
    """13 x 32 stage values per lane: 8 active lanes per workgroup -- that path has to be correct, not fast."""
    traj = _short_traj("synthetic32", "LGL3", 3, 5, 0.08)
    _against_restatement(oracle, "synthetic32", "synthetic32", "LGL3", traj, (32, 0, 0), "synthetic32 LGL3 x3")
    traj = _short_traj("synthetic32", "LGL3", 19, 6, 0.08)                            # three workgroups, the last one short
    _against_restatement(oracle, "synthetic32", "synthetic32", "LGL3", traj, (32, 0, 0), "synthetic32 LGL3 x19")


@pytest.mark.parametrize("mode,control", [("LGL5", "HighestOrderSpline"), ("LGL3", "BlockConstant")])
def test_phase_estimate_with_autoscaling_is_the_estimate_of_the_scaled_data(oracle, mode, control):
    """Phase.get_meshinfo_integrator with AutoScaling on: the scaled ODE integrated over ActiveTraj / XtUPUnits -- the restatement on the
    scaled rows with the right-hand side f(y units) ut / ux."""
    from asset_asrl_amd.ode import ShuttleReentry
    nb, xv, uv = 29, 5, 2
    src = _short_traj("reentry", mode, nb, 61, 0.16 if mode == "LGL5" else 0.08)
    edges = src[::gck.MODE_CS[mode] - 1, xv]
    ph = ShuttleReentry().phase(mode)
    ph.setControlMode(control)
    ph.setTraj(src, (edges - edges[0]) / (edges[-1] - edges[0]), np.ones(nb, dtype=int))
    units = np.array([2.0, 0.5, 3.0, 1.5, 0.8, 4.0, 1.25, 2.5])
    ph.setUnits(units)
    ph.setAutoScaling(True)
    traj = np.asarray(ph.ActiveTraj, dtype=float)
    assert traj.shape == src.shape and np.abs(traj - src).max() < 1e-12
    blocked = control == "BlockConstant"
    tsnd, err, dist = ph.get_meshinfo_integrator()
    f = ick.oracle_rhs(oracle, "reentry")
    rhs_scaled = lambda rows: f(rows * units[None, :]) * (units[xv] / units[:xv])[None, :]
    scaled = traj / units[None, :]
    opt = gck.options()
    x64, steps64, st64 = gck.reintegrate(rhs_scaled, scaled, mode, blocked, xv, uv, opt)
    assert (st64 == 0).all()
    B = 2.0 * gck.state_bound(x64, steps64[:, 0], opt["abs_tol"])
    with np.errstate(invalid="ignore"):
        got = (tsnd, err, dist, np.abs(err).max(axis=0), np.abs(dist).max(axis=0))
    w = gck.compare_estimate(got, scaled, mode, xv, x64, B, f"AutoScaling {mode}")
    print(f"AutoScaling {mode} {control}: worst |got - restatement| / (2 bound): tsnd {w[0]:.3f}, mesh_errors {w[1]:.3f}, mesh_dist {w[2]:.3f}")
    ph.setAutoScaling(False)                                                          # and the scaling is not a no-op
    assert np.abs(ph.get_meshinfo_integrator()[1] / err - 1.0).max() > 0.1


def test_a_nan_state_stops_its_two_intervals_and_shows_in_max_err(oracle):
    mode, nb, node, state, xv = "LGL5", 9, 7, 2, 5
    traj = _short_traj("reentry", mode, nb, 8, 0.16)
    traj[node, state] = np.nan
    opt = gck.options()
    tsnd, err, dist, emax, dmax, xend, steps, status = mesh.mesh_error_integrator("reentry", mode, traj, False, _options(xv, opt), details=True)
    touching = np.array([node - 1, node])
    others = np.setdiff1d(np.arange(2 * nb), touching)
    assert (status[touching] == 2).all() and np.isnan(xend[touching]).all()
    assert (status[others] == 0).all()
    x64, steps64, st64 = gck.reintegrate(ick.oracle_rhs(oracle, "reentry"), traj, mode, False, xv, 2, opt)
    assert np.array_equal(st64, status)
    wx = gck.compare_states(xend[others], x64[others], 2.0 * gck.state_bound(x64[others], steps64[others, 0], opt["abs_tol"]), "NaN state")
    # max_err is NaN (fmax would drop it), so every mesh_dist is; mesh_errors only in the block that holds the two intervals
    assert np.isnan(dist).all() and np.isnan(dmax).all()
    nan_blocks = np.zeros(nb + 1, dtype=bool)
    nan_blocks[node // 2] = True
    assert np.array_equal(np.isnan(err).all(axis=0), nan_blocks) and np.array_equal(np.isnan(err).any(axis=0), nan_blocks)
    assert np.array_equal(np.isnan(emax), nan_blocks)
    print(f"NaN state: worst |device - restatement| / (2 bound) of the other end states {wx:.3f}")


def test_the_step_cap_ends_an_interval_with_a_status(oracle):
    """max_steps = 3 on a case whose restatement needs more: those intervals stop with status 1 after exactly three steps, NaN end states;
    the loop is finite by construction.  (An interval within one step of the cap may fall on either side in another float64 code.)"""
    c = gck.fixture()[1]["reentry_LGL7_10"]
    xv = 5
    need = c["steps64"].sum(axis=1)
    assert (need > 4).sum() >= 5 and (need <= 2).sum() >= 0
    opt = gck.options(max_steps=3)
    t0 = time.perf_counter()
    tsnd, err, dist, emax, dmax, xend, steps, status = mesh.mesh_error_integrator("reentry", c["mode"], c["traj"], False, _options(xv, opt), details=True)
    assert time.perf_counter() - t0 < 5.0
    assert (status[need > 4] == 1).all() and (status[need <= 2] == 0).all() and set(status) <= {0, 1}
    capped = status == 1
    assert (steps[capped].sum(axis=1) == 3).all() and np.isnan(xend[capped]).all() and np.isfinite(xend[~capped]).all()
    assert np.isnan(dist).all()                                                       # max_err is NaN
    ok = gck.compare_states(xend[~capped], c["x_exact"][~capped], gck.state_bound(c["x_exact"], c["steps64"][:, 0], opt["abs_tol"])[~capped], "cap")
    print(f"step cap 3: {int(capped.sum())} of {capped.size} intervals stopped; the others within {ok:.3f} of their bound")


@pytest.mark.parametrize("what,change,word", INPUT_ERRORS, ids=[e[0] for e in INPUT_ERRORS])
def test_input_errors_with_a_device_present(what, change, word):
    traj = ick.ragged_traj("reentry", "LGL7", 4, seed=3, T=1.0)
    if "edit" in change:
        change["edit"](traj)
    rc, msg, out = _call(change.get("ode", "reentry"), _lib.MODES["LGL7"], 0, traj, change.get("nnodes", 13),
                         _opts(**change["opt"]) if "opt" in change else None)
    assert rc != 0 and word in msg, (what, rc, msg)
    assert all(np.all(o == -7) for o in out), what


def test_a_plain_function_is_refused_and_valid_input_runs():
    from asset_asrl_amd import vf
    traj = ick.ragged_traj("reentry", "LGL7", 4, seed=3, T=1.0)
    a = vf.Arguments(6)
    x0, x1, x2, t, u0, u1 = a.tolist()
    fn = jit.ensure_function(vf.stack([x0 * x0 + x1 * u0 - vf.sin(x2), u0 * u0 + u1 * u1 - 1.0 + t * x0 * vf.exp(-1.0 * x1)]), "pathcon")
    rc, msg, out = _call(fn, _lib.MODES["Function"], 0, traj, 13)
    assert rc != 0 and "not a transcription" in msg and all(np.all(o == -7) for o in out)
    with pytest.raises(_lib.AssetHipError, match="nb >= 1"):
        mesh.mesh_error_integrator("reentry", "LGL7", traj[:1])
    rc, msg, out = _call("reentry", _lib.MODES["LGL7"], 0, traj, 13, _opts())
    assert rc == 0 and not np.any(out[0][:5] == -7.0) and not np.any(out[7][:12] == -7)
    tsnd, err, dist = mesh.mesh_error_integrator("reentry", "LGL7", traj[:4])[:3]     # one block is a mesh here (de Boor needs two)
    assert tsnd.tolist() == [0.0, 1.0] and err.shape == (5, 2) and np.array_equal(err[:, 0], err[:, 1])


def test_adaptive_loop_with_the_integrator_estimator_converges_on_the_cart_pole(shim):  # noqa: F811
    """test_AdaptiveMesh/test_CartPole.py with MeshErrorEstimator = "integrator": from 16 LGL5 segments the loop converges and lands
    inside the reference's 58.832 +- 0.1."""
    import kkt_harness as kh
    mode = "LGL5"
    prob = kh.cartpole_problem(mode, "HighestOrderSpline", 16)
    ph = prob["phase"]
    ph.setAdaptiveMesh(True)
    ph.MeshErrFactor = 20.0
    ph.setMeshErrorEstimator("integrator")
    used = []

    def meshinfo(p):
        used.append(p.MeshErrorEstimator)
        return p._meshinfo()                                                          # what checkMesh itself dispatches to
    t0 = time.perf_counter()
    prob, x, lam, info = kh.solve_adaptive(lambda pr: kh.DeviceProvider(shim, pr), lambda p: kh.cartpole_problem(mode, "HighestOrderSpline", None, phase=p),
                                           prob, meshinfo, step_cap=np.inf)
    dt = time.perf_counter() - t0
    assert info["converged"] and info["feasible"], info
    assert ph.MeshConverged and info["mesh_converged"] and used and set(used) == {"integrator"}
    assert abs(info["objective"] - REFERENCE_OBJECTIVE) < REFERENCE_TOLERANCE
    its = ph.MeshIters
    assert its[0].numsegs == 16 and its[0].max_error > ph.MeshTol > its[-1].max_error
    print(f"cart-pole LGL5, integrator estimator: segments {[m.numsegs for m in its]}, max errors {[f'{m.max_error:.2e}' for m in its]}, "
          f"objective {info['objective']:.6f}, {dt:.1f} s")
