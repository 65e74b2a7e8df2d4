"""The device de Boor estimator (csrc/mesh_kernels.h through asset_hip_mesh_error_deboor, asset_asrl_amd/mesh.py and
Phase.get_meshinfo_deboor) against the 50-digit fixture tests/golden/mesh_error.npz, and -- where there is no fixture -- against the
float64 oracle, both under the conditioning-aware bounds of tests/mesh_checker.py: ragged and time-reversed meshes, 2 to 100 000 blocks,
BlockConstant control with and without controls and parameters, smooth trajectories where rounding dominates the estimate, AutoScaling,
NaN data, and the input errors of the C entry point."""
import ctypes as C

import numpy as np
import pytest

import interp_checker as ick
import mesh_checker as mck
from asset_asrl_amd import _lib, jit, mesh

pytestmark = pytest.mark.gpu

_ODES = {}


def _device_name(case):
    """The device-side name of the case's ODE (user ODEs are compiled, or found in the module cache, once per session)."""
    key = (case["ode"], case["mode"], case["blocked"])
    if key not in _ODES:
        ode = mck.device_ode(case)
        _ODES[key] = ode if isinstance(ode, str) else jit.ensure_kernel(ode, case["mode"], case["blocked"])
    return _ODES[key]


def _own_maxima(err, dist, emax, dmax, what):
    """error_max / dist_max are the maxima of the device's own columns, bit for bit -- numpy's maximum: NaN where a state is NaN."""
    np.testing.assert_array_equal(emax, np.abs(err).max(axis=0), err_msg=f"{what}: error_max")
    np.testing.assert_array_equal(dmax, np.abs(dist).max(axis=0), err_msg=f"{what}: dist_max")


@pytest.mark.parametrize("name", mck.case_names())
def test_device_matches_the_50_digit_fixture(name):
    c = mck.fixture()[1][name]
    tsnd, err, dist, emax, dmax = mesh.mesh_error_deboor(_device_name(c), c["mode"], c["traj"], c["blocked"])
    wt, we, wd = mck.compare_with_fixture(c, (tsnd, err, dist), what=name)
    print(f"{name} [{c['family']}]: worst |got - ref| / bound: tsnd {wt:.3f}, mesh_errors {we:.3f}, mesh_dist {wd:.3f}")
    _own_maxima(err, dist, emax, dmax, name)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "time-reversed"])
@pytest.mark.parametrize("nb", [63, 64, 65, 128, 129, 100000])
def test_workgroup_edges_and_a_large_mesh_against_the_oracle(oracle, nb, reverse):
    """One thread per block in workgroups of 64: the last workgroup full, one thread over, one short; and 1563 workgroups.  No fixture:
    the reference is the float64 oracle, each side within tau of the exact value, so the bound is 2 tau."""
    traj = ick.ragged_traj("reentry", "LGL7", nb, seed=900 + nb)
    if reverse:
        traj = traj[::-1].copy()
    tsnd, err, dist, emax, dmax = mesh.mesh_error_deboor("reentry", "LGL7", traj)
    ref = oracle.mesh_error_deboor(oracle.get_ode("reentry", 0), oracle.MODES["LGL7"], traj)
    w = mck.compare_float64_codes((tsnd, err, dist), ref, traj, "LGL7", False, 5, 2, ick.oracle_rhs(oracle, "reentry"),
                                  mck.eps_f("reentry"), what=f"reentry LGL7 x{nb}")
    print(f"reentry LGL7 x{nb} reversed={reverse}: worst |device - oracle| / (2 tau): tsnd {w[0]:.3f}, mesh_errors {w[1]:.3f}, mesh_dist {w[2]:.3f}")
    _own_maxima(err, dist, emax, dmax, f"x{nb}")


@pytest.mark.parametrize("mode,control", [("LGL5", "HighestOrderSpline"), ("LGL3", "BlockConstant")])
def test_phase_estimate_with_autoscaling_is_the_estimate_in_scaled_units(oracle, mode, control):
    """Phase.get_meshinfo_deboor with AutoScaling on: the estimate of the trajectory and dynamics written in scaled units, x / ux, t / ut,
    f ut / ux -- computed by the checker in longdouble, from the oracle's right-hand side, with the bound of the scaled data."""
    from asset_asrl_amd.ode import ShuttleReentry
    nb, xv, uv = 29, 5, 2
    src = ick.ragged_traj("reentry", mode, nb, seed=61)
    edges = src[::mck.MODE_CS[mode] - 1, xv]
    ph = ShuttleReentry().phase(mode)
    ph.setControlMode(control)
    ph.setTraj(src, (edges - edges[0]) / (edges[-1] - edges[0]), np.ones(nb, dtype=int))
    units = np.array([2.0, 0.5, 3.0, 1.5, 0.8, 4.0, 1.25, 2.5])
    ph.setUnits(units)
    ph.setAutoScaling(True)
    traj = np.asarray(ph.ActiveTraj, dtype=float)
    assert traj.shape == src.shape and np.abs(traj - src).max() < 1e-12            # physical units, the ragged mesh
    blocked = control == "BlockConstant"
    tsnd, err, dist = ph.get_meshinfo_deboor()
    f = ick.oracle_rhs(oracle, "reentry")
    rhs_scaled = lambda rows: f(rows * units[None, :]) * (units[xv] / units[:xv])[None, :]
    scaled = traj / units[None, :]
    rt, re, rerr, rdist = mck.estimate(scaled, mode, blocked, xv, uv, rhs_scaled)
    tau = mck.tau_of(*mck.tolerance_data(scaled, mode, blocked, xv, uv, rhs_scaled), mck.eps_f("reentry"))
    w = mck.compare((tsnd, err, dist), (rt, re, rerr, rdist), tau, mck.block_widths(scaled, mode, xv), mode, what=f"AutoScaling {mode}")
    print(f"AutoScaling {mode} {control}: worst |got - ref| / bound: tsnd {w[0]:.3f}, mesh_errors {w[1]:.3f}, mesh_dist {w[2]:.3f}")
    # and the scaling is not a no-op: the unscaled estimate is another one
    ph.setAutoScaling(False)
    assert np.abs(ph.get_meshinfo_deboor()[1] / err - 1.0).max() > 0.1


def _call(ode, mode, blocked, traj, nnodes):
    """asset_hip_mesh_error_deboor itself: (status, message, outputs -- pre-filled with a sentinel)."""
    traj = np.ascontiguousarray(traj, dtype=np.float64)
    n = max(nnodes, 2)
    out = [np.full(n + 1, -7.0), np.full((n + 1) * 8, -7.0), np.full((n + 1) * 8, -7.0), np.full(n + 1, -7.0), np.full(n + 1, -7.0)]
    dp = C.POINTER(C.c_double)
    rc = _lib.lib().asset_hip_mesh_error_deboor(ode.encode(), mode, int(blocked), traj.ctypes.data_as(dp), nnodes,
                                                *[a.ctypes.data_as(dp) for a in out], 0)
    return rc, _lib.lib().asset_hip_last_error().decode(errors="replace"), out


def test_input_errors_are_statuses_with_a_message_and_nothing_is_written():
    from asset_asrl_amd import vf
    traj = ick.ragged_traj("reentry", "LGL7", 4, seed=3)                        # 13 nodes
    a = vf.Arguments(6)
    x0, x1, x2, t, u0, u1 = a.tolist()
    fn = jit.ensure_function(vf.stack([x0 * x0 + x1 * u0 - vf.sin(x2), u0 * u0 + u1 * u1 - 1.0 + t * x0 * vf.exp(-1.0 * x1)]), "pathcon")
    for what, args, word in (("one block", ("reentry", _lib.MODES["LGL7"], 0, traj, 4), "nb >= 2"),
                             ("a node count that is not nb (cs - 1) + 1", ("reentry", _lib.MODES["LGL7"], 0, traj, 12), "nb*(cs-1)+1"),
                             ("an unknown ODE", ("no_such_ode", _lib.MODES["LGL7"], 0, traj, 13), "no_such_ode"),
                             ("a plain function", (fn, _lib.MODES["Function"], 0, traj, 13), "not a transcription")):
        rc, msg, out = _call(*args)
        assert rc != 0 and word in msg, (what, rc, msg)
        assert all(np.all(o == -7.0) for o in out), what                         # refused before anything ran
    with pytest.raises(_lib.AssetHipError, match="nb >= 2"):
        mesh.mesh_error_deboor("reentry", "LGL7", traj[:4])
    rc, msg, out = _call("reentry", _lib.MODES["LGL7"], 0, traj, 13)           # (the same call with valid arguments runs)
    assert rc == 0 and not np.any(out[0][:5] == -7.0)


@pytest.mark.parametrize("mode,blocked,nb,node,state", [("LGL7", False, 70, 101, 2), ("LGL5", True, 9, 0, 4), ("Trapezoidal", False, 5, 5, 0)])
def test_a_nan_state_shows_in_the_estimate_and_in_both_maxima(oracle, mode, blocked, nb, node, state):
    """One NaN state: mesh_errors / mesh_dist are NaN exactly where the restatement's are (the blocks that hold the node and their
    neighbours, in the states the right-hand side carries it to), finite entries stay inside the bound, and error_max / dist_max of
    those blocks are NaN -- numpy's maximum.  (fmax would drop the NaN and report 0 for a block whose only entry is NaN.)"""
    traj = ick.ragged_traj("reentry", mode, nb, seed=8)
    traj[node, state] = np.nan
    rhs = ick.oracle_rhs(oracle, "reentry")
    tsnd, err, dist, emax, dmax = mesh.mesh_error_deboor("reentry", mode, traj, blocked)
    rt, re, rerr, rdist = mck.estimate(traj, mode, blocked, 5, 2, rhs)
    assert np.isnan(rerr).any() and not np.isnan(rerr).all()
    # the bound of the finite entries: |f|_inf over the finite components only (a finite entry of a block that holds the NaN node is a
    # state whose right-hand side does not see it); compare() reads tau only where the reference is finite
    with np.errstate(invalid="ignore"):
        ts, tp = mck.tolerance_data(traj, mode, blocked, 5, 2, lambda rows: np.nan_to_num(rhs(rows), nan=0.0))
    tau = np.nan_to_num(mck.tau_of(ts, tp, mck.eps_f("reentry")), nan=0.0)
    assert np.all(tau[~np.isnan(rerr[:, :-1])] > 0.0)
    mck.compare((tsnd, err, dist), (rt, re, rerr, rdist), tau, mck.block_widths(traj, mode, 5), mode, what=f"NaN {mode}")
    _own_maxima(err, dist, emax, dmax, f"NaN {mode}")
    nan_blocks = np.isnan(rerr).any(axis=0)
    assert np.array_equal(np.isnan(emax), nan_blocks) and np.array_equal(np.isnan(dmax), nan_blocks)
    assert nan_blocks.sum() >= 2 and not nan_blocks.all()
