"""The reference's ADAPTIVE MESH loop around the de Boor estimate (SURVEY section 8 row f-3 and its caller: ODEPhaseBase.cpp:1443-1542
checkMesh / updateMesh, defaults ODEPhaseBase.h:96-118 -- here Phase.checkMesh / Phase.updateMesh, asset_asrl_amd/mesh.py:
MeshIterateInfo), end to end on the problem the reference tests it with: /root/reference/asset_asrl/test/test_AdaptiveMesh/
test_CartPole.py:36-107 -- the cart-pole swing-up from 32 (LGL3) / 16 (LGL5) / 10 (LGL7) segments with AdaptiveMesh on,
MeshErrFactor = 20, the default MeshTol = 1e-6; it asserts that the mesh converged and the objective is 58.83219229674185 +- 0.1.

Solve (tests/kkt_harness.py), estimate the error of the solution, re-mesh by the error density, solve again from the re-distributed
solution -- until the estimate is below the tolerance:
* on the CPU with the oracle's assembly AND the oracle's estimator (oracle/mesh.cpp);
* on the GPU (-m gpu) with the device kernels through the C ABI / KktAssembly and the DEVICE estimator (csrc/mesh_kernels.h), every
  mesh a new handle.

And on the re-entry problem (test_AdaptiveMesh/test_Reentry.py): from 40 / 20 / 15 segments at MeshTol = 1e-7 the loop ends on 446 / 78 /
31 segments with the cross-range -0.59588007165 / -0.59588007419 / -0.59588003641 -- the reference's recorded -0.5958800738629952 to
2e-9 / 3e-10 / 4e-8: its number is a mesh-converged one, and the converged meshes of this build land on it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import interp_checker as ick
import kkt_harness as kh
import mesh_checker as mck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_OBJECTIVE, REFERENCE_TOLERANCE = 58.83219229674185, 0.1       # test_AdaptiveMesh/test_CartPole.py:38-39
START = {"LGL3": 32, "LGL5": 16, "LGL7": 10}                            # :100
# this build: (segments of the converged mesh, objective on it) -- the continuous optimum is 58.8077; LGL3 stops at the
# tolerance with 160 segments (the increase per iteration is capped at MeshIncFactor = 5), where its discretisation error is 0.036
OWN = {"LGL3": (160, 58.843744), "LGL5": (43, 58.808245), "LGL7": (21, 58.807779)}


def _run(mode, make_provider, meshinfo):
    prob = kh.cartpole_problem(mode, "HighestOrderSpline", START[mode])
    ph = prob["phase"]
    ph.setAdaptiveMesh(True)
    ph.MeshErrFactor = 20.0                                              # :73
    prob, x, lam, info = kh.solve_adaptive(make_provider, lambda p: kh.cartpole_problem(mode, "HighestOrderSpline", None, phase=p),
                                           prob, meshinfo, step_cap=np.inf)
    assert info["converged"] and info["feasible"], info
    assert ph.MeshConverged and info["mesh_converged"]                                        # the reference's assertions
    assert abs(info["objective"] - REFERENCE_OBJECTIVE) < REFERENCE_TOLERANCE
    its = ph.MeshIters
    assert len(its) == 2 and its[0].numsegs == START[mode] and its[0].max_error > ph.MeshTol > its[-1].max_error
    assert its[0].up_numsegs == its[1].numsegs == ph.numDefects == OWN[mode][0]
    assert abs(info["objective"] - OWN[mode][1]) < 5e-6, info["objective"]
    return ph, x, info


@pytest.mark.parametrize("mode", list(START))
def test_oracle_loop_converges_to_the_reference_objective(oracle, mode):
    ode = oracle.get_ode("cartpole", 0)
    ph, x, info = _run(mode, lambda pr: kh.OracleProvider(oracle, pr),
                       lambda p: oracle.mesh_error_deboor(ode, oracle.MODES[mode], np.asarray(p.ActiveTraj), False))
    # the new mesh is not uniform: the error density put more segments where the pole swings through
    h = np.diff(np.asarray(ph.DefBinSpacing))
    assert h.max() / h.min() > 1.5


# ---- the same loop on the re-entry problem: test_AdaptiveMesh/test_Reentry.py:112-250 -- from 40 / 20 / 15 segments, MeshTol = 1e-7,
#      MeshIncFactor = 5, 'solve' then 'optimize'; mesh converged and the cross-range -0.5958800738629952 +- 1e-2
RE_START = {"LGL3": 40, "LGL5": 20, "LGL7": 15}
RE_OWN = {"LGL3": ([40, 200, 446], -0.59588007165), "LGL5": ([20, 72, 78], -0.59588007419), "LGL7": ([15, 31], -0.59588003641)}
RE_REFERENCE = -0.5958800738629952


def _run_reentry(mode, make_provider, meshinfo):
    prob = kh.reentry_problem(mode, "HighestOrderSpline", RE_START[mode])
    ph = prob["phase"]
    ph.setAdaptiveMesh(True)
    ph.setMeshTol(1.0e-7)
    ph.MeshIncFactor = 5
    prob, x, lam, info = kh.solve_adaptive(make_provider, lambda p: kh.reentry_problem(mode, "HighestOrderSpline", None, phase=p), prob,
                                           meshinfo, solver=kh.solve_reentry)
    assert info["converged"] and info["feasible"] and ph.MeshConverged, info
    assert abs(info["objective"] - RE_REFERENCE) < 1e-2                                       # the reference's own assertion
    assert [m.numsegs for m in ph.MeshIters] == RE_OWN[mode][0] and ph.MeshIters[-1].max_error < 1e-7
    assert abs(info["objective"] - RE_OWN[mode][1]) < 2e-9, info["objective"]
    # on the converged mesh the objective IS the reference's recorded value (its own meshes were converged to the same tolerance)
    assert abs(info["objective"] - RE_REFERENCE) < (5e-9 if mode != "LGL7" else 5e-8)
    return ph


@pytest.mark.parametrize("mode", list(RE_START))
def test_oracle_loop_on_the_reentry_problem(oracle, mode):
    ode = oracle.get_ode("reentry", 0)
    _run_reentry(mode, lambda pr: kh.OracleProvider(oracle, pr),
                 lambda p: oracle.mesh_error_deboor(ode, oracle.MODES[mode], np.asarray(p.ActiveTraj), False))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    pk = os.path.join(ROOT, "asset_asrl_amd")
    so = str(tmp_path_factory.mktemp("shim") / "shim_driver.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "host_shim_driver.cpp"),
                           "-o", so, "-L" + pk, "-lasset_host", "-lasset_hip", "-Wl,-rpath," + pk])
    return C.CDLL(so)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["LGL3", "LGL7"])
def test_device_loop_converges_to_the_reference_objective(oracle, shim, mode):
    ph, x, info = _run(mode, lambda pr: kh.DeviceProvider(shim, pr), lambda p: p.get_meshinfo_deboor())
    # the device estimate of the final solution against the oracle's
    ode = oracle.get_ode("cartpole", 0)
    t_o, e_o, d_o = oracle.mesh_error_deboor(ode, oracle.MODES[mode], np.asarray(ph.ActiveTraj), False)
    t_d, e_d, d_d = ph.get_meshinfo_deboor()
    assert np.abs(t_d - t_o).max() < 1e-14 and np.abs(e_d - e_o).max() < 1e-9 * max(1.0, np.abs(e_o).max()) + 1e-12
    # (that is a 1 % check, the errors of a converged mesh being about 1e-7: on top of it every entry is held to the bound of its own block and state -- two float64 codes,
    #  2 tau; tests/mesh_checker.py)
    traj = np.asarray(ph.ActiveTraj)
    w = mck.compare_float64_codes((t_d, e_d, d_d), (t_o, e_o, d_o), traj, mode, False, 4, 1, ick.oracle_rhs(oracle, "cartpole"),
                                  mck.eps_f("cartpole"), what=f"cartpole {mode}")
    print(f"cartpole {mode} x{ph.numDefects}: worst |device - oracle| / (2 tau): tsnd {w[0]:.3f}, mesh_errors {w[1]:.3f}, mesh_dist {w[2]:.3f}")


@pytest.mark.gpu
def test_device_loop_on_the_reentry_problem(oracle, shim):
    _run_reentry("LGL5", lambda pr: kh.DeviceProvider(shim, pr), lambda p: p.get_meshinfo_deboor())
