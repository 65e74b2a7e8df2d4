"""The integrator-based mesh-error estimator (csrc/integ_kernels.h, csrc/rk_tables.h, asset_hip_mesh_error_integrator, mesh.py, phase.py)
as far as it can be checked without a GPU: the Runge-Kutta tableau against the reference header's numbers and its own order conditions,
the float64 restatement of tests/integ_checker.py against the 50-digit fixture (the condition its bounds rest on), the argument checks
of IntegratorOptions, the estimator switch of Phase, the C entry point's input errors, and that a run-time compiled ODE gets the two
new kernels.  The device itself: tests/test_gpu_mesh_error_integ.py."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

import integ_checker as gck
import interp_checker as ick
from asset_asrl_amd import _lib, jit, mesh
from asset_asrl_amd.ode import ShuttleReentry
from helpers import Workload, make_vanderpol

HERE = os.path.dirname(os.path.abspath(__file__))
REF = json.load(open(os.path.join(HERE, "golden", "rk_tables.json")))["tables"]


# ---- tableau
@pytest.mark.parametrize("which", ["a", "c", "b", "bhat"])
def test_product_tableau_equals_the_reference_header_bit_for_bit(which):
    np.testing.assert_array_equal(_lib.rk_table(which), np.array(REF[which], dtype=float), err_msg=f"csrc/rk_tables.h {which}")


def test_tableau_satisfies_its_row_sums_and_quadrature_conditions():
    a, c, b, bhat = (_lib.rk_table(k) for k in ("a", "c", "b", "bhat"))
    assert np.all(np.triu(a, 1) == 0.0)                                              # explicit
    assert np.abs(a.sum(axis=1) - c).max() <= 4e-15
    nodes = np.concatenate([[0.0], c])
    for k in range(8):
        assert abs((b * nodes ** k).sum() - 1.0 / (k + 1)) <= 1e-15, ("b", k)
    for k in range(7):
        assert abs((bhat * nodes ** k).sum() - 1.0 / (k + 1)) <= 1e-15, ("bhat", k)
    assert abs((bhat * nodes ** 7).sum() - 1.0 / 8.0) > 1e-6                          # ... and bhat is the order-7 one


def test_rk_table_query_errors():
    buf = np.zeros(144)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert _lib.lib().asset_hip_rk_table(b"nope", p, 144) < 0 and b"unknown table" in _lib.lib().asset_hip_last_error()
    assert _lib.lib().asset_hip_rk_table(b"a", p, 143) < 0 and b"too small" in _lib.lib().asset_hip_last_error()
    assert np.all(buf == 0.0)


# ---- the restatement against the 50-digit fixture
@pytest.mark.parametrize("name", gck.case_names())
def test_restatement_uses_at_most_a_quarter_of_the_bound(oracle, name):
    """The float64 restatement (the oracle's right-hand side), run again here, reproduces the fixture's step counts and stays within
    accepted64 AbsTol of the 50-digit end states on every interval: a quarter of the bound the device is held to.  The fixed-step
    case: numsteps + 1 steps, none rejected, and the float64 result within the recorded d64 of the longdouble one."""
    c = gck.fixture()[1][name]
    xv, uv, _ = c["sizes"]
    opt = gck.case_options(c)
    x64, steps, status = gck.reintegrate(ick.oracle_rhs(oracle, c["ode"]), c["traj"], c["mode"], c["blocked"], xv, uv, opt)
    assert (status == 0).all()
    np.testing.assert_array_equal(steps, c["steps64"])
    err = np.abs(x64.astype(gck.LD) - c["x_exact"].astype(gck.LD)).astype(float)
    H = np.diff(c["traj"][:, xv])
    assert np.abs(H).max() <= 0.2
    assert (np.abs(err - c["err64"]) <= gck.U * np.abs(c["x_exact"])).all()          # (x_exact is stored rounded to float64)
    if opt["adaptive"]:
        quarter = steps[:, :1] * np.broadcast_to(opt["abs_tol"], (xv,))[None, :]
        assert (c["err64"] <= quarter).all(), float((c["err64"] / quarter).max())
        assert (4.0 * quarter <= gck.state_bound(c["x_exact"], steps[:, 0], opt["abs_tol"])).all()
        print(f"{name}: restatement uses {float((c['err64'] / quarter).max()):.3g} of accepted64 AbsTol, steps {steps.sum(axis=0)}")
    else:
        numsteps = (np.abs(H / opt["def_step"])).astype(int) + 1
        np.testing.assert_array_equal(steps, np.column_stack([numsteps + 1, 0 * numsteps]))
        assert numsteps.max() <= 8                                                    # beyond, 0.9 H / numsteps needs numsteps + 2 steps
        d = np.abs(x64.astype(gck.LD) - c["xld"]).astype(float)
        assert (d <= c["d64"] + 1e-300).all() and c["d64"].max() < 64 * gck.U * np.abs(c["x_exact"]).max()


def test_fixture_holds_the_cases_and_its_own_convergence():
    meta, cases = gck.fixture()
    assert 10 <= len(cases) <= 16
    assert all(c["convergence"] < 1e-25 and c["traj"].shape[0] - 1 <= 70 for c in cases.values())
    have = {(c["ode"], c["mode"], c["blocked"]) for c in cases.values()}
    for want in [("reentry", m, False) for m in ("Trapezoidal", "LGL3", "LGL5", "LGL7")] + [("reentry", "LGL5", True), ("vanderpol", "LGL7", False),
                                                                                          ("twobody_lt", "LGL5", False)]:
        assert want in have, want
    assert any(c["ode"] == "shape_1_0_0" for c in cases.values()) and any(c["ode"] == "shape_5_3_2" for c in cases.values())
    assert any(c["reverse"] for c in cases.values()) and any(c["options"].get("adaptive") is False for c in cases.values())


# ---- IntegratorOptions
def test_integrator_options_defaults_and_argument_checks():
    o = mesh.IntegratorOptions(5)
    assert (o.DefStepSize, o.MinStepSize, o.MaxStepSize, o.MaxStepChange, o.Adaptive, o.MaxSteps) == (0.01, 0.01 / 10000, 0.01 * 10000, 3.0, True, 100000)
    assert np.array_equal(o.AbsTols, np.full(5, 1e-12)) and np.array_equal(o.RelTols, np.zeros(5))
    o.setAbsTol(-1e-9)
    o.setRelTol(-1e-8)
    assert np.array_equal(o.AbsTols, np.full(5, 1e-9)) and np.array_equal(o.RelTols, np.full(5, 1e-8))       # abs(), as the reference
    o.setAbsTols(np.arange(1, 6) * 1e-10)
    o.setRelTols([0.0, 1e-9, 0.0, 0.0, 1e-7])
    assert o.AbsTols[4] == 5e-10 and o.RelTols[4] == 1e-7
    for setter in (o.setAbsTols, o.setRelTols):
        with pytest.raises(ValueError, match="Incorrectly sized tolerance vector"):
            setter(np.ones(4))
    o.setStepSizes(0.1, 0.001, 10.0)
    assert (o.DefStepSize, o.MinStepSize, o.MaxStepSize) == (0.1, 0.001, 10.0)
    for args, word in (((0.1, 0.2, 1.0), "greater than minimum"), ((0.1, 0.01, 0.05), "less maximum"), ((-0.1, -0.2, 1.0), "positive")):
        with pytest.raises(ValueError, match=word):
            o.setStepSizes(*args)
    assert (o.DefStepSize, o.MinStepSize, o.MaxStepSize) == (0.1, 0.001, 10.0)        # a refused call changes nothing
    c, keep = o._c()
    assert (c.def_step, c.min_step, c.max_step, c.max_step_change, c.adaptive, c.max_steps) == (0.1, 0.001, 10.0, 3.0, 1, 100000)
    assert c.abs_tols[4] == 5e-10 and c.rel_tols[1] == 1e-9


# ---- Phase
def _phase(mode="LGL5", nseg=10):
    w = Workload("reentry", mode, nseg)
    return ShuttleReentry().phase(mode, w.traj, nseg)


def test_phase_estimator_switch_and_check_mesh_dispatch(monkeypatch):
    ph = _phase()
    assert ph.MeshErrorEstimator == "deboor" and isinstance(ph.integrator, mesh.IntegratorOptions) and ph.integrator.xv == 5
    nb = ph.numDefects
    tsnd = np.linspace(0.0, 1.0, nb + 1)
    calls = []

    def fake(tag, level):
        def f():
            calls.append(tag)
            return tsnd, np.full((5, nb + 1), level), np.ones((5, nb + 1))
        return f
    monkeypatch.setattr(ph, "get_meshinfo_deboor", fake("deboor", 1e-3))
    monkeypatch.setattr(ph, "get_meshinfo_integrator", fake("integrator", 1e-9))
    assert ph.checkMesh() is False and calls == ["deboor"]                            # the default is unchanged
    ph.setMeshErrorEstimator("integrator")
    assert ph.MeshErrorEstimator == "integrator"
    assert ph.checkMesh() is True and calls == ["deboor", "integrator"] and ph.MeshIters[-1].max_error == 1e-9
    ph.setMeshErrorEstimator("simpson")
    with pytest.raises(ValueError, match="Unknown mesh error estimator"):
        ph.checkMesh()
    assert len(ph.MeshIters) == 2
    ph.setMeshErrorEstimator("deboor")
    ph.MeshErrorCriteria = "endtoend"
    with pytest.raises(ValueError, match="Unknown mesh error criteria"):             # still refused, with the existing error
        ph.checkMesh()
    # getMeshInfo(integ=...) picks the estimator by its argument
    ph.MeshErrorCriteria = "max"
    ph.getMeshInfo(integ=True, n=4)
    ph.getMeshInfo(integ=False, n=4)
    assert calls[-2:] == ["integrator", "deboor"]


def test_get_mesh_info_with_the_integrator_needs_a_device_not_an_implementation():
    """getMeshInfo(integ=True) used to raise NotImplementedError; now it reaches the library, which has no CPU fallback: without a
    device its no-device error, with one the estimate."""
    ph = _phase()
    if os.path.exists("/dev/kfd"):
        tsnd, bins, error = ph.getMeshInfo(integ=True, n=7)
        assert tsnd.shape == error.shape == (ph.numDefects + 1,) and bins.shape == (8,)
        return
    with pytest.raises(_lib.AssetHipError, match="no HIP device visible"):
        ph.getMeshInfo(integ=True)
    with pytest.raises(_lib.AssetHipError, match="no HIP device visible"):
        ph.get_meshinfo_integrator()


# ---- the C entry point's input errors (all are found before the device is touched)
def _call(ode, mode, blocked, traj, nnodes, opt=None):
    traj = np.ascontiguousarray(traj, dtype=np.float64)
    n = max(nnodes, 2)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    outs = [np.full(n + 1, -7.0), np.full((n + 1) * 8, -7.0), np.full((n + 1) * 8, -7.0), np.full(n + 1, -7.0), np.full(n + 1, -7.0),
            np.full(n * 8, -7.0)]
    ints = [np.full(n * 2, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)]
    rc = _lib.lib().asset_hip_mesh_error_integrator(ode.encode(), mode, int(blocked), traj.ctypes.data_as(dp), nnodes,
                                                    C.byref(opt) if opt is not None else None, *[a.ctypes.data_as(dp) for a in outs],
                                                    *[a.ctypes.data_as(ip) for a in ints], 0)
    return rc, _lib.lib().asset_hip_last_error().decode(errors="replace"), outs + ints


def _opts(**kw):
    d = dict(def_step=0.01, min_step=1e-6, max_step=100.0, max_step_change=3.0, adaptive=1, max_steps=100000)
    d.update(kw)
    return _lib.IntegOptions(d["def_step"], d["min_step"], d["max_step"], d["max_step_change"], d["adaptive"], d["max_steps"], None, None)


INPUT_ERRORS = [
    ("no block", dict(nnodes=1), "nb >= 1"),
    ("a node count that is not nb (cs - 1) + 1", dict(nnodes=12), "nb*(cs-1)+1"),
    ("an unknown ODE", dict(ode="no_such_ode"), "no_such_ode"),
    ("duplicate times", dict(edit=lambda t: t.__setitem__((4, 5), t[3, 5])), "duplicate times"),
    ("non-monotonic times", dict(edit=lambda t: t.__setitem__((4, 5), t[2, 5])), "not monotonic"),
    ("a NaN time", dict(edit=lambda t: t.__setitem__((4, 5), np.nan)), "not monotonic"),
    ("a zero default step", dict(opt=dict(def_step=0.0, min_step=0.0)), "positive"),
    ("a negative minimum step", dict(opt=dict(min_step=-1e-6)), "positive"),
    ("min > def", dict(opt=dict(min_step=0.1)), "min <= def <= max"),
    ("def > max", dict(opt=dict(max_step=0.001)), "min <= def <= max"),
    ("max_steps 0", dict(opt=dict(max_steps=0)), "max_steps"),
]


@pytest.mark.parametrize("what,change,word", INPUT_ERRORS, ids=[e[0] for e in INPUT_ERRORS])
def test_input_errors_are_statuses_with_a_message_and_nothing_is_written(what, change, word):
    traj = ick.ragged_traj("reentry", "LGL7", 4, seed=3, T=1.0)                       # 13 nodes
    if "edit" in change:
        change["edit"](traj)
    rc, msg, out = _call(change.get("ode", "reentry"), _lib.MODES["LGL7"], 0, traj, change.get("nnodes", 13),
                         _opts(**change["opt"]) if "opt" in change else None)
    assert rc != 0 and word in msg, (what, rc, msg)
    assert all(np.all(o == -7) for o in out), what


def test_valid_input_gets_as_far_as_the_device():
    traj = ick.ragged_traj("reentry", "LGL7", 4, seed=3, T=1.0)
    rc, msg, out = _call("reentry", _lib.MODES["LGL7"], 0, traj, 13, _opts())
    if os.path.exists("/dev/kfd"):
        assert rc == 0 and not np.any(out[0][:5] == -7.0)
    else:
        assert rc != 0 and "no HIP device visible" in msg and all(np.all(o == -7) for o in out)


# ---- run-time compiled ODEs get the kernels
def test_run_time_module_holds_the_integrator_kernels(monkeypatch):
    monkeypatch.delenv("ASSET_HIP_JIT", raising=False)
    ode = make_vanderpol()
    name = jit.ensure_kernel(ode, "LGL7", False, compile_only=True)
    mods = glob.glob(os.path.join(jit.JIT_DIR, name, "module_lgl7_0_*.rtc"))
    assert len(mods) == 1
    head = open(mods[0], "rb").read(1 << 16).split(b"\n")
    names = head[2:2 + int(head[1])]
    assert any(b"integ_reintegrate_kernel" in ln and name.encode() in ln for ln in names)
    assert any(b"integ_mesh_error_kernel" in ln for ln in names)
    L = _lib.lib()
    slots = {}
    s = 0
    while L.asset_hip_kernel_slot_name(s) is not None:
        slots[L.asset_hip_kernel_slot_name(s).decode()] = s
        s += 1
    assert "K_INTEG_STEP" in slots and "K_INTEG_ERROR" in slots
    assert L.asset_hip_kernel_slot_kinds(slots["K_INTEG_STEP"]) == 1 and L.asset_hip_kernel_slot_kinds(slots["K_INTEG_ERROR"]) == 1
