"""The batched propagation (csrc/propagate_kernels.h, csrc/capi/propagate_plan.h, asset_hip_propagate*, asset_asrl_amd/integrator.py) as
far as it can be checked without a GPU: the launch plan covers every (problem, column) pair exactly once, the C entry points' input
errors, the argument handling of ``ode.integrator``, that exactly one run-time module of an ODE holds the three kernels, and the
conditions the bounds of tests/propagate_checker.py rest on, against the 50-digit fixture.  The device itself:
tests/test_gpu_propagate.py."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import propagate_checker as pck
from asset_asrl_amd import _lib, jit, mesh
from asset_asrl_amd.integrator import Integrator
from asset_asrl_amd.ode import ShuttleReentry
from helpers import make_vanderpol

LDS_BUDGET = 48 * 1024            # csrc/capi/propagate_plan.h: PROP_LDS_BUDGET


# ---- launch plan
def _pairs_covered(p, m, C):
    """count[m, max(C, 1)] of how often the plan's lanes serve each (problem, column) pair."""
    wg, lane, ps = np.meshgrid(np.arange(p["grid"]), np.arange(p["lanes"]), np.arange(p["passes"]), indexing="ij")
    prob = wg * p["problems_per_wg"] + lane // p["group"]
    col = ps * p["group"] + lane % p["group"]
    ok = (prob < m) & (col < max(C, 1))
    count = np.zeros((m, max(C, 1)), dtype=np.int64)
    np.add.at(count, (prob[ok], col[ok]), 1)
    return count


@pytest.mark.parametrize("stm", [0, 1])
def test_launch_plan_covers_every_problem_and_column_exactly_once(stm):
    for n in range(1, 33):
        for uv in range(5):
            for pv in range(4):
                for m in (1, 2, 63, 64, 65, 1000):
                    p = _lib.propagate_plan(n, uv, pv, m, stm)
                    what = (n, uv, pv, m, stm, p)
                    C_ = n + uv + pv if stm else 0
                    G = p["group"]
                    assert 1 <= G <= 64 and G & (G - 1) == 0, what
                    assert 1 <= p["lanes"] <= 64 and p["lanes"] % G == 0 and p["problems_per_wg"] == p["lanes"] // G, what
                    assert p["columns"] == C_ and p["passes"] == (max(C_, 1) + G - 1) // G, what
                    assert p["grid"] == (m + p["problems_per_wg"] - 1) // p["problems_per_wg"], what
                    assert 0 < p["lds_bytes"] <= LDS_BUDGET, what
                    assert p["lds_bytes"] == 13 * n * 8 * (p["lanes"] + (p["problems_per_wg"] if stm else 0)), what
                    if stm:
                        assert G == min(1 << (C_ - 1).bit_length(), p["lanes"]), what      # the power of two that holds C, or the workgroup
                    if m <= 65 or (uv, pv) in ((0, 0), (4, 3)):
                        assert (_pairs_covered(p, m, C_) == 1).all(), what


def test_launch_plan_of_the_shapes_the_gpu_tests_use():
    for (n, uv, pv), want in (((5, 2, 0), dict(group=8, lanes=64, passes=1, problems_per_wg=8)),
                              ((6, 3, 0), dict(group=16, lanes=64, passes=1, problems_per_wg=4)),
                              ((32, 0, 0), dict(group=8, lanes=8, passes=4, problems_per_wg=1))):
        p = _lib.propagate_plan(n, uv, pv, 10, True)
        assert {k: p[k] for k in want} == want, (n, uv, pv, p)
    assert _lib.propagate_plan(5, 2, 0, 200, False)["lanes"] == 64 and _lib.propagate_plan(32, 0, 0, 2, False)["lanes"] == 8
    out = (C.c_longlong * 7)()
    assert _lib.lib().asset_hip_propagate_plan(0, 0, 0, 1, 0, out) == -1 and _lib.lib().asset_hip_propagate_plan(3, 0, 0, 0, 1, out) == -1
    assert _lib.lib().asset_hip_propagate_plan(3, 0, 0, 1, 1, None) == -1


# ---- the C entry points' input errors (all are found before the device is touched)
def _opts(**kw):
    d = dict(def_step=0.01, min_step=1e-6, max_step=100.0, max_step_change=3.0, adaptive=1, max_steps=100000)
    d.update(kw)
    return _lib.IntegOptions(d["def_step"], d["min_step"], d["max_step"], d["max_step_change"], d["adaptive"], d["max_steps"], None, None)


def _call(stm, ode="reentry", m=3, ns=1, opt=None, tf_edit=None, null=None):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rng = np.random.default_rng(5)
    y0 = rng.uniform(0.5, 1.0, (max(m, 1), 8))
    tf = y0[:, 5] + 0.1
    if tf_edit is not None:
        tf[1] = tf_edit
    outs = dict(xs=np.full(max(m, 1) * max(ns, 1) * 5, -7.0), jac=np.full(max(m, 1) * 5 * 9, -7.0),
                steps=np.full(max(m, 1) * 2, -7, dtype=np.int32), status=np.full(max(m, 1), -7, dtype=np.int32))
    a = dict(y0=y0.ctypes.data_as(dp), tf=tf.ctypes.data_as(dp), xs=outs["xs"].ctypes.data_as(dp), jac=outs["jac"].ctypes.data_as(dp),
             steps=outs["steps"].ctypes.data_as(ip), status=outs["status"].ctypes.data_as(ip))
    if null:
        a[null] = None
    o = C.byref(opt) if opt is not None else None
    L = _lib.lib()
    if stm:
        rc = L.asset_hip_propagate_stm(ode.encode() if ode else None, a["y0"], m, a["tf"], o, a["xs"], a["jac"], a["steps"], a["status"], 0)
    else:
        rc = L.asset_hip_propagate(ode.encode() if ode else None, a["y0"], m, a["tf"], ns, o, a["xs"], a["steps"], a["status"], 0)
    return rc, L.asset_hip_last_error().decode(errors="replace"), list(outs.values())


EINVAL, ENOODE, ENODEV = -1, -2, -3
INPUT_ERRORS = [
    ("a null ODE name", dict(ode=None), EINVAL, "null"),
    ("null initial rows", dict(null="y0"), EINVAL, "null"),
    ("null final times", dict(null="tf"), EINVAL, "null"),
    ("null states", dict(null="xs"), EINVAL, "null"),
    ("no problem", dict(m=0), EINVAL, "m must be"),
    ("a negative count", dict(m=-4), EINVAL, "m must be"),
    ("an unknown ODE", dict(ode="no_such_ode"), ENOODE, "no_such_ode"),
    ("a NaN final time", dict(tf_edit=np.nan), EINVAL, "not finite (problem 1)"),
    ("an infinite final time", dict(tf_edit=np.inf), EINVAL, "not finite"),
    ("a zero default step", dict(opt=dict(def_step=0.0, min_step=0.0)), EINVAL, "positive"),
    ("a negative minimum step", dict(opt=dict(min_step=-1e-6)), EINVAL, "positive"),
    ("min > def", dict(opt=dict(min_step=0.1)), EINVAL, "min <= def <= max"),
    ("def > max", dict(opt=dict(max_step=0.001)), EINVAL, "min <= def <= max"),
    ("a zero max_step_change", dict(opt=dict(max_step_change=0.0)), EINVAL, "max_step_change"),
    ("max_steps 0", dict(opt=dict(max_steps=0)), EINVAL, "max_steps"),
]


@pytest.mark.parametrize("stm", [False, True], ids=["propagate", "propagate_stm"])
@pytest.mark.parametrize("what,change,code,word", INPUT_ERRORS, ids=[e[0] for e in INPUT_ERRORS])
def test_input_errors_are_statuses_with_a_message_and_nothing_is_written(what, change, code, word, stm):
    kw = dict(change)
    if "opt" in kw:
        kw["opt"] = _opts(**kw["opt"])
    rc, msg, out = _call(stm, **kw)
    assert rc == code and word in msg, (what, rc, msg)
    assert all(np.all(o == -7) for o in out), what


def test_entry_point_specific_input_errors():
    rc, msg, out = _call(False, ns=0)
    assert rc == EINVAL and "ns must be" in msg and all(np.all(o == -7) for o in out)
    rc, msg, out = _call(True, null="jac")
    assert rc == EINVAL and "null" in msg and all(np.all(o == -7) for o in out)
    # a name that differs from a registered one by a trailing blank is another name
    rc, msg, _ = _call(False, ode="reentry ")
    assert rc == ENOODE


@pytest.mark.parametrize("stm", [False, True], ids=["propagate", "propagate_stm"])
def test_valid_input_gets_as_far_as_the_device(stm):
    rc, msg, out = _call(stm, opt=_opts())
    if os.path.exists("/dev/kfd"):
        assert rc == 0 and not np.any(out[0] == -7.0)
    else:
        assert rc == ENODEV and "no HIP device visible" in msg and all(np.all(o == -7) for o in out)


# ---- ode.integrator
def test_integrator_method_names_and_defaults():
    ode = ShuttleReentry()
    a, b, c = ode.integrator(0.05), ode.integrator("DOPRI87", 0.05), ode.integrator("DP87", 0.05)
    for g in (a, b, c):
        assert isinstance(g, Integrator) and isinstance(g, mesh.IntegratorOptions)
        assert (g.DefStepSize, g.MinStepSize, g.MaxStepSize, g.MaxStepChange, g.Adaptive) == (0.05, 0.05 / 10000, 0.05 * 10000, 3.0, True)
        assert np.array_equal(g.AbsTols, np.full(5, 1e-12)) and np.array_equal(g.RelTols, np.zeros(5))
    a.setAbsTol(1e-9)
    a.setStepSizes(0.1, 0.001, 10.0)
    assert a.AbsTols[3] == 1e-9 and a._c()[0].def_step == 0.1
    with pytest.raises(NotImplementedError, match="DOPRI54"):
        ode.integrator("DOPRI54", 0.05)
    with pytest.raises(ValueError, match="Unknown integration method"):
        ode.integrator("RK4", 0.05)
    with pytest.raises(TypeError):
        ode.integrator()
    with pytest.raises(TypeError):
        ode.integrator("DOPRI87")
    with pytest.raises(ValueError, match="greater than minimum"):
        a.setStepSizes(0.1, 0.2, 1.0)


def test_integrator_checks_row_width_and_the_number_of_final_times():
    g = ShuttleReentry().integrator(0.05)
    row = np.linspace(0.1, 0.8, 8)
    for call in (lambda: g.integrate(row[:7], 1.0), lambda: g.integrate_stm(np.append(row, 1.0), 1.0),
                 lambda: g.integrate_parallel(np.ones((3, 5)), [1.0, 1.0, 1.0]), lambda: g.integrate_dense(row[:6], 1.0, 4)):
        with pytest.raises(ValueError, match=r"8 columns \[x,t,u,p\]"):
            call()
    for call in (lambda: g.integrate_parallel([row, row], [1.0]), lambda: g.integrate_stm_parallel([row], [1.0, 2.0]),
                 lambda: g.integrate_dense_parallel([row, row, row], [1.0, 2.0], 5)):
        with pytest.raises(ValueError, match="final times"):
            call()
    with pytest.raises(ValueError, match="at least two rows"):
        g.integrate_dense(row, 1.0, 1)
    if not os.path.exists("/dev/kfd"):                                                # no CPU fallback
        with pytest.raises(_lib.AssetHipError, match="no HIP device visible"):
            g.integrate(row, 1.0)


# ---- run-time compiled ODEs: ONE module holds the kernels
def _module_names(name, tag):
    mods = glob.glob(os.path.join(jit.JIT_DIR, name, f"module_{tag}_*.rtc"))
    assert len(mods) == 1, mods
    head = open(mods[0], "rb").read(1 << 16).split(b"\n")
    return head[2:2 + int(head[1])]


def test_only_the_lgl3_module_of_a_user_ode_holds_the_propagation_kernels(monkeypatch):
    monkeypatch.delenv("ASSET_HIP_JIT", raising=False)
    ode = make_vanderpol()
    name = jit.ensure_kernel(ode, "LGL3", False, compile_only=True)
    jit.ensure_kernel(ode, "LGL5", False, compile_only=True)
    jit.ensure_kernel(ode, "LGL3", True, compile_only=True)
    home, lgl5, blocked = _module_names(name, "lgl3_0"), _module_names(name, "lgl5_0"), _module_names(name, "lgl3_1")
    for kernel in (b"prop_batch_kernel", b"prop_stm_kernel", b"prop_stm_jac_kernel"):
        assert any(kernel in ln and name.encode() in ln for ln in home), kernel
        assert not any(kernel in ln for ln in lgl5) and not any(kernel in ln for ln in blocked), kernel
    L = _lib.lib()
    slots, s = {}, 0
    while L.asset_hip_kernel_slot_name(s) is not None:
        slots[L.asset_hip_kernel_slot_name(s).decode()] = s
        s += 1
    for k in ("K_PROP_BATCH", "K_PROP_STM", "K_PROP_JAC"):
        assert L.asset_hip_kernel_slot_kinds(slots[k]) == 1, k


# ---- the checker against the 50-digit fixture (test infrastructure only)
def test_fixture_holds_the_cases_and_its_own_convergence():
    meta, cases = pck.fixture()
    assert 9 <= len(cases) <= 16 and os.path.getsize(pck.FIXTURE) < 512 * 1024
    assert all(c["convergence"] < 1e-25 for c in cases.values())
    odes = {c["ode"] for c in cases.values()}
    assert odes >= {"twobody_lt", "reentry", "vanderpol", "shape_5_3_2", "shape_1_0_0", "synthetic32"}
    for fam in ("twobody_lt", "reentry", "vanderpol", "shape_5_3_2", "synthetic32"):
        assert any(c["ode"] == fam and c["ns"] == 9 for c in cases.values()), fam
    assert any((c["tfs"] < c["rows"][:, c["sizes"][0]]).any() for c in cases.values())              # backward in time
    assert sum(c["options"].get("adaptive") is False for c in cases.values()) == 1
    s5 = cases["shape_5_3_2_dense"]["rows"]
    assert np.all(s5[:, 6:] != 0.0)                                                                # controls and parameters held non-zero
    assert cases["synthetic32_dense"]["m"] == 2 and np.abs(cases["kepler_full"]["rows"][0, 7:]).max() == 0.0


@pytest.mark.parametrize("name", pck.case_names())
def test_restatement_meets_the_conditions_of_the_bounds(oracle, name):
    """Regenerated in memory, the float64 restatement reproduces what the fixture records (step counts exactly, states and S to rounding of
    the recorded float64), stays within B / 4 of the 50-digit states on every adaptive case, and its S within the recorded eS."""
    c = pck.fixture()[1][name]
    r = pck.restate_case(oracle, c)
    for a in ("steps64", "steps64_end", "steps64_stm"):
        np.testing.assert_array_equal(r[a], c[a], err_msg=a)
    np.testing.assert_array_equal(r["x64"], c["x64"])
    np.testing.assert_array_equal(r["S64"], c["S64"])
    np.testing.assert_array_equal(r["eS"], c["eS"])
    used = pck.check_restatement(c, r)
    opt = pck.case_options(c)
    if opt["adaptive"]:
        assert (np.abs(r["S64"] - c["S_exact"]).max(axis=(1, 2)) <= c["eS"]).all()
        print(f"{name}: restatement uses {used} of B / 4; eS {c['eS'].max():.3e}; steps {c['steps64'].sum(axis=0)}")
    else:
        np.testing.assert_array_equal(r["d64"], c["d64"])
        np.testing.assert_array_equal(r["dS64"], c["dS64"])
        H = c["tfs"] - c["rows"][:, c["sizes"][0]]
        numsteps = (np.abs(H / opt["def_step"])).astype(int) + 1
        np.testing.assert_array_equal(c["steps64_end"], np.column_stack([numsteps + 1, 0 * numsteps]))


def test_kepler_full_revolution_returns_to_its_start(oracle):
    """A known answer that owes nothing to the extrapolation: after one period the two-body state is x0 again."""
    c = pck.fixture()[1]["kepler_full"]
    x0 = c["rows"][:, :6]
    B = pck.state_bound(c["S_max"], c["steps64"][:, 0], pck.case_options(c)["abs_tol"])
    pck.compare(c["x_exact"][:, -1], x0, 64 * pck.U * np.abs(c["S_max"]).sum(axis=2), "50-digit end state against x0 (tf rounded to float64)")
    pck.compare(c["x64"][:, -1], x0, B, "float64 restatement, dense, against x0")
    pck.compare(c["x64_end"], x0, pck.state_bound(c["S_max"], c["steps64_end"][:, 0], pck.case_options(c)["abs_tol"]),
                "float64 restatement, ns = 1, against x0")


def test_restatement_copies_the_state_at_an_output_time_it_has_already_reached(oracle):
    """|H| / (ns - 1) below the spacing of doubles at t0: neighbouring output times round to the same double.  Such a sample is the
    state as it is -- a step of size 0 would make the controller divide by a zero error estimate."""
    f, fj = pck.oracle_f(oracle, "shape_1_0_0"), pck.oracle_fj(oracle, "shape_1_0_0")
    row = np.array([0.7, 1.0])
    tf = 1.0 + 4 * np.spacing(1.0)
    times = pck.sample_times(row[1], tf, 9)
    assert len(np.unique(times)) < 9 and times[-1] == tf
    import integ_checker as gck
    r = pck.propagate(f, fj, row, tf, 9, gck.options())
    assert r["status"] == 0 and np.isfinite(r["xs"]).all() and r["steps"][0] == len(np.unique(times)) - 1
    assert np.abs(r["xs"] - 0.7).max() < 1e-14
