"""Everything about the propagation with a controller that needs no device: the constructor forms of ``ode.integrator`` and their
argument errors, what a controller module holds (cross-compiled for gfx950 and registered without a device), the input errors of
asset_hip_propagate_ctrl* -- all found before the device is touched --, the reference of tests/controller_checker.py against the
50-digit fixture and against central differences, and the launch plan of a controlled problem's STM."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import controller_cases as cc
import controller_checker as cck
import propagate_checker as pck
from asset_asrl_amd import _lib, jit, vf

EINVAL, ENOODE, ENODEV = -1, -2, -3


# ---- ode.integrator: constructor forms and their errors
def test_constructor_forms():
    ode = cc.make_ode("vanderpol")
    ucon, varlocs = cc.law("vdp_fb")
    for g in (ode.integrator(0.1, ucon, varlocs), ode.integrator("DOPRI87", 0.1, ucon, varlocs), ode.integrator(0.1, ucon, tuple(varlocs)),
              ode.integrator(0.1, ucon, np.array(varlocs))):
        assert g.controller[0] == "law" and g.controller[1] is ucon and g.controller[2] == [1, 2] and g.DefStepSize == 0.1 and g.method == "DOPRI87"
    g = ode.integrator(0.1, cc.law("vdp_pass")[0], 4)                                  # (varlocs as an int)
    assert g.controller[2] == [4]
    for v, want in ((0.25, [0.25]), ([0.5], [0.5]), (np.array([-1.0]), [-1.0]), (3, [3.0])):
        g = ode.integrator(0.1, v)
        assert g.controller[0] == "constant" and g.controller[1].tolist() == want
    assert ode.integrator("DP87", 0.1, 0.25).controller[0] == "constant"
    assert ode.integrator(0.1).controller is None and ode.integrator("DOPRI87", 0.1).controller is None
    tb = cc.make_ode("twobody_lt").integrator(0.1, vf.Arguments(3).normalized() * 0.01, [3, 4, 5])   # (the textbook call)
    assert tb.controller[2] == [3, 4, 5]
    assert cc.make_ode("twobody_lt").integrator(0.1, [0.0, 0.01, 0.0]).controller[1].tolist() == [0.0, 0.01, 0.0]


def test_constructor_errors_are_raised_before_any_device_work(monkeypatch):
    monkeypatch.setattr(jit, "ensure_controller_module", lambda *a, **k: pytest.fail("a module was asked for"))
    ode = cc.make_ode("vanderpol")                                                     # rows [x0, x1, t, u, mu]
    ucon, varlocs = cc.law("vdp_fb")
    a2 = vf.Arguments(2)
    for args, word in (((0.1, ucon, [1]), "2 inputs"), ((0.1, ucon, [0, 1, 2]), "2 inputs"),
                       ((0.1, vf.stack([a2[0], a2[1]]), [1, 2]), "2 outputs"),
                       ((0.1, ucon, [1, 5]), "out of range"), ((0.1, ucon, [-1, 2]), "out of range"), ((0.1, ucon, [1, 1]), "repeats"),
                       ((0.1, ucon, [1, 3]), "inside the control slots"), ((0.1, ucon, [1.5, 2]), "sequence of ints"),
                       ((0.1, [1.0, 2.0]), "2 values")):
        with pytest.raises(ValueError, match=word):
            ode.integrator(*args)
    from helpers import make_shape                                                     # (an ODE without controls)
    for args in ((0.1, vf.Arguments(1)[0], [0]), (0.1, 0.5)):
        with pytest.raises(ValueError, match="UV == 0"):
            make_shape(1, 0, 0).integrator(*args)
    table = object()                                                                   # (a trajectory table of whatever class, or its rows)
    for args in ((0.1, table), (0.1, table, [3]), (0.1, np.zeros((4, 5))), (0.1, np.zeros((4, 5)), [3]), ("DOPRI87", 0.1, table)):
        with pytest.raises(NotImplementedError, match="trajectory-table controller.*InterpTable1D"):
            ode.integrator(*args)
    with pytest.raises(TypeError):
        ode.integrator(0.1, ucon)
    with pytest.raises(TypeError):
        ode.integrator(0.1, ucon, varlocs, 7)
    g = ode.integrator(0.1, ucon, varlocs)
    row, ev = [1.0, 0.0, 0.0, 0.1, 1.0], [(vf.Arguments(5)[1] * 1.0, 0, 0)]
    for call in (lambda: g.integrate(row, 1.0, ev), lambda: g.integrate_parallel([row], [1.0], ev), lambda: g.integrate_parallel([row], [1.0], events=ev)):
        with pytest.raises(NotImplementedError, match="events with a controller"):
            call()
    for call in (lambda: g.integrate_dense(row, 1.0, 5, events=ev), lambda: g.integrate_stm(row, 1.0, events=ev)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match=r"5 columns \[x,t,u,p\]"):
        g.integrate(row[:4], 1.0)


def test_the_constant_controller_writes_the_rows_and_takes_the_held_control_path(monkeypatch):
    ode = cc.make_ode("vanderpol")
    g = ode.integrator(0.1, 0.25)
    seen = []
    monkeypatch.setattr(g, "_propagate", lambda Y, T, ns: seen.append((Y.copy(), ns)) or (np.zeros((2, ns, 2)), np.zeros((2, 2), dtype=np.int32),
                                                                                         np.zeros(2, dtype=np.int32)))
    monkeypatch.setattr(g, "_propagate_ctrl", lambda *a: pytest.fail("the controller kernels"))
    rows = np.array([[1.0, 0.0, 0.0, 9.0, 1.0], [0.5, 0.1, 0.2, -9.0, 0.7]])
    out = g.integrate_parallel(rows, [1.0, 1.2])
    g.integrate_dense_parallel(rows, [1.0, 1.2], 3)
    assert [s[1] for s in seen] == [1, 3] and all(np.array_equal(s[0][:, 3], [0.25, 0.25]) for s in seen)
    assert np.array_equal(seen[0][0][:, [0, 1, 2, 4]], rows[:, [0, 1, 2, 4]]) and rows[0, 3] == 9.0, "the caller's rows are not written"
    assert [r[3] for r in out] == [0.25, 0.25]


def test_rows_are_filled_from_the_controls_the_kernels_return(monkeypatch):
    g = cc.integrator("vdp_fb", 0.1)
    rows, tfs = np.array([[1.0, 0.0, 0.0, 9.0, 1.0], [0.5, 0.1, 0.2, -9.0, 0.7]]), np.array([1.0, 1.2])

    def fake(Y, T, ns):
        assert np.array_equal(Y, rows)
        return (np.full((2, ns, 2), 3.0), np.arange(2 * ns, dtype=float).reshape(2, ns, 1) + 0.5, np.zeros((2, 2), dtype=np.int32),
                np.zeros(2, dtype=np.int32))
    monkeypatch.setattr(g, "_propagate_ctrl", fake)
    monkeypatch.setattr(g, "_propagate", lambda *a: pytest.fail("the held-control kernels"))
    end = np.array(g.integrate_parallel(rows, tfs))
    assert end[:, 3].tolist() == [0.5, 1.5] and end[:, 2].tolist() == [1.0, 1.2] and end[:, 4].tolist() == [1.0, 0.7] and (end[:, :2] == 3.0).all()
    dense = np.array(g.integrate_dense_parallel(rows, tfs, 3))
    assert dense[:, :, 3].tolist() == [[0.5, 1.5, 2.5], [3.5, 4.5, 5.5]] and np.array_equal(dense[1, :, 2], pck.sample_times(0.2, 1.2, 3))


# ---- the module
def _module_files(name):
    return glob.glob(os.path.join(jit.JIT_DIR, name, "module_ctrl_0_*.rtc"))


def _module_names(name):
    mods = _module_files(name)
    assert len(mods) == 1, mods
    head = open(mods[0], "rb").read(1 << 16).split(b"\n")
    return head[2:2 + int(head[1])]


def test_a_controller_module_cross_compiles_and_holds_the_three_kernels(monkeypatch):
    monkeypatch.delenv("ASSET_HIP_JIT", raising=False)
    ode = cc.make_ode("vanderpol")
    name = jit.ensure_controller_module(ode, *cc.law("vdp_fb"), compile_only=True)
    names = _module_names(name)
    assert len(names) == 3 and all(jit.device_name(ode).encode() in ln and name.encode() in ln for ln in names)
    assert [sum(k in ln for ln in names) for k in (b"prop_ctrl_batch_kernel", b"prop_ctrl_stm_kernel", b"prop_ctrl_jac_kernel")] == [1, 1, 1]
    meta = (C.c_longlong * 64)()
    assert _lib.lib().asset_hip_rtc_module_meta(_module_files(name)[0].encode(), meta, 64) == 42 and list(meta[:8]) == [5, 2, 1, 1, 0, 0, 5, 1]
    # the same mathematics under fresh objects is the same module; another law or other varlocs are another
    a = vf.Arguments(2)
    from helpers import make_vanderpol
    assert jit.ensure_controller_module(make_vanderpol(), -0.5 * (vf.tanh(a[0]) * vf.cos(a[1])), [1, 2], compile_only=True) == name
    assert len(_module_files(name)) == 1
    assert jit.ensure_controller_module(ode, cc.law("vdp_fb")[0], [0, 2], compile_only=True) != name
    assert jit.ensure_controller_module(ode, *cc.law("vdp_pass"), compile_only=True) != name
    monkeypatch.setenv("ASSET_HIP_JIT", "hipcc")
    with pytest.raises(_lib.AssetHipError, match="compiled in process"):
        jit.ensure_controller_module(ode, *cc.law("vdp_fb"), compile_only=True)
    L = _lib.lib()
    slots, s = {}, 0
    while L.asset_hip_kernel_slot_name(s) is not None:
        slots[L.asset_hip_kernel_slot_name(s).decode()] = s
        s += 1
    assert all(L.asset_hip_kernel_slot_kinds(slots[k]) == 16 for k in ("K_PROP_CTRL_BATCH", "K_PROP_CTRL_STM", "K_PROP_CTRL_JAC"))   # (kind 5 only)


@pytest.fixture(scope="module")
def module():
    """vanderpol under vdp_fb (pre-built: controller_cases.LAWS), registered WITHOUT a device"""
    mp = pytest.MonkeyPatch()
    mp.delenv("ASSET_HIP_JIT", raising=False)
    try:
        yield jit.ensure_controller_module(cc.make_ode("vanderpol"), *cc.law("vdp_fb"), compile_only=False)
    finally:
        mp.undo()


def test_the_sizes_of_a_module_are_read_without_a_device(module):
    L = _lib.lib()
    v = [C.c_int32(-1) for _ in range(3)]
    assert L.asset_hip_controller_module_sizes(module.encode(), *[C.byref(x) for x in v]) == 0 and [x.value for x in v] == [2, 1, 1]
    assert L.asset_hip_controller_module_sizes(module.encode(), None, None, None) == 0
    assert L.asset_hip_controller_module_sizes(b"reentry", None, None, None) == ENOODE
    assert L.asset_hip_controller_module_sizes(None, None, None, None) == EINVAL
    assert L.asset_hip_event_module_sizes(module.encode(), None, None, None, None) == ENOODE, "a controller module is not an event module"


def _opts(**kw):
    d = dict(def_step=0.01, min_step=1e-6, max_step=100.0, max_step_change=3.0, adaptive=1, max_steps=100000)
    d.update(kw)
    return _lib.IntegOptions(d["def_step"], d["min_step"], d["max_step"], d["max_step_change"], d["adaptive"], d["max_steps"], None, None)


def _call(module, entry="batch", name="", m=3, ns=2, opt=None, tf_edit=None, null=None):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    mm, nn = max(m, 1), max(ns, 1)
    y0 = np.random.default_rng(5).uniform(0.5, 1.0, (mm, 5))
    tf = y0[:, 2] + 0.1
    if tf_edit is not None:
        tf[1] = tf_edit
    outs = dict(xs=np.full(mm * nn * 2, -7.0), us=np.full(mm * nn, -7.0), jac=np.full(mm * 2 * 6, -7.0), steps=np.full(mm * 2, -7, dtype=np.int32),
                status=np.full(mm, -7, dtype=np.int32), last=np.full(mm * 2, -7.0))
    a = {k: v.ctypes.data_as(dp if v.dtype == np.float64 else ip) for k, v in outs.items()}
    a.update(y0=y0.ctypes.data_as(dp), tf=tf.ctypes.data_as(dp))
    if null:
        a[null] = None
    name = module if name == "" else name
    nm = name.encode() if name else None
    L = _lib.lib()
    o = C.byref(opt) if opt is not None else None
    if entry == "batch":
        rc = L.asset_hip_propagate_ctrl(nm, a["y0"], m, a["tf"], ns, o, a["xs"], a["us"], a["steps"], a["status"], 0)
    elif entry == "stm":
        rc = L.asset_hip_propagate_ctrl_stm(nm, a["y0"], m, a["tf"], o, a["xs"], a["us"], a["jac"], a["steps"], a["status"], 0)
    else:
        rc = L.asset_hip_propagate_ctrl_stm_lanes(nm, a["y0"], m, a["tf"], o, a["xs"], a["us"], a["jac"], a["steps"], a["status"], a["last"], 0)
    return rc, L.asset_hip_last_error().decode(errors="replace"), list(outs.values())


INPUT_ERRORS = [("a null module name", dict(name=None), EINVAL, "null")] + \
    [(f"null {k} ({e})", dict(null=k, entry=e), EINVAL, "null") for e in ("batch", "stm", "lanes") for k in ("y0", "tf", "xs", "us")] + \
    [(f"null jac ({e})", dict(null="jac", entry=e), EINVAL, "null") for e in ("stm", "lanes")] + [
    ("null xf_last", dict(null="last", entry="lanes"), EINVAL, "null"),
    ("no problem", dict(m=0), EINVAL, "m must be"),
    ("no sample", dict(ns=0), EINVAL, "ns must be"),
    ("an unknown module", dict(name="no_such_module"), ENOODE, "no controller module registered as 'no_such_module'"),
    ("an ODE's name is not a controller module", dict(name="reentry"), ENOODE, "'reentry' is not a controller module"),
    ("an ODE's name is not a controller module (stm)", dict(name="reentry", entry="stm"), ENOODE, "not a controller module"),
    ("a NaN final time", dict(tf_edit=np.nan), EINVAL, "not finite (problem 1)"),
    ("an infinite final time (stm)", dict(tf_edit=np.inf, entry="stm"), EINVAL, "not finite (problem 1)"),
    ("a zero default step", dict(opt=dict(def_step=0.0, min_step=0.0)), EINVAL, "positive"),
    ("min > def", dict(opt=dict(min_step=0.1)), EINVAL, "min <= def <= max"),
    ("a zero max_step_change", dict(opt=dict(max_step_change=0.0), entry="lanes"), EINVAL, "max_step_change"),
    ("max_steps 0", dict(opt=dict(max_steps=0)), EINVAL, "max_steps"),
]


@pytest.mark.parametrize("what,change,code,word", INPUT_ERRORS, ids=[e[0] for e in INPUT_ERRORS])
def test_input_errors_are_statuses_with_a_message_and_nothing_is_written(module, what, change, code, word):
    kw = dict(change)
    if "opt" in kw:
        kw["opt"] = _opts(**kw["opt"])
    rc, msg, out = _call(module, **kw)
    assert rc == code and word in msg, (what, rc, msg)
    assert all(np.all(o == -7) for o in out), what


def test_an_event_module_is_not_a_controller_module_and_a_controller_module_is_not_a_function(module):
    import event_cases
    ev = jit.ensure_event_module(event_cases.make_ode("vanderpol"), [event_cases.event_function("vanderpol", "x1")], compile_only=False)
    rc, msg, out = _call(module, name=ev)
    assert rc == ENOODE and "is not a controller module" in msg and all(np.all(o == -7) for o in out)
    from asset_asrl_amd.evaluator import DefectEvaluator
    with pytest.raises(_lib.AssetHipError, match="a controller module is launched through asset_hip_propagate_ctrl"):
        DefectEvaluator(module, "Function", False, np.zeros((1, 5), dtype=np.int32), np.zeros((1, 1), dtype=np.int32), 5, 1, device=0)


@pytest.mark.parametrize("entry", ["batch", "stm", "lanes"])
def test_valid_input_gets_as_far_as_the_device(module, entry):
    rc, msg, out = _call(module, entry=entry, opt=_opts())
    if os.path.exists("/dev/kfd"):
        assert rc == 0 and not np.any(out[0][:6] == -7.0)
    else:
        assert rc == ENODEV and "no HIP device visible" in msg and all(np.all(o == -7) for o in out)


def test_the_stm_plan_of_a_controlled_problem_has_no_control_columns():
    p = _lib.propagate_plan(16, 0, 2, 3, True)                                         # coupled16 under a law: C' = 18 columns
    assert p["group"] == 16 and p["passes"] == 2 and p["columns"] == 18
    assert _lib.propagate_plan(5, 0, 2, 9, True)["group"] == 8 and _lib.propagate_plan(8, 0, 1, 9, True)["group"] == 16
    assert _lib.propagate_plan(11, 4, 0, 33, False)["lanes"] == 32                     # (halved lanes of the batch kernel)


# ---- the reference
@pytest.mark.parametrize("name", sorted(cck.LAWS))
def test_closed_loop_jacobian_agrees_with_central_differences(oracle, name):
    system, varlocs, K, JK = cck.LAWS[name]
    n, uv, pv = cck.SIZES[system]
    N = n + 1 + uv + pv
    f_c, fj_c = cck.closed_loop_of(oracle, name)
    rng = np.random.default_rng(len(name))
    for _ in range(3):
        y = rng.uniform(0.3, 1.2, N)
        fv, J = fj_c(y)
        assert np.array_equal(fv, f_c(y)) and np.all(J[:, n + 1:n + 1 + uv] == 0.0)
        z = y.copy()
        z[n + 1:n + 1 + uv] = -55.0
        assert np.array_equal(f_c(z), fv), "the row's own controls are not read"
        h = 1.0e-6
        for i in range(N):
            e = np.zeros(N)
            e[i] = h
            fd = (f_c(y + e) - f_c(y - e)) / (2 * h)
            # central differences: h^2 |f'''| / 6 + u |f| / h, with |f|, |f'''| of order 1 .. 10 here
            assert np.allclose(J[:, i], fd, rtol=0.0, atol=2.0e-9 * max(1.0, np.abs(fv).max())), (name, i, J[:, i], fd)
        # the law's own Jacobian against central differences of the law
        zz = y[varlocs]
        for q in range(len(varlocs)):
            e = np.zeros(len(varlocs))
            e[q] = h
            assert np.allclose(JK(zz)[:, q], (K(zz + e) - K(zz - e)) / (2 * h), rtol=0.0, atol=2.0e-9)


def test_the_dsl_laws_are_the_checkers_laws():
    for name, (system, varlocs) in cc.LAWS.items():
        ucon, vl = cc.law(name)
        assert vl == cck.LAWS[name][1] == varlocs and system == cck.LAWS[name][0]
        z = np.random.default_rng(7).uniform(0.4, 1.1, len(vl))
        np.testing.assert_allclose(ucon.compute(z), cck.LAWS[name][2](z), rtol=1e-14, atol=0.0)


def test_fixture_holds_the_cases_the_issue_names():
    meta, cases = cck.fixture()
    assert meta["dps"] == 50 and os.path.getsize(cck.FIXTURE) < 200 * 1024
    assert sorted(cases) == ["pd", "pd_fixed", "vdp_fb"]
    pd, vdp, fx = cases["pd"], cases["vdp_fb"], cases["pd_fixed"]
    assert (pd["rows"].shape[0], pd["ns"], vdp["rows"].shape[0], vdp["ns"], fx["rows"].shape[0], fx["ns"]) == (5, 4, 3, 3, 3, 1)
    assert (pd["tfs"] > pd["rows"][:, 2]).any() and (pd["tfs"] < pd["rows"][:, 2]).any(), "both time directions"
    assert fx["options"]["adaptive"] is False and pd["options"].get("adaptive", True)
    for c in cases.values():
        assert np.abs(c["tfs"] - c["rows"][:, 2]).max() <= 0.5 and np.all(c["S_exact"][:, :, 2] == 0.0), "short arcs; zero u columns"
        assert c["S_exact"].shape == (c["rows"].shape[0], 2, 4) and c["x_exact"].shape == (c["rows"].shape[0], c["ns"], 2)


@pytest.mark.parametrize("name", cck.case_names())
def test_restatement_meets_the_fixture_and_the_quarter_of_every_bound(oracle, name):
    case = cck.fixture()[1][name]
    r = cck.restate_case(oracle, case)
    for a in ("x64", "x64_end", "S64", "steps64", "steps64_end", "eS"):
        assert np.array_equal(r[a], case[a]), f"{name}: the fixture's record of the restatement ({a})"
    used = cck.check_restatement(case, r, cck.closed_loop_of(oracle, case["law"])[0])
    print(f"{name}: fractions of the quarter bounds the float64 restatement uses: {used}")
    assert np.all(r["S64"][:, :, 2] == 0.0), "the restated u columns are exactly zero"
