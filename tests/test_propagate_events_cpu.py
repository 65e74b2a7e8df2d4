"""Everything about the propagation with events that needs no device: the checker of tests/event_checker.py against the 50-digit fixture
(test infrastructure only), the input errors of asset_hip_propagate_events -- all found before the device is touched, against a module
that is registered without one --, the argument errors of ``ode.integrator``'s event overloads, and what an event module holds."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import event_cases
import event_checker as eck
from asset_asrl_amd import _lib, jit
from helpers import make_vanderpol

EINVAL, ENOODE, ENODEV = -1, -2, -3


# ---- the checker against the fixture
def test_fixture_holds_the_cases_the_bounds_were_derived_for():
    meta, cases = eck.fixture()
    assert meta["digits"] == 50 and os.path.getsize(eck.FIXTURE) < 256 * 1024
    assert {c["system"] for c in cases.values()} == {"oscillator", "freefall", "twobody_lt", "vanderpol"}
    osc = [c for c in cases.values() if c["system"] == "oscillator"]
    assert {c["direction"][0] for c in osc} == {-1, 0, 1} and {c["stop"][0] for c in osc} >= {0, 1, 3}
    n_of = lambda c: eck.SYSTEMS[c["system"]]["n"]
    assert any((c["tfs"] < c["rows"][:, n_of(c)]).all() for c in cases.values()), "a case backward in time"
    assert {c["event_tol"] for c in cases.values()} == {1.0e-6, 1.0e-10}
    fall = cases["fall_impact"]
    assert np.allclose(fall["t_event"][:, 0, 0] - fall["rows"][:, 2], np.sqrt(2.0 * fall["rows"][:, 0] / fall["rows"][:, 3]), rtol=1e-15)
    assert np.unique(np.round(fall["t_event"][:, 0, 0], 3)).size == fall["rows"].shape[0], "another impact time in every lane"
    any_dir = cases["osc_any_stop0"]
    k = np.round((any_dir["t_event"][0, 0, :4] - np.pi / 2) / np.pi, 12)
    assert k.tolist() == [0.0, 1.0, 2.0, 3.0], "crossings at pi / 2 + k pi"
    for c in cases.values():
        assert c["S_max"].shape == (c["rows"].shape[0], n_of(c), n_of(c))


@pytest.mark.parametrize("name", eck.case_names())
def test_restatement_meets_the_fixture_and_the_conditions_of_the_bounds(name):
    case = eck.fixture()[1][name]
    res = eck.restate_case(case)
    assert all(r["status"] == 0 for r in res)
    assert np.array_equal([r["steps"][0] for r in res], case["accepted64"])
    eck.check_conditions(case, res)
    B = eck.state_bounds(case, case["accepted64"])
    eck.compare_case(case, eck.restatement_as_got(res), B, what="float64 restatement:")
    quarter = eck.restate_case(case, tol_factor=0.25)                                  # (tests/event_checker.py: QUARTER)
    eck.compare_case(case, eck.restatement_as_got(quarter), B, factor=0.25, what="float64 restatement at EventTol / 4, a quarter of the bounds:")


def test_longdouble_restatement_of_the_tight_case():
    case = eck.fixture()[1]["osc_tight_tol"]
    res = eck.restate_case(case, dtype=eck.LD)
    assert all(r["x"].dtype == eck.LD for r in res)
    eck.compare_case(case, eck.restatement_as_got(res), eck.state_bounds(case, case["accepted64"]), what="longdouble restatement:")


def test_restatement_ignores_a_value_that_is_exactly_zero_at_a_step_end():
    """g = x0 of a problem at rest in the origin is 0 at every step end: no occurrence, whatever the direction"""
    sysd = eck.SYSTEMS["oscillator"]
    r = eck.propagate_events(sysd["f"], [sysd["events"]["x0"][0]], [0.0, 0.0, 0.0], 5.0, [0], [1], eck.gck.options(def_step=0.1, max_step=1.0))
    assert r["count"] == [0] and r["stopped"] == -1 and r["status"] == 0 and r["t_end"] == 5.0


# ---- the C entry point's input errors
@pytest.fixture(scope="module")
def module():
    """vanderpol with two events (pre-built: event_cases.MODULES), registered WITHOUT a device"""
    mp = pytest.MonkeyPatch()
    mp.delenv("ASSET_HIP_JIT", raising=False)
    try:
        yield jit.ensure_event_module(event_cases.make_ode("vanderpol"), [event_cases.event_function("vanderpol", "x1"),
                                                                          event_cases.event_function("vanderpol", "pos")], compile_only=False)
    finally:
        mp.undo()


def _opts(**kw):
    d = dict(def_step=0.01, min_step=1e-6, max_step=100.0, max_step_change=3.0, adaptive=1, max_steps=100000)
    d.update(kw)
    return _lib.IntegOptions(d["def_step"], d["min_step"], d["max_step"], d["max_step_change"], d["adaptive"], d["max_steps"], None, None)


def _call(module, name="", m=3, ne=2, direction=(0, 1), stop=(0, 2), tol=1.0e-6, iters=10, locs=4, opt=None, tf_edit=None, null=None):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    mm, K = max(m, 1), max(locs, 1)
    y0 = np.random.default_rng(5).uniform(0.5, 1.0, (mm, 5))
    tf = y0[:, 2] + 0.1
    if tf_edit is not None:
        tf[1] = tf_edit
    d, s = np.array(direction, dtype=np.int32), np.array(stop, dtype=np.int32)
    outs = dict(xf=np.full(mm * 2, -7.0), t_end=np.full(mm, -7.0), stopped=np.full(mm, -7, dtype=np.int32), ev_count=np.full(mm * 2, -7, dtype=np.int32),
                ev_rows=np.full(mm * 2 * K * 3, -7.0), ev_resid=np.full(mm * 2 * K, -7.0), ev_conv=np.full(mm * 2 * K, -7, dtype=np.int32),
                steps=np.full(mm * 2, -7, dtype=np.int32), status=np.full(mm, -7, dtype=np.int32))
    a = {k: v.ctypes.data_as(dp if v.dtype == np.float64 else ip) for k, v in outs.items()}
    a.update(y0=y0.ctypes.data_as(dp), tf=tf.ctypes.data_as(dp), direction=d.ctypes.data_as(ip), stop=s.ctypes.data_as(ip))
    if null:
        a[null] = None
    name = module if name == "" else name
    L = _lib.lib()
    rc = L.asset_hip_propagate_events(name.encode() if name else None, a["y0"], m, a["tf"], C.byref(opt) if opt is not None else None, ne,
                                      a["direction"], a["stop"], tol, iters, locs, a["xf"], a["t_end"], a["stopped"], a["ev_count"], a["ev_rows"],
                                      a["ev_resid"], a["ev_conv"], a["steps"], a["status"], 0)
    return rc, L.asset_hip_last_error().decode(errors="replace"), list(outs.values())


INPUT_ERRORS = [("a null module name", dict(name=None), EINVAL, "null")] + \
    [(f"null {k}", dict(null=k), EINVAL, "null") for k in ("y0", "tf", "direction", "stop", "xf", "t_end", "stopped", "ev_count", "ev_rows",
                                                           "ev_resid", "ev_conv")] + [
    ("no problem", dict(m=0), EINVAL, "m must be"),
    ("an unknown module", dict(name="no_such_module"), ENOODE, "no_such_module"),
    ("an ODE's name is not an event module", dict(name="reentry"), ENOODE, "reentry"),
    ("one event for a module of two", dict(ne=1), EINVAL, "the module has 2 events"),
    ("three events for a module of two", dict(ne=3), EINVAL, "the module has 2 events"),
    ("direction 2", dict(direction=(0, 2)), EINVAL, "direction must be -1, 0 or 1 (event 1)"),
    ("direction -2", dict(direction=(-2, 0)), EINVAL, "direction must be -1, 0 or 1 (event 0)"),
    ("a negative stop", dict(stop=(0, -1)), EINVAL, "stop must not be negative (event 1)"),
    ("stop beyond max_locs", dict(stop=(5, 0)), EINVAL, "stop exceeds max_locs"),
    ("a zero event_tol", dict(tol=0.0), EINVAL, "event_tol"),
    ("a NaN event_tol", dict(tol=float("nan")), EINVAL, "event_tol"),
    ("no evaluation", dict(iters=0), EINVAL, "max_event_iters"),
    ("no stored occurrence", dict(locs=0, stop=(0, 0)), EINVAL, "max_locs"),
    ("a NaN final time", dict(tf_edit=np.nan), EINVAL, "not finite (problem 1)"),
    ("a zero default step", dict(opt=dict(def_step=0.0, min_step=0.0)), EINVAL, "positive"),
    ("min > def", dict(opt=dict(min_step=0.1)), EINVAL, "min <= def <= max"),
    ("a zero max_step_change", dict(opt=dict(max_step_change=0.0)), EINVAL, "max_step_change"),
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


def test_valid_input_gets_as_far_as_the_device(module):
    rc, msg, out = _call(module, opt=_opts())
    if os.path.exists("/dev/kfd"):
        assert rc == 0 and not any(np.any(o == -7) for o in out)
    else:
        assert rc == ENODEV and "no HIP device visible" in msg and all(np.all(o == -7) for o in out)


def test_the_sizes_of_a_module_are_read_without_a_device(module):
    v = [C.c_int32(-1) for _ in range(4)]
    assert _lib.lib().asset_hip_event_module_sizes(module.encode(), *[C.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [2, 1, 1, 2]
    assert _lib.lib().asset_hip_event_module_sizes(module.encode(), None, None, None, None) == 0
    assert _lib.lib().asset_hip_event_module_sizes(b"reentry", None, None, None, None) == ENOODE
    assert _lib.lib().asset_hip_event_module_sizes(None, None, None, None, None) == EINVAL


# ---- what a module holds
def _module_files(name, tag):
    return glob.glob(os.path.join(jit.JIT_DIR, name, f"module_{tag}_*.rtc"))


def _module_names(name, tag):
    mods = _module_files(name, tag)
    assert len(mods) == 1, mods
    head = open(mods[0], "rb").read(1 << 16).split(b"\n")
    return head[2:2 + int(head[1])]


def test_an_event_module_holds_one_kernel_of_the_ode_and_its_events(monkeypatch):
    monkeypatch.delenv("ASSET_HIP_JIT", raising=False)
    ode = make_vanderpol()
    funcs = [event_cases.event_function("vanderpol", "x1")]
    name = jit.ensure_event_module(ode, funcs, compile_only=True)
    names = _module_names(name, "events_0")
    assert len(names) == 1 and b"prop_event_kernel" in names[0] and jit.device_name(ode).encode() in names[0] and name.encode() in names[0]
    # the same mathematics under fresh objects is the same module; directions and stop counts are not part of it
    from asset_asrl_amd import vf
    again = jit.ensure_event_module(make_vanderpol(), [vf.Arguments(5)[1] * 1.0], compile_only=True)
    assert again == name and len(_module_files(name, "events_0")) == 1
    assert jit.ensure_event_module(ode, [event_cases.event_function("vanderpol", "pos")], compile_only=True) != name
    g = ode.integrator(0.1)
    seen = []
    monkeypatch.setattr(jit, "ensure_event_module", lambda o, f, compile_only=None: seen.append(list(f)) or name)
    monkeypatch.setattr(_lib.lib(), "asset_hip_propagate_events", lambda *a: seen.append(a[0]) or ENODEV, raising=False)
    for direction, stop in ((0, 0), (-1, 1), (1, 3)):
        with pytest.raises(_lib.AssetHipError):
            g.integrate([1.0, 0.0, 0.0, 0.1, 1.0], 1.0, [(funcs[0], direction, stop)])
    assert seen[0] == funcs and seen[1:] == [name.encode()] * 3, "one module, asked for once, for every direction / stop list"


def test_the_home_module_of_an_ode_names_the_three_propagation_kernels_it_named_before(monkeypatch):
    monkeypatch.delenv("ASSET_HIP_JIT", raising=False)
    ode = make_vanderpol()
    name = jit.ensure_kernel(ode, "LGL3", False, compile_only=True)
    prop = sorted(ln for ln in _module_names(name, "lgl3_0") if b"prop_" in ln)
    assert len(prop) == 3 and [any(k in ln for ln in prop) for k in (b"prop_batch_kernel", b"prop_stm_kernel", b"prop_stm_jac_kernel")] == [True] * 3
    assert not any(b"prop_event" in ln for ln in prop)
    L = _lib.lib()
    slots, s = {}, 0
    while L.asset_hip_kernel_slot_name(s) is not None:
        slots[L.asset_hip_kernel_slot_name(s).decode()] = s
        s += 1
    assert "K_PROP_EVENT" in slots and L.asset_hip_kernel_slot_kinds(slots["K_PROP_EVENT"]) == 8   # (bit 3: modules of kind 4 only)
    assert all(L.asset_hip_kernel_slot_kinds(slots[k]) == 1 for k in ("K_PROP_BATCH", "K_PROP_STM", "K_PROP_JAC"))


# ---- ode.integrator
def test_event_attributes_and_argument_errors(monkeypatch):
    from asset_asrl_amd import vf
    ode = make_vanderpol()
    g = ode.integrator(0.1)
    assert (g.EventTol, g.MaxEventIters, g.MaxEventLocs) == (1.0e-6, 10, 8)
    row, x1 = [1.0, 0.0, 0.0, 0.1, 1.0], event_cases.event_function("vanderpol", "x1")
    with pytest.raises(ValueError, match="has 3 inputs, the ODE's rows have 5"):
        g.integrate(row, 1.0, [(vf.Arguments(3)[0] * 1.0, 0, 0)])
    with pytest.raises(ValueError, match="not a scalar"):
        g.integrate(row, 1.0, [(vf.stack([x1, x1]), 0, 0)])
    for bad, word in (([(x1, 2, 0)], "direction"), ([(x1, 0, -1)], "stop count"), ([(x1, 0, 9)], "MaxEventLocs"), ([], "1..8 events"),
                      ([(x1, 0, 0)] * 9, "1..8 events"), ([(x1, 0)], r"\(g, direction, stop\)"), ([(x1, 0.5, 0)], "direction")):
        with pytest.raises(ValueError, match=word):
            g.integrate_parallel([row], [1.0], bad)
    g.EventTol = 0.0
    with pytest.raises(ValueError, match="EventTol"):
        g.integrate_parallel([row], [1.0], events=[(x1, 0, 0)])
    g.EventTol = 1.0e-6
    for call in (lambda: g.integrate_dense(row, 1.0, 5, events=[(x1, 0, 0)]),
                 lambda: g.integrate_dense_parallel([row], [1.0], 5, events=[(x1, 0, 0)]), lambda: g.integrate_stm(row, 1.0, events=[(x1, 0, 0)]),
                 lambda: g.integrate_stm_parallel([row], [1.0], events=[(x1, 0, 0)])):
        with pytest.raises(NotImplementedError, match="with events is not implemented"):
            call()
    # a list as the third argument means events, an int still means threads, and events may be given by keyword
    calls = []
    monkeypatch.setattr(g, "_propagate_events", lambda Y, T, ev, details: calls.append(("events", len(ev), details)) or ([], {}))
    monkeypatch.setattr(g, "_propagate", lambda Y, T, ns: calls.append(("plain", ns)) or (np.zeros((1, 1, 2)), np.zeros((1, 2), dtype=np.int32),
                                                                                          np.zeros(1, dtype=np.int32)))
    g.integrate_parallel([row], [1.0], [(x1, 0, 0)])
    g.integrate_parallel([row], [1.0], [(x1, 0, 0)], 4)
    g.integrate_parallel([row], [1.0], events=[(x1, 0, 0), (x1, 1, 1)], threads=2, details=True)
    g.integrate_parallel([row], [1.0], 4)
    g.integrate_parallel([row], [1.0], 4, True)
    g.integrate_parallel([row], [1.0])
    assert calls == [("events", 1, False), ("events", 1, False), ("events", 2, True), ("plain", 1), ("plain", 1), ("plain", 1)]
    with pytest.raises(TypeError, match="events given twice"):
        g.integrate_parallel([row], [1.0], [(x1, 0, 0)], events=[(x1, 0, 0)])


# ---- the host-side reader of a module's meta table, and the entry points an event module must not reach
def _rtc_parts(path):
    """(header lines up to the size line, code bytes) of a module file"""
    raw = open(path, "rb").read()
    lines, pos = [], 0
    for _ in range(2):
        e = raw.index(b"\n", pos)
        lines.append(raw[pos:e]), (pos := e + 1)
    for _ in range(int(lines[1])):
        e = raw.index(b"\n", pos)
        lines.append(raw[pos:e]), (pos := e + 1)
    e = raw.index(b"\n", pos)
    size = int(raw[pos:e])
    code = raw[e + 1:]
    assert len(code) == size
    return lines, code


def test_meta_reader_takes_a_whole_image_and_refuses_a_damaged_one(module, tmp_path):
    L = _lib.lib()
    path = _module_files(module, "events_0")[0]
    meta = (C.c_longlong * 64)()
    assert L.asset_hip_rtc_module_meta(path.encode(), meta, 64) == 42 and list(meta[:8]) == [4, 2, 1, 1, 0, 0, 5, 2]
    assert L.asset_hip_rtc_module_meta(path.encode(), meta, 8) == EINVAL and L.asset_hip_rtc_module_meta(None, meta, 64) == EINVAL
    assert L.asset_hip_rtc_module_meta(str(tmp_path / "none.rtc").encode(), meta, 64) == EINVAL
    home = _module_files(jit.ensure_kernel(make_vanderpol(), "LGL3", False, compile_only=True), "lgl3_0")[0]
    assert L.asset_hip_rtc_module_meta(home.encode(), meta, 64) == 42 and list(meta[:6]) == [1, 2, 1, 1, 2, 0]   # (any kind of module)
    lines, code = _rtc_parts(path)
    assert code[:4] == b"\x7fELF"

    def result(image):
        p = tmp_path / "damaged.rtc"
        p.write_bytes(b"\n".join(lines) + b"\n" + str(len(image)).encode() + b"\n" + image)
        out = (C.c_longlong * 64)(*([-7] * 64))
        rc = L.asset_hip_rtc_module_meta(str(p).encode(), out, 64)
        assert rc in (42, EINVAL) and (rc == 42 or all(v == -7 for v in out))
        return rc, list(out[:8])
    assert result(code) == (42, [4, 2, 1, 1, 0, 0, 5, 2])
    for cut in (1, 3, 4, 16, 63, 64, 65, 200, len(code) // 4, len(code) // 2, len(code) - 64, len(code) - 1):
        assert result(code[:cut])[0] == EINVAL, cut                                   # (the section headers lie at the image's end)
    assert result(b"\0" * 4096)[0] == EINVAL and result(b"x" * 8 + code[8:])[0] == EINVAL
    rng = np.random.default_rng(3)
    for field in (0x28, 0x3c, 0x3a, 0x3e):                                             # e_shoff, e_shnum, e_shentsize, e_shstrndx
        bad = bytearray(code)
        bad[field:field + 2] = b"\xff\xff"
        result(bytes(bad))                                                            # an error or the table, never a fault
    shoff = int.from_bytes(code[0x28:0x30], "little")
    for _ in range(40):                                                               # bytes of the section headers at random
        bad = bytearray(code)
        for k in rng.integers(shoff, len(code), 6):
            bad[k] = int(rng.integers(0, 256))
        result(bytes(bad))
    bad = code.replace(b"asset_rtc_meta\0", b"asset_rtc_mete\0")
    assert result(bad)[0] == EINVAL


def test_an_event_module_is_not_a_function(module):
    from asset_asrl_amd.evaluator import DefectEvaluator
    with pytest.raises(_lib.AssetHipError, match="an event module is launched through asset_hip_propagate_events"):
        DefectEvaluator(module, "Function", False, np.zeros((1, 5), dtype=np.int32), np.zeros((1, 2), dtype=np.int32), 5, 2, device=0)
    plan = _lib.LaunchPlan()
    assert _lib.lib().asset_hip_launch_plan_query(module.encode(), _lib.FUNCTION, 0, 0, 0, 1, 256, C.byref(plan)) == EINVAL
    assert "event module" in _lib.lib().asset_hip_last_error().decode()
