"""Everything about the propagation with events AND the state-transition matrix that needs no device: the restatement of
tests/event_stm_checker.py against the closed-form variational flows (test infrastructure only), the launch plan of a module of kind 6,
what such a module holds, the kinds of the kernel slots, the input errors of asset_hip_propagate_events_stm -- all found before the
device is touched, against a module that is registered without one --, the arena layout of the call, and the argument errors of
``integrate_events_stm*``."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import event_checker as eck
import event_stm_cases as cases
import event_stm_checker as sck
import propagate_checker as pck
from asset_asrl_amd import _lib, jit

EINVAL, ENOODE, ENODEV = -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSED_CASES = [n for n in eck.case_names() if eck.fixture()[1][n]["system"] in sck.CLOSED]


# ---- the restatement against the closed forms
def test_the_closed_forms_are_the_variational_flows():
    """d / d [x0, p] of event_checker.exact_flow by central differences in longdouble, at a time that is not a round number"""
    LD = sck.LD
    for system, row in (("oscillator", [0.7, -0.4, 0.3]), ("freefall", [3.0, 1.5, -0.2, 9.81])):
        n, t = 2, LD("1.734")
        S = sck.closed_S(system, row, t)
        cols = list(range(n)) + list(range(n + 1, len(row)))
        assert S.shape == (n, len(cols)) and S.dtype == LD
        for c, k in enumerate(cols):
            d = LD("1e-7")
            hi, lo = np.array(row, dtype=LD), np.array(row, dtype=LD)
            hi[k] += d
            lo[k] -= d
            fd = (eck.exact_flow(system, hi, t) - eck.exact_flow(system, lo, t)) / (2 * d)
            assert np.abs(fd - S[:, c]).max() < 1e-11, (system, k)       # (both flows are at most quadratic or trigonometric: d^2 / 6)
        assert np.array_equal(sck.closed_S(system, row, LD(row[2]))[:, :n], np.eye(n))


@pytest.mark.parametrize("name", CLOSED_CASES)
def test_restatement_meets_the_closed_forms_within_a_quarter_of_the_bounds(name):
    case = eck.fixture()[1][name]
    n = eck.SYSTEMS[case["system"]]["n"]
    eS, res = sck.eS_closed(case)
    plain = eck.restate_case(case)
    B = eck.state_bounds(case, case["accepted64"])
    worst = 0.0
    for i, (r, p) in enumerate(zip(res, plain)):
        # the state side of the restatement with columns is event_checker's own machine, bit for bit
        assert r["steps"] == p["steps"] and r["count"] == p["count"] and r["stopped"] == p["stopped"] and r["t_end"] == p["t_end"]
        assert np.array_equal(r["x"], p["x"])
        for lj, pj in zip(r["locs"], p["locs"]):
            assert len(lj) == len(pj) and all(np.array_equal(a["x"], b["x"]) and a["t"] == b["t"] for a, b in zip(lj, pj))
        items = sck.items_of(r)
        assert len(items) == 1 + sum(min(c, case["max_locs"]) for c in r["count"])
        for k, (t, x, Sm) in enumerate(items):
            ref = sck.closed_S(case["system"], case["rows"][i], sck.LD(float(t)))
            bound = pck.stm_bound(ref.astype(float)[None], eS[i:i + 1]) / 4.0
            worst = max(worst, pck.compare(np.asarray(Sm)[None], ref[None], bound, f"{name} problem {i} item {k}: S, a quarter of the bound"))
            xref = eck.exact_flow(case["system"], case["rows"][i], sck.LD(float(t)))
            pck.compare(np.asarray(x)[None], xref[None], B[i][None] / 4.0, f"{name} problem {i} item {k}: state at the returned time")
    assert (eS > 0).all() and (eS < 1.0e-8).all(), eS          # (AbsTol 1e-12 and sensitivities of order one: eS is of the tolerance's order)
    print(f"{name}: eS = {eS}, worst ratio {worst:.3g}")


def test_restatement_of_a_problem_that_does_not_move_and_of_one_that_fails():
    sysd = eck.SYSTEMS["freefall"]
    opt = eck.gck.options(def_step=0.1, max_step=0.5)
    r = sck.propagate_events_stm(sysd["f"], sck.jacobian_of("freefall"), [sysd["events"]["height"][0]], [1.0, 0.0, 2.0, 9.81], 2.0, [0], [1], opt)
    assert r["status"] == 0 and r["steps"] == (0, 0) and r["count"] == [0]
    assert np.array_equal(r["S"], [[1, 0, 0], [0, 1, 0]]), "tf == t0: the identity in the x columns, zero elsewhere"
    r = sck.propagate_events_stm(sysd["f"], sck.jacobian_of("freefall"), [sysd["events"]["height"][0]], [10.0, 0.0, 0.0, 9.81], 3.0, [0], [0],
                                 dict(opt, max_steps=3))
    assert r["status"] == 1 and np.isnan(r["S"]).all() and np.isnan(r["x"]).all()


# ---- the module
@pytest.fixture(scope="module")
def module():
    """vanderpol with two events, kind 6 (pre-built: event_stm_cases.MODULES), registered WITHOUT a device"""
    mp = pytest.MonkeyPatch()
    mp.delenv("ASSET_HIP_JIT", raising=False)
    try:
        yield jit.ensure_event_stm_module(cases.make_ode("vanderpol"), [cases.event_function("vanderpol", "x1"),
                                                                        cases.event_function("vanderpol", "pos")], compile_only=False)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def module4():
    """the same ODE and events as a module of kind 4"""
    mp = pytest.MonkeyPatch()
    mp.delenv("ASSET_HIP_JIT", raising=False)
    try:
        yield jit.ensure_event_module(cases.make_ode("vanderpol"), [cases.event_function("vanderpol", "x1"),
                                                                    cases.event_function("vanderpol", "pos")], compile_only=False)
    finally:
        mp.undo()


def _plan(module, m):
    out = (C.c_longlong * 7)(*([-7] * 7))
    rc = _lib.lib().asset_hip_propagate_events_stm_plan(module.encode() if module else None, m, out)
    return rc, dict(zip(("group", "lanes", "passes", "problems_per_wg", "lds_bytes", "grid", "columns"), [int(v) for v in out]))


@pytest.mark.parametrize("system,names,want", [("vanderpol", ("x1", "pos"), dict(group=4, lanes=64, passes=1, problems_per_wg=16)),
                                                ("twobody_lt", ("rv",), dict(group=16, lanes=64, passes=1, problems_per_wg=4)),
                                                ("shape_11_4_2", ("x0c",), dict(group=32, lanes=32, passes=1, problems_per_wg=1)),
                                                ("synthetic32", ("x0c",), dict(group=8, lanes=8, passes=4, problems_per_wg=1))])
def test_the_plan_of_a_kind_6_launch_is_that_of_the_stm_kernel(monkeypatch, system, names, want):
    monkeypatch.delenv("ASSET_HIP_JIT", raising=False)
    ode = cases.make_ode(system)
    mod = jit.ensure_event_stm_module(ode, [cases.event_function(system, e) for e in names], compile_only=False)
    for m in (1, 5, 64, 65, 1000):
        rc, plan = _plan(mod, m)
        assert rc == 0 and plan == _lib.propagate_plan(ode.XVars(), ode.UVars(), ode.PVars(), m, True), (system, m)
        assert {k: plan[k] for k in want} == want and plan["columns"] == ode.XVars() + ode.UVars() + ode.PVars()
    assert _plan(mod, 0)[0] == EINVAL and _plan(None, 1)[0] == EINVAL and _plan("no_such_module", 1)[0] == ENOODE


def test_the_plan_query_refuses_a_module_of_kind_4(module4):
    rc, plan = _plan(module4, 3)
    assert rc == ENOODE and all(v == -7 for v in plan.values())


def _module_files(name, tag):
    return glob.glob(os.path.join(jit.JIT_DIR, name, f"module_{tag}_*.rtc"))


def _module_names(name, tag):
    mods = _module_files(name, tag)
    assert len(mods) == 1, mods
    head = open(mods[0], "rb").read(1 << 16).split(b"\n")
    return head[2:2 + int(head[1])]


def test_a_kind_6_module_names_exactly_the_two_new_kernels(module, module4):
    names = _module_names(module, "eventstm_0")
    assert len(names) == 2 and sorted(b"prop_event_stm_kernel" in ln for ln in names) == [False, True]
    assert sorted(b"prop_event_jac_kernel" in ln for ln in names) == [False, True]
    assert all(jit.device_name(cases.make_ode("vanderpol")).encode() in ln and module.encode() in ln for ln in names)
    L = _lib.lib()
    meta = (C.c_longlong * 64)()
    assert L.asset_hip_rtc_module_meta(_module_files(module, "eventstm_0")[0].encode(), meta, 64) == 42
    assert list(meta[:8]) == [6, 2, 1, 1, 0, 0, 5, 2], "kind 6, the ODE's sizes, its input count, ne"
    # the module of kind 4 of the same ODE and events keeps exactly its one kernel, under another name
    names4 = _module_names(module4, "events_0")
    assert module4 != module and len(names4) == 1 and b"prop_event_kernel" in names4[0]
    v = [C.c_int32(-1) for _ in range(4)]
    assert L.asset_hip_event_module_sizes(module.encode(), *[C.byref(x) for x in v]) == 0 and [x.value for x in v] == [2, 1, 1, 2]
    # the same mathematics under fresh objects is the same module
    from asset_asrl_amd import vf
    from helpers import make_vanderpol
    a = vf.Arguments(5)
    assert jit.ensure_event_stm_module(make_vanderpol(), [a[1] * 1.0, a[0] * a[0] + 1.0], compile_only=True) == module


def test_slot_kinds():
    L = _lib.lib()
    slots, s = {}, 0
    while L.asset_hip_kernel_slot_name(s) is not None:
        slots[L.asset_hip_kernel_slot_name(s).decode()] = s
        s += 1
    kinds = lambda k: L.asset_hip_kernel_slot_kinds(slots[k])
    assert kinds("K_PROP_EVENT_STM") == 32 and kinds("K_PROP_EVENT_JAC") == 32                   # (bit 5: modules of kind 6 only)
    assert kinds("K_PROP_EVENT") == 8 and all(kinds(k) == 16 for k in ("K_PROP_CTRL_BATCH", "K_PROP_CTRL_STM", "K_PROP_CTRL_JAC"))
    assert all(kinds(k) == 1 for k in ("K_PROP_BATCH", "K_PROP_STM", "K_PROP_JAC"))
    assert sum(1 for k in slots if kinds(k) & 32) == 2 and sum(1 for k in slots if kinds(k) & 8) == 1


# ---- the C entry point's input errors
def _opts(**kw):
    d = dict(def_step=0.01, min_step=1e-6, max_step=100.0, max_step_change=3.0, adaptive=1, max_steps=100000)
    d.update(kw)
    return _lib.IntegOptions(d["def_step"], d["min_step"], d["max_step"], d["max_step_change"], d["adaptive"], d["max_steps"], None, None)


def _call(module, name="", m=3, ne=2, direction=(0, 1), stop=(0, 2), tol=1.0e-6, iters=10, locs=4, opt=None, tf_edit=None, null=()):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    mm, K = max(m, 1), max(locs, 1)
    y0 = np.random.default_rng(5).uniform(0.5, 1.0, (mm, 5))
    tf = y0[:, 2] + 0.1
    if tf_edit is not None:
        tf[1] = tf_edit
    d, s = np.array(direction, dtype=np.int32), np.array(stop, dtype=np.int32)
    outs = dict(xf=np.full(mm * 2, -7.0), jac=np.full(mm * 2 * 6, -7.0), t_end=np.full(mm, -7.0), stopped=np.full(mm, -7, dtype=np.int32),
                ev_count=np.full(mm * 2, -7, dtype=np.int32), ev_rows=np.full(mm * 2 * K * 3, -7.0), ev_resid=np.full(mm * 2 * K, -7.0),
                ev_conv=np.full(mm * 2 * K, -7, dtype=np.int32), ev_jac=np.full(mm * 2 * K * 2 * 6, -7.0),
                steps=np.full(mm * 2, -7, dtype=np.int32), status=np.full(mm, -7, dtype=np.int32))
    a = {k: v.ctypes.data_as(dp if v.dtype == np.float64 else ip) for k, v in outs.items()}
    a.update(y0=y0.ctypes.data_as(dp), tf=tf.ctypes.data_as(dp), direction=d.ctypes.data_as(ip), stop=s.ctypes.data_as(ip))
    for k in ((null,) if isinstance(null, str) else null):
        a[k] = None
    name = module if name == "" else name
    L = _lib.lib()
    rc = L.asset_hip_propagate_events_stm(name.encode() if name else None, a["y0"], m, a["tf"], C.byref(opt) if opt is not None else None, ne,
                                          a["direction"], a["stop"], tol, iters, locs, a["xf"], a["jac"], a["t_end"], a["stopped"],
                                          a["ev_count"], a["ev_rows"], a["ev_resid"], a["ev_conv"], a["ev_jac"], a["steps"], a["status"], 0)
    return rc, L.asset_hip_last_error().decode(errors="replace"), outs


INPUT_ERRORS = [("a null module name", dict(name=None), EINVAL, "null")] + \
    [(f"null {k}", dict(null=k), EINVAL, "null") for k in ("y0", "tf", "direction", "stop", "xf", "jac", "t_end", "stopped", "ev_count", "ev_rows",
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
    ("a negative event_tol", dict(tol=-1.0e-6), EINVAL, "event_tol"),
    ("a NaN event_tol", dict(tol=float("nan")), EINVAL, "event_tol"),
    ("no evaluation", dict(iters=0), EINVAL, "max_event_iters"),
    ("no stored occurrence", dict(locs=0, stop=(0, 0)), EINVAL, "max_locs"),
    ("a NaN final time", dict(tf_edit=np.nan), EINVAL, "not finite (problem 1)"),
    ("an infinite final time", dict(tf_edit=np.inf), EINVAL, "not finite (problem 1)"),
    ("a zero default step", dict(opt=dict(def_step=0.0, min_step=0.0)), EINVAL, "positive"),
    ("min > def", dict(opt=dict(min_step=0.1)), EINVAL, "min <= def <= max"),
    ("max_steps 0", dict(opt=dict(max_steps=0)), EINVAL, "max_steps"),
]


@pytest.mark.parametrize("what,change,code,word", INPUT_ERRORS, ids=[e[0] for e in INPUT_ERRORS])
def test_input_errors_are_statuses_with_a_message_and_nothing_is_written(module, what, change, code, word):
    kw = dict(change)
    if "opt" in kw:
        kw["opt"] = _opts(**kw["opt"])
    rc, msg, out = _call(module, **kw)
    assert rc == code and word in msg, (what, rc, msg)
    assert all(np.all(o == -7) for o in out.values()), what


def test_each_entry_refuses_the_other_kind_of_event_module(module, module4):
    rc, msg, out = _call(module, name=module4)
    assert rc == ENOODE and "kind 4" in msg and module4 in msg and all(np.all(o == -7) for o in out.values())
    # the entry without the STM refuses a module of kind 6 the same way
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    y0, tf = np.full((1, 5), 0.5), np.array([0.6])
    d, s = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    fo = [np.full(16, -7.0) for _ in range(4)]
    io = [np.full(16, -7, dtype=np.int32) for _ in range(5)]
    L = _lib.lib()
    rc = L.asset_hip_propagate_events(module.encode(), y0.ctypes.data_as(dp), 1, tf.ctypes.data_as(dp), None, 2, d.ctypes.data_as(ip),
                                      s.ctypes.data_as(ip), 1.0e-6, 10, 2, fo[0].ctypes.data_as(dp), fo[1].ctypes.data_as(dp),
                                      io[0].ctypes.data_as(ip), io[1].ctypes.data_as(ip), fo[2].ctypes.data_as(dp), fo[3].ctypes.data_as(dp),
                                      io[2].ctypes.data_as(ip), io[3].ctypes.data_as(ip), io[4].ctypes.data_as(ip), 0)
    assert rc == ENOODE and "kind 6" in L.asset_hip_last_error().decode() and all(np.all(o == -7) for o in fo + io)


@pytest.mark.parametrize("null", [(), ("ev_jac",), ("ev_jac", "steps", "status")], ids=["full", "no ev_jac", "no ev_jac, steps, status"])
def test_valid_input_gets_as_far_as_the_device(module, null):
    rc, msg, out = _call(module, opt=_opts(), null=null)
    given = [o for k, o in out.items() if k not in null]
    if os.path.exists("/dev/kfd"):
        assert rc == 0, msg
        assert not any(np.all(o == -7) for o in given) and all(np.all(out[k] == -7) for k in null)
    else:
        assert rc == ENODEV and "no HIP device visible" in msg and all(np.all(o == -7) for o in out.values())


def test_a_kind_6_module_is_not_a_function(module):
    from asset_asrl_amd.evaluator import DefectEvaluator
    with pytest.raises(_lib.AssetHipError, match="an event module is launched through asset_hip_propagate_events_stm"):
        DefectEvaluator(module, "Function", False, np.zeros((1, 5), dtype=np.int32), np.zeros((1, 2), dtype=np.int32), 5, 2, device=0)
    plan = _lib.LaunchPlan()
    assert _lib.lib().asset_hip_launch_plan_query(module.encode(), _lib.FUNCTION, 0, 0, 0, 1, 256, C.byref(plan)) == EINVAL
    assert "event module" in _lib.lib().asset_hip_last_error().decode()


# ---- the arena layout of the call
_ARENA = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "capi/arena.h"
using asset_hip::Arena;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
template <class T>
struct Layout {
  Arena<T> a;
  std::vector<size_t> off, cnt;
  void take(T** dest, size_t count) { off.push_back(a.take(dest, count)), cnt.push_back(count); }
  size_t tiled() const {
    size_t at = 0;
    for (size_t k = 0; k < off.size(); k++) {
      CHECK(off[k] == at);
      at += cnt[k];
    }
    CHECK(at == a.total() && !a.overflowed());
    return at;
  }
};
int main() {
  // asset_hip_propagate_events_stm: y0 | tf | abs | rel | xf | t_end | ev_rows | ev_resid | S | jac | (ev_jac wanted: ev_S | ev_jac);
  // steps | status | stopped | ev_count | ev_conv   (include/asset_hip.h: the array shapes)
  const size_t n = 5, uv = 2, pv = 1, N = n + 1 + uv + pv, C = N - 1, m = 3, ne = 2, locs = 3, occ = m * ne * locs;
  for (int want = 0; want < 2; want++) {
    Layout<double> d;
    Layout<int> i;
    double *S = nullptr, *jac = nullptr, *ev_S = nullptr, *ev_jac = nullptr, *head = nullptr;
    for (size_t c : {m * N, m, n, n, m * n, m, occ * (n + 1), occ}) d.take(&head, c);
    d.take(&S, m * n * C), d.take(&jac, m * n * (N + 1));
    d.take(want ? &ev_S : nullptr, want ? occ * n * C : 0), d.take(want ? &ev_jac : nullptr, want ? occ * n * (N + 1) : 0);
    int* ih = nullptr;
    for (size_t c : {m * 2, m, m, m * ne, occ}) i.take(&ih, c);
    const size_t base = m * N + m + 2 * n + m * n + m + occ * (n + 2) + m * n * (C + N + 1);
    CHECK(d.tiled() == base + (want ? occ * n * (C + N + 1) : 0) && i.tiled() == m * 4 + m * ne + occ);
    std::vector<double> mem(d.a.total());
    d.a.bind(mem.data());
    CHECK(S == mem.data() + (base - m * n * (C + N + 1)) && jac == S + m * n * C);
    if (want) CHECK(ev_S == jac + m * n * (N + 1) && ev_jac == ev_S + occ * n * C && ev_jac + occ * n * (N + 1) == mem.data() + mem.size());
    else CHECK(ev_S == nullptr && ev_jac == nullptr && jac + m * n * (N + 1) == mem.data() + mem.size());   // (not allocated, and the kernels see null)
  }
  std::printf("ok\n");
  return 0;
}
"""


def test_arena_layout_of_the_call_with_and_without_ev_jac(tmp_path):
    src, exe = tmp_path / "arena.cpp", tmp_path / "arena"
    src.write_text(_ARENA)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "asset_asrl_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
    # the entry point takes its arrays in that order (capi.hip: propagate_events_impl)
    text = open(os.path.join(ROOT, "asset_asrl_amd", "csrc", "capi.hip")).read()
    body = text[text.index("int propagate_events_impl("):]
    body = body[:body.index("c.allocate()")]
    order = [body.index(k) for k in ("problems_take(c, a", "&a.xf", "&a.t_end", "&a.ev_rows", "&a.ev_resid", "&a.S,", "&a.jac,", "&a.ev_S :",
                                     "&a.ev_jac :", "&a.stopped", "&a.ev_count", "&a.ev_conv")]
    assert order == sorted(order)


# ---- ode.integrator
def test_argument_errors_of_the_new_methods(monkeypatch):
    from asset_asrl_amd import vf
    ode = cases.make_ode("vanderpol")
    g = ode.integrator(0.1)
    row, x1 = [1.0, 0.0, 0.0, 0.1, 1.0], cases.event_function("vanderpol", "x1")
    monkeypatch.setattr(jit, "ensure_event_stm_module", lambda *a, **k: pytest.fail("a module was asked for"))
    with pytest.raises(ValueError, match="has 3 inputs, the ODE's rows have 5"):
        g.integrate_events_stm(row, 1.0, [(vf.Arguments(3)[0] * 1.0, 0, 0)])
    with pytest.raises(ValueError, match="not a scalar"):
        g.integrate_events_stm(row, 1.0, [(vf.stack([x1, x1]), 0, 0)])
    for bad, word in (([(x1, 2, 0)], "direction"), ([(x1, 0, -1)], "stop count"), ([(x1, 0, 9)], "MaxEventLocs"), ([], "1..8 events"),
                      ([(x1, 0, 0)] * 9, "1..8 events"), ([(x1, 0)], r"\(g, direction, stop\)"), ([(x1, 0.5, 0)], "direction")):
        with pytest.raises(ValueError, match=word):
            g.integrate_events_stm_parallel([row], [1.0], bad)
    with pytest.raises(ValueError, match="needs events"):
        g.integrate_events_stm_parallel([row], [1.0], None)
    with pytest.raises(ValueError, match="5 columns"):
        g.integrate_events_stm_parallel([row[:4]], [1.0], [(x1, 0, 0)])
    with pytest.raises(ValueError, match="1 initial rows but 2 final times"):
        g.integrate_events_stm_parallel([row], [1.0, 2.0], [(x1, 0, 0)])
    g.EventTol = 0.0
    with pytest.raises(ValueError, match="EventTol"):
        g.integrate_events_stm(row, 1.0, [(x1, 0, 0)])


def test_one_module_per_event_list_and_the_constant_controller_is_taken(monkeypatch):
    ode = cases.make_ode("vanderpol")
    x1 = cases.event_function("vanderpol", "x1")
    seen = []
    monkeypatch.setattr(jit, "ensure_event_stm_module", lambda o, f, compile_only=None: seen.append(list(f)) or "the_module")
    monkeypatch.setattr(jit, "ensure_event_module", lambda *a, **k: pytest.fail("the module of kind 4 was asked for"))

    def entry(*a):
        seen.append((a[0], np.ctypeslib.as_array(a[1], (5,)).copy(), bool(a[19])))
        return ENODEV
    monkeypatch.setattr(_lib.lib(), "asset_hip_propagate_events_stm", entry, raising=False)
    g = ode.integrator(0.1, 0.75)                                                          # the constant controller: the held-control path
    for kw in (dict(), dict(event_jacs=True), dict(details=True)):
        with pytest.raises(_lib.AssetHipError):
            g.integrate_events_stm([1.0, 0.0, 0.0, 0.1, 1.0], 1.0, [(x1, 0, 1)], **kw)
    assert seen[0] == [x1] and [s[0] for s in seen[1:]] == [b"the_module"] * 3, "one module, asked for once"
    assert all(s[1].tolist() == [1.0, 0.0, 0.0, 0.75, 1.0] for s in seen[1:]), "the controller's value in the control column"
    assert [s[2] for s in seen[1:]] == [False, True, False], "ev_jac is passed only when it is asked for"


def test_a_control_law_is_refused_and_the_events_keyword_of_the_stm_calls_still_raises():
    import controller_cases as cc
    ode = cc.make_ode("vanderpol")
    ucon, varlocs = cc.law("vdp_fb")
    g = ode.integrator(0.1, ucon, varlocs)
    row, ev = [1.0, 0.0, 0.0, 0.1, 1.0], [(cases.event_function("vanderpol", "x1"), 0, 0)]
    for call in (lambda: g.integrate_events_stm(row, 1.0, ev), lambda: g.integrate_events_stm_parallel([row], [1.0], ev, event_jacs=True)):
        with pytest.raises(NotImplementedError, match="events with a controller"):
            call()
    h = cases.make_ode("vanderpol").integrator(0.1)
    for call in (lambda: h.integrate_stm(row, 1.0, events=ev), lambda: h.integrate_stm_parallel([row], [1.0], events=ev),
                 lambda: h.integrate_dense(row, 1.0, 5, events=ev), lambda: h.integrate_dense_parallel([row], [1.0], 5, events=ev)):
        with pytest.raises(NotImplementedError, match="with events is not implemented"):
            call()
