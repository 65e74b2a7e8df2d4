"""Which error comes back when an integrating entry point of the C ABI is given TWO wrong inputs: the first failing check wins, in the
order include/asset_hip.h's entry points have always had -- null arguments, m, ns, the entry lookup, what only events check (ne,
event_tol, max_event_iters, max_locs, then per event direction / stop), the options in the order of their own rules, the final
times, the launch plan, the device.  The tests of the single errors (test_propagate_cpu.py, test_propagate_controller_cpu.py,
test_propagate_events_cpu.py, test_integ_cpu.py) pin every text alone; their callers are used here with two changes at once.  No
device is touched and no output byte is written."""
import numpy as np
import pytest

import controller_cases as cc
import event_cases
import interp_checker as ick
import test_integ_cpu as t_integ
import test_propagate_controller_cpu as t_ctrl
import test_propagate_cpu as t_prop
import test_propagate_events_cpu as t_events
from asset_asrl_amd import _lib, jit

EINVAL, ENOODE = -1, -2
BAD_STEP, BAD_ORDER, BAD_CHANGE, BAD_STEPS = dict(def_step=0.0, min_step=0.0), dict(min_step=0.1), dict(max_step_change=0.0), dict(max_steps=0)


def _check(rc, msg, out, code, word, unless=()):
    assert rc == code and word in msg and not any(w in msg for w in unless), (rc, msg)
    assert all(np.all(o == -7) for o in out)


def _with_opts(change, opts):
    kw = dict(change)
    if "opt" in kw:
        kw["opt"] = opts(**kw["opt"])
    return kw


# (two changes, the code and a word of the text that wins, words of the text that loses)
PROPAGATE = [
    ("null rows before m", dict(null="y0", m=0), EINVAL, "null", ("m must",)),
    ("m before ns", dict(m=0, ns=0), EINVAL, "m must be", ()),
    ("m before the name", dict(m=0, ode="no_such_ode"), EINVAL, "m must be", ("no_such_ode",)),
    ("ns before the name", dict(ns=0, ode="no_such_ode"), EINVAL, "ns must be", ("no_such_ode",)),
    ("the name before the options", dict(ode="no_such_ode", opt=BAD_STEP), ENOODE, "no_such_ode", ("positive",)),
    ("the options before the final times", dict(opt=BAD_STEPS, tf_edit=np.nan), EINVAL, "max_steps", ("finite",)),
    ("positive steps before their order", dict(opt=dict(def_step=0.0, min_step=0.1)), EINVAL, "positive", ("<=",)),
    ("the steps' order before max_step_change", dict(opt=dict(min_step=0.1, max_step_change=0.0)), EINVAL, "min <= def <= max", ("change",)),
    ("max_step_change before max_steps", dict(opt=dict(max_step_change=0.0, max_steps=0)), EINVAL, "max_step_change", ("max_steps",)),
    ("the final times before the device", dict(tf_edit=np.inf), EINVAL, "not finite (problem 1)", ("device",)),
]


PROPAGATE_BOTH = [(stm, *e) for stm in (False, True) for e in PROPAGATE if not (stm and "ns" in e[1])]   # (asset_hip_propagate_stm has no ns)


@pytest.mark.parametrize("stm,what,change,code,word,unless", PROPAGATE_BOTH, ids=[("stm: " if e[0] else "") + e[1] for e in PROPAGATE_BOTH])
def test_propagate_reports_the_first_failing_check(stm, what, change, code, word, unless):
    _check(*t_prop._call(stm, **_with_opts(change, t_prop._opts)), code, word, unless)


@pytest.fixture(scope="module")
def ctrl_module():
    mp = pytest.MonkeyPatch()
    mp.delenv("ASSET_HIP_JIT", raising=False)
    try:
        yield jit.ensure_controller_module(cc.make_ode("vanderpol"), *cc.law("vdp_fb"), compile_only=False)
    finally:
        mp.undo()


CONTROLLER = [
    ("xf_last before everything", dict(entry="lanes", null="last", m=0, name="no_such_module"), EINVAL, "null", ("m must", "no_such")),
    ("null controls before m", dict(null="us", m=0), EINVAL, "null", ("m must",)),
    ("m before ns", dict(m=0, ns=0), EINVAL, "m must be", ()),
    ("ns before the name", dict(ns=0, name="no_such_module"), EINVAL, "ns must be", ("no_such",)),
    ("m before the name (stm)", dict(entry="stm", m=0, name="reentry"), EINVAL, "m must be", ("reentry",)),
    ("an unknown name before the options", dict(name="no_such_module", opt=BAD_ORDER), ENOODE, "no controller module registered", ("<=",)),
    ("another kind of name before the options", dict(entry="stm", name="reentry", opt=BAD_CHANGE), ENOODE, "is not a controller module", ("change",)),
    ("the options before the final times", dict(entry="lanes", opt=BAD_STEP, tf_edit=np.nan), EINVAL, "positive", ("finite",)),
    ("the final times before the device", dict(entry="stm", tf_edit=np.nan), EINVAL, "not finite (problem 1)", ("device",)),
]


@pytest.mark.parametrize("what,change,code,word,unless", CONTROLLER, ids=[e[0] for e in CONTROLLER])
def test_controller_propagation_reports_the_first_failing_check(ctrl_module, what, change, code, word, unless):
    _check(*t_ctrl._call(ctrl_module, **_with_opts(change, t_ctrl._opts)), code, word, unless)


@pytest.fixture(scope="module")
def event_module():
    mp = pytest.MonkeyPatch()
    mp.delenv("ASSET_HIP_JIT", raising=False)
    try:
        yield jit.ensure_event_module(event_cases.make_ode("vanderpol"), [event_cases.event_function("vanderpol", "x1"),
                                                                          event_cases.event_function("vanderpol", "pos")], compile_only=False)
    finally:
        mp.undo()


EVENTS = [
    ("null directions before m", dict(null="direction", m=0), EINVAL, "null", ("m must",)),
    ("m before the name", dict(m=0, name="no_such_module"), EINVAL, "m must be", ("no_such",)),
    ("the name before ne", dict(name="reentry", ne=1, direction=(0,), stop=(0,)), ENOODE, "reentry", ("events",)),
    ("ne before event_tol", dict(ne=1, tol=0.0), EINVAL, "the module has 2 events", ("event_tol",)),
    ("event_tol before max_event_iters", dict(tol=0.0, iters=0), EINVAL, "event_tol", ("iters",)),
    ("max_event_iters before max_locs", dict(iters=0, locs=0, stop=(0, 0)), EINVAL, "max_event_iters", ("max_locs",)),
    ("max_locs before the directions", dict(locs=0, stop=(0, 0), direction=(2, 0)), EINVAL, "max_locs must be", ("direction",)),
    ("an event's direction before its stop", dict(direction=(0, 2), stop=(0, -1)), EINVAL, "direction must be -1, 0 or 1 (event 1)", ("stop",)),
    ("event 0 before event 1", dict(direction=(0, 2), stop=(-1, 0)), EINVAL, "stop must not be negative (event 0)", ("direction",)),
    ("a negative stop before one beyond max_locs", dict(stop=(-1, 5)), EINVAL, "stop must not be negative (event 0)", ("exceeds",)),
    ("the directions before the options", dict(direction=(0, 2), opt=BAD_STEP), EINVAL, "direction must be", ("positive",)),
    ("stop beyond max_locs before the options", dict(stop=(5, 0), opt=BAD_STEPS), EINVAL, "stop exceeds max_locs", ("max_steps",)),
    ("the options before the final times", dict(opt=BAD_ORDER, tf_edit=np.nan), EINVAL, "min <= def <= max", ("finite",)),
    ("the final times before the device", dict(tf_edit=np.nan), EINVAL, "not finite (problem 1)", ("device",)),
]


@pytest.mark.parametrize("what,change,code,word,unless", EVENTS, ids=[e[0] for e in EVENTS])
def test_event_propagation_reports_the_first_failing_check(event_module, what, change, code, word, unless):
    _check(*t_events._call(event_module, **_with_opts(change, t_events._opts)), code, word, unless)


ESTIMATOR = [
    ("the name before the node count", dict(ode="no_such_ode", nnodes=12), ENOODE, "no_such_ode", ("nb*",)),
    ("the node count before the times", dict(nnodes=12, edit=(4, 3)), EINVAL, "nb*(cs-1)+1", ("duplicate",)),
    ("the earlier node's time error", dict(edit=(4, 2), edit2=(9, 8)), EINVAL, "not monotonic (node 3)", ("duplicate",)),
    ("the times before the options", dict(edit=(4, 3), opt=BAD_STEP), EINVAL, "duplicate times (node 3)", ("positive",)),
    ("the options in their order", dict(opt=dict(max_step=0.001, max_steps=0)), EINVAL, "min <= def <= max", ("max_steps",)),
]


@pytest.mark.parametrize("what,change,code,word,unless", ESTIMATOR, ids=[e[0] for e in ESTIMATOR])
def test_integrator_estimator_reports_the_first_failing_check(what, change, code, word, unless):
    traj = ick.ragged_traj("reentry", "LGL7", 4, seed=3, T=1.0)                       # 13 nodes, times in column 5
    for key in ("edit", "edit2"):
        if key in change:
            traj[change[key][0], 5] = traj[change[key][1], 5]
    _check(*t_integ._call(change.get("ode", "reentry"), _lib.MODES["LGL7"], 0, traj, change.get("nnodes", 13),
                          t_integ._opts(**change["opt"]) if "opt" in change else None), code, word, unless)
