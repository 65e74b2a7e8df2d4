"""The ODEs and event functions of the tests of the propagation with events AND the state-transition matrix
(tests/test_propagate_events_stm_cpu.py, tests/test_gpu_propagate_events_stm.py, and the pre-build of __graft_entry__.build()): those of
tests/event_cases.py, and the 32-state library ODE of the STM tests with one event (lane groups of 8, four column passes)."""
from __future__ import annotations

import functools

import event_cases

SYNTH_LEVEL = 0.0         # the event of synthetic32: x0 - SYNTH_LEVEL

# (system, event names): every module of kind 6 the tests use
MODULES = (("oscillator", ("x0",)), ("freefall", ("height",)), ("twobody_lt", ("rv",)), ("twobody_lt", ("pos",)), ("vanderpol", ("x1",)),
           ("vanderpol", ("pos",)), ("vanderpol", ("x1", "pos")), ("shape_11_4_2", ("x0c",)), ("synthetic32", ("x0c",)),
           ("twobody_lt", ("rv", "rv")))
# modules of kind 4 the tests compare with that tests/event_cases.py does not list
MODULES_KIND4 = (("synthetic32", ("x0c",)), ("twobody_lt", ("rv", "rv")))


@functools.lru_cache(maxsize=None)
def make_ode(system: str):
    if system == "synthetic32":
        from asset_asrl_amd.ode import ODE_LIBRARY
        return ODE_LIBRARY["synthetic32"]()
    return event_cases.make_ode(system)


@functools.lru_cache(maxsize=None)
def event_function(system: str, event: str):
    if system == "synthetic32":
        from asset_asrl_amd import vf
        assert event == "x0c"
        return vf.Arguments(33)[0] - SYNTH_LEVEL
    return event_cases.event_function(system, event)


def events_of(system: str, names, direction, stop):
    """The list of (g, direction, stop) ``integrate_events_stm_parallel`` takes."""
    return [(event_function(system, e), int(d), int(s)) for e, d, s in zip(names, direction, stop)]


def prebuild(jit):
    for system, names in MODULES:
        jit.ensure_event_stm_module(make_ode(system), [event_function(system, e) for e in names])
    for system, names in MODULES_KIND4:
        jit.ensure_event_module(make_ode(system), [event_function(system, e) for e in names])
