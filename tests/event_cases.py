"""The ODEs and event functions of the event tests, through the DSL (tests/test_propagate_events_cpu.py, tests/test_gpu_propagate_events.py,
and the pre-build of __graft_entry__.build()).  tests/event_checker.py: SYSTEMS holds the same right-hand sides and events as numpy
callbacks, written independently of these."""
from __future__ import annotations

import functools

SHAPE_LEVEL = 0.25

# (system, event names): every event module the tests use
MODULES = (("oscillator", ("x0",)), ("oscillator", ("x0", "x0m", "x1")), ("freefall", ("height",)), ("twobody_lt", ("rv",)),
           ("twobody_lt", ("pos",)), ("vanderpol", ("x1",)), ("vanderpol", ("pos",)), ("vanderpol", ("x1", "pos")), ("shape_11_4_2", ("x0c",)))


@functools.lru_cache(maxsize=None)
def make_ode(system: str):
    from asset_asrl_amd import vf
    from asset_asrl_amd.ode import ODEArguments, ODEBase
    if system == "oscillator":
        class Oscillator(ODEBase):
            def __init__(self):
                a = ODEArguments(2, 0, 0)
                x0, x1 = a.XVec().tolist()
                super().__init__(vf.stack([x1, -1.0 * x0]), 2, 0, 0, name="oscillator")
        return Oscillator()
    if system == "freefall":
        class FreeFall(ODEBase):
            def __init__(self):
                a = ODEArguments(2, 0, 1)
                h, v = a.XVec().tolist()
                super().__init__(vf.stack([v, -1.0 * a.PVar(0) + 0.0 * h]), 2, 0, 1, name="freefall")
        return FreeFall()
    if system == "twobody_lt":
        from asset_asrl_amd.workloads import TwoBody
        return TwoBody()
    if system == "vanderpol":
        from helpers import make_vanderpol
        return make_vanderpol()
    if system == "shape_11_4_2":
        from helpers import make_shape
        return make_shape(11, 4, 2)
    raise KeyError(system)


@functools.lru_cache(maxsize=None)
def event_function(system: str, event: str):
    """The scalar vf function of the ODE's input row [x, t, u, p]."""
    from asset_asrl_amd import vf
    ode = make_ode(system)
    a = vf.Arguments(ode.XVars() + 1 + ode.UVars() + ode.PVars())
    table = {
        ("oscillator", "x0"): lambda: a[0] * 1.0,
        ("oscillator", "x0m"): lambda: a[0] - 0.01,
        ("oscillator", "x1"): lambda: a[1] * 1.0,
        ("freefall", "height"): lambda: a[0] * 1.0,
        ("twobody_lt", "rv"): lambda: a[0] * a[3] + a[1] * a[4] + a[2] * a[5],
        ("twobody_lt", "pos"): lambda: a[0] * a[0] + a[1] * a[1] + a[2] * a[2],
        ("vanderpol", "x1"): lambda: a[1] * 1.0,
        ("vanderpol", "pos"): lambda: a[0] * a[0] + 1.0,
        ("shape_11_4_2", "x0c"): lambda: a[0] - SHAPE_LEVEL,
    }
    return table[(system, event)]()


def events_of(system: str, names, direction, stop):
    """The list of (g, direction, stop) ``integrate_parallel`` takes."""
    return [(event_function(system, e), int(d), int(s)) for e, d, s in zip(names, direction, stop)]


def prebuild(jit):
    for system, names in MODULES:
        jit.ensure_event_module(make_ode(system), [event_function(system, e) for e in names])
