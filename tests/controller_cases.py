"""The ODEs and control laws of the controller tests, through the DSL (tests/test_propagate_controller_cpu.py,
tests/test_gpu_propagate_controller.py, and the pre-build of __graft_entry__.build()).  tests/controller_checker.py: LAWS holds the same
laws and their Jacobians as numpy callbacks, written independently of these."""
from __future__ import annotations

import functools

# law name -> (system, varlocs): every controller module the tests use.  The ODE input row is [x, t, u, p].
LAWS = {
    "pd": ("pd", [0, 1, 4]),                        # u = -p0 x0 - 0.4 x1
    "pd_nan": ("pd", [0, 1, 4]),                    # u = -sqrt(p0) x0 - 0.4 x1: NaN for a negative p0
    "vdp_fb": ("vanderpol", [1, 2]),                # u = -0.5 tanh(x1) cos t
    "vdp_pass": ("vanderpol", [4]),                 # u = mu, the row's parameter
    "tangential": ("twobody_lt", [3, 4, 5]),        # u = 0.01 v / |v|
    "shape_5_3_2": ("shape_5_3_2", [0, 5, 9]),      # the shape law of x0, t and p0 (below)
    "shape_8_3_1": ("shape_8_3_1", [0, 8, 12]),
    "shape_11_4_0": ("shape_11_4_0", [0, 11]),      # ... without a parameter
    "coupled16": ("coupled16", [0, 16, 20]),
}


@functools.lru_cache(maxsize=None)
def make_ode(system: str):
    from asset_asrl_amd import vf
    from asset_asrl_amd.ode import ODEArguments, ODEBase
    if system == "pd":
        class DoubleIntegrator(ODEBase):
            def __init__(self):
                a = ODEArguments(2, 1, 1)
                x0, x1 = a.XVec().tolist()
                super().__init__(vf.stack([x1, a.UVar(0) + 0.0 * x0 + 0.0 * a.PVar(0)]), 2, 1, 1, name="pd")
        return DoubleIntegrator()
    if system == "twobody_lt":
        from asset_asrl_amd.workloads import TwoBody
        return TwoBody()
    if system == "vanderpol":
        from helpers import make_vanderpol
        return make_vanderpol()
    if system == "coupled16":
        from helpers import make_coupled
        return make_coupled(16)
    if system.startswith("shape_"):
        from helpers import make_shape
        return make_shape(*(int(v) for v in system.split("_")[1:]))
    raise KeyError(system)


@functools.lru_cache(maxsize=None)
def law(name: str):
    """(ucon, varlocs): the vf function of ``len(varlocs)`` inputs and the entries of the ODE's input row it reads."""
    from asset_asrl_amd import vf
    system, varlocs = LAWS[name]
    a = vf.Arguments(len(varlocs))
    if name == "pd":
        u = -1.0 * (a[2] * a[0]) - 0.4 * a[1]
    elif name == "pd_nan":
        u = -1.0 * (vf.sqrt(a[2]) * a[0]) - 0.4 * a[1]
    elif name == "vdp_fb":
        u = -0.5 * (vf.tanh(a[0]) * vf.cos(a[1]))
    elif name == "vdp_pass":
        u = a[0]
    elif name == "tangential":
        u = a.normalized() * 0.01
    else:
        uv = make_ode(system).UVars()
        z, t = a[0], a[1]
        outs = []
        for k in range(uv):
            v = 0.3 * vf.sin(z + 0.5 * k) + 0.2 * vf.cos((k + 1.0) * t)
            if len(varlocs) == 3:
                v = v + (0.1 * (k + 1)) * (a[2] * z)
            outs.append(v)
        u = vf.stack(outs)
    return u, list(varlocs)


def integrator(name: str, def_step, method=None):
    ucon, varlocs = law(name)
    ode = make_ode(LAWS[name][0])
    return ode.integrator(def_step, ucon, varlocs) if method is None else ode.integrator(method, def_step, ucon, varlocs)


def prebuild(jit):
    for name, (system, _) in LAWS.items():
        jit.ensure_controller_module(make_ode(system), *law(name))
