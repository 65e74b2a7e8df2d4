"""Per-entry check of the blocks of the plain per-application functions (csrc/func_kernels.h: mesh spacing, nodal spacing, control
spline, segment quadratures, user functions) against tests/golden/func_entries/<name>.npz (made by
tests/golden/make_golden_func_entries.py): the 50-digit value of EVERY entry of fx, jx, gx = J^T lam and hx = sum_k lam_k grad^2 f_k of
six applications of every function, and for every entry a running error bound E in units of u = 2^-53.  The fixtures have the keys of
tests/golden/defect_entries/, so the comparison itself is tests/defect_checker.py's ``check`` and the slot order its ``block_slots``;
here are the constants, the oracle's side and the product's DSL definitions of the functions.  Nothing under test is run here.

    bound(E, kind) = kappa_kind * u * E          an entry with E = 0 has no rounded term: it must be EXACTLY the stored value
                                                 (a structural zero must be 0.0)

The four kappa are measured, not chosen (``measure_constants``): the oracle is run over the whole fixture on the CPU -- the closed
forms of oracle/pathfuncs.cpp for spacing, spline and quadrature, both derivative providers (AD2 and the generated analytic code) for
the two user functions and the integrands --, the worst |oracle - ref| / (u E) per quantity is multiplied by 8 and rounded up to a
power of two.  The factor 8 is the project's (tests/defect_checker.py): the device functor is generated code with its own operation
order and FMA contraction.  The device's own results never enter.  The measured ratios and the constants are in every fixture's
metadata (``constants``) and in DESIGN.md section 2; tests/test_func_entries_cpu.py holds KAPPA below to them.
"""
from __future__ import annotations

import json
import os

import numpy as np

import defect_checker as dc
from defect_checker import KINDS, U, block_slots, pow2_ceil  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "func_entries")

# 8 x (worst oracle ratio), rounded up to a power of two -- see measure_constants() and the fixtures' metadata
KAPPA = {"fx": 4.0, "jx": 4.0, "gx": 4.0, "hx": 4.0}

LDS_BUDGET = 40 * 1024 - 64                # csrc/func_kernels.h: ASSET_FUNC_LDS_BUDGET


def stage_class(ir: int, orr: int) -> int:
    """csrc/func_kernels.h: FuncStage<F>::APW -- LD = NKKT | 1, the largest of 64, 32, 16, 8, 4 applications per workgroup whose rows fit
    the LDS budget, else 0 (direct stores)"""
    ld = (ir * (ir + 1) // 2 + orr * ir) | 1
    for apw in (64, 32, 16, 8, 4):
        if apw * ld * 8 <= LDS_BUDGET:
            return apw
    return 0


def all_names():
    return sorted(fn[:-4] for fn in os.listdir(DIR) if fn.endswith(".npz"))


_CACHE = {}


def load(name: str):
    """The fixture ``name``: dict of x[ns, IR], lam[ns, OR], fx[ns, OR], jx[ns, OR, IR], gx[ns, IR], hx[ns, IR (IR + 1) / 2] (lower
    triangle, row-major), the bounds fxE ... hxE, ac[ns, nconst] where the function reads constants, IR, OR, NKKT and meta.  Loaded
    once; read-only."""
    if name not in _CACHE:
        with np.load(os.path.join(DIR, name + ".npz")) as f:
            d = {k: f[k] for k in f.files}
        d["meta"] = json.loads(str(d["meta"]))
        d["name"] = name
        d["IR"], d["OR"] = d["x"].shape[1], d["lam"].shape[1]
        d["NKKT"] = d["IR"] * (d["IR"] + 1) // 2 + d["OR"] * d["IR"]
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = d
    return _CACHE[name]


def check(got, fixture, application_ids, kind, kappa=None):
    """defect_checker.check with the constants of this file"""
    return dc.check(got, fixture, application_ids, kind, kappa=KAPPA[kind] if kappa is None else kappa)


# --------------------------------------------------------------------------- the oracle's side
def providers(fixture):
    """[(provider id, name)]: the closed forms of oracle/pathfuncs.cpp have no derivative provider; the user functions and the
    quadratures (through their integrand) have two"""
    return ((0, "ad2"), (1, "generated")) if fixture["meta"]["kind"] in ("user", "lgl_integral") else ((0, "closed"),)


def oracle_blocks(ob, fixture, provider):
    """The oracle's (fx, jx, gx, hx lower triangle) of every fixture application, stacked as the fixture stacks them"""
    m = fixture["meta"]
    kind, a = m["kind"], m["args"]
    if kind == "lgl_mesh_spacing":
        fn = lambda s, x, l: ob.lgl_mesh_spacing_all(a["cs"], x, l)
    elif kind == "single_mesh_spacing":
        fn = lambda s, x, l: ob.single_mesh_spacing_all(float(fixture["ac"][s, 0]), x, l, scale=a["scale"])
    elif kind == "user":
        ode = ob.get_ode(a["oracle"], provider)
        fn = lambda s, x, l: ob.defect_all(ode, ob.MODES["Function"], x, l)
    elif kind == "lgl_integral":
        ode = ob.get_ode(a["integrand"], provider)
        fn = lambda s, x, l: ob.lgl_integral_all(ode, a["cs"], a["xv"], a["pv"], x, l)
    else:
        fn = lambda s, x, l: ob.control_spline_all(a["cs"], a["usize"], x, l, order=a["order"])
    il = np.tril_indices(fixture["IR"])
    out = [[], [], [], []]
    for s in range(fixture["x"].shape[0]):
        fx, jx, gx, hx = fn(s, fixture["x"][s], fixture["lam"][s])
        for o, v in zip(out, (fx, jx, gx, hx[il])):
            o.append(v)
    return dict(zip(KINDS, (np.stack(o) for o in out)))


def measure_constants():
    """dict(worst = {kind: {provider: worst |oracle - ref| / (u E) over every entry of every fixture}}, at, kappa = {kind: ...},
    inexact = entries with E = 0 the oracle does not reproduce exactly (must be 0), factor)."""
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import bindings as ob
    ob.build()
    worst = {k: {"closed": 0.0, "ad2": 0.0, "generated": 0.0} for k in KINDS}
    at = {k: None for k in KINDS}
    inexact = 0
    for name in all_names():
        f = load(name)
        ids = np.arange(f["x"].shape[0])
        for prov, pname in providers(f):
            got = oracle_blocks(ob, f, prov)
            for k in KINDS:
                r = check(got[k], f, ids, k, kappa=1.0)
                if not np.isfinite(r["worst"]):
                    inexact += int(np.sum((f[k + "E"] == 0) & (got[k].reshape(f[k].shape) != f[k])))
                    r = check(np.where(f[k + "E"] == 0, f[k], got[k].reshape(f[k].shape)), f, ids, k, kappa=1.0)
                if r["worst"] > worst[k][pname]:
                    worst[k][pname] = r["worst"]
                    if r["worst"] >= max(worst[k].values()):
                        at[k] = [name, pname, r["where"][0], r["where"][1]]
    kappa = {k: pow2_ceil(8.0 * max(worst[k].values())) for k in KINDS}
    return dict(worst=worst, at=at, kappa=kappa, inexact=inexact, factor=8.0)


# --------------------------------------------------------------------------- the product's own definitions
def product_function(fixture):
    """The function of a fixture in the product's DSL: (vf function, the name it is compiled under).  The name is what
    __graft_entry__.build() pre-compiles and what the GPU tests ask jit.ensure_function for."""
    from asset_asrl_amd import pathfuncs, vf
    m = fixture["meta"]
    kind, a, name = m["kind"], m["args"], "fe_" + fixture["name"]
    if kind == "lgl_mesh_spacing":
        return pathfuncs.LGLMeshSpacing(a["cs"]), name
    if kind == "single_mesh_spacing":
        return pathfuncs.SingleMeshSpacing(None, a["scale"]), name
    if kind == "control_spline":
        return pathfuncs.LGLControlSpline(a["cs"], a["usize"], a["order"]), name
    if kind == "user":
        if a["oracle"] == "pathcon":
            x0, x1, x2, t, u0, u1 = vf.Arguments(6).tolist()
            return vf.stack([x0 * x0 + x1 * u0 - vf.sin(x2), u0 * u0 + u1 * u1 - 1.0 + t * x0 * vf.exp(-1.0 * x1)]), name
        b = vf.Arguments(4)
        return vf.stack([b[0] * b[2] - b[1] * b[3] - 0.5]), name
    g = vf.Arguments(a["xv"] + a["pv"])
    y = [g.coeff(i) for i in range(a["xv"] + a["pv"])]
    integrand = {"integrand_quad2": lambda: y[1] * y[1] + y[0],
                 "integrand_powp": lambda: y[3] * y[0] * y[0] + vf.sin(y[1]) * y[2] + vf.exp(-1.0 * (y[0] * y[2])) / (1.0 + y[3] * y[3]),
                 "integrand_wide7": lambda: y[0] * y[1] * vf.sin(y[2]) + vf.exp(-0.5 * (y[3] * y[4])) * vf.sqrt(1.0 + y[5] * y[5])
                 + y[6] * y[6] * y[0] / (2.0 + y[1] * y[1])}[a["integrand"]]()
    return pathfuncs.LGLIntegral(integrand, a["cs"], a["xv"], a["pv"]), name


# tests/test_gpu_func_entries.py: seven members that cover the staging classes, each on a ragged mesh of its own, and an eighth with
# a single application (what the accumulation function of an integral parameter function is in real use); BUNDLE_MAX is 8
BUNDLE_MEMBERS = ("lgl_mesh_spacing4", "single_mesh_spacing_ac", "lgl_integral4_quad2", "control_spline4_2", "control_spline4_3",
                  "control_spline4_4", "control_spline4_5", "pairwise")


def prebuild_device_functions(jit):
    """Every fixture's function and the two bundles of tests/test_gpu_func_entries.py, compiled into the module cache
    (__graft_entry__.build())"""
    dev = {n: jit.ensure_function(*product_function(load(n))) for n in all_names()}
    members = [dev[n] for n in BUNDLE_MEMBERS]
    jit.ensure_bundle(members)
    jit.ensure_bundle(members[::-1])
    return dev
