"""Generate tests/golden/func_entries/<name>.npz: every entry of the blocks (fx, jx, gx = J^T lam, hx = sum_k lam_k grad^2 f_k) of six
applications of the plain per-application functions of a phase -- mesh spacing, nodal spacing with a per-application constant, the
control spline, segment quadratures, two user functions -- as 50-digit values, each with a running error bound E of its own.  The
same kind of fixture as tests/golden/defect_entries/ (same keys: x, lam, fx ... hx as the lower triangle by rows, fxE ... hxE in float32
rounded upward, meta; ``ac[ns, nconst]`` where the function reads constants of its applications), so tests/defect_checker.py's
``check`` and ``block_slots`` read it as they read that one.

Nothing is restated here that exists: the value formulas are those of make_golden_pathfuncs.py (``single_mesh_spacing``,
``lgl_mesh_spacing``, ``control_spline``, ``lgl_integral``, the integrands), the AD scalar with running errors is
make_golden_defect_entries.py's ``DE`` / ``ME`` (its rules are in that file's docstring), the weights are those of lgl_tables.json.
Nothing of asset_asrl_amd.vf is imported.  New here: the two user functions of tests/test_gpu_function.py and the integrand

    I7(y) = y0 y1 sin(y2) + exp(-0.5 y3 y4) sqrt(1 + y5^2) + y6^2 y0 / (2 + y1^2)

which couples every input with another one, so the node blocks of the quadrature's Hessian are dense.

The functions are chosen by the staging class of csrc/func_kernels.h they reach (``FuncStage<F>::APW``, applications per workgroup:
the largest of 64, 32, 16, 8, 4 with APW (NKKT | 1) 8 <= 40 KiB - 64, else 0 = direct stores): see ``FUNCTIONS`` and ``stage_class``.

Applications, as the defect fixture chooses its segments: three plain ones; one whose segment widths are 1e-4 of a plain one's
(spline entries up to 1 / h^3 ~ 1e12 beside O(1) ones); one with reversed time (h < 0); one whose multipliers span 1e-6 ... 1e3 in
magnitude with two of them exactly 0.0 (with one or two outputs the ends of the span stay and none is zero).  Node times sit off the
exact LGL spacing, as make_golden_pathfuncs.nodes places them.  The two user functions have no segment width: their "narrow"
application has inputs of 1e-4 of a plain draw, their "reversed" one the negated draw.

No input had to be excluded: were one to be (cancellation that a first-order E cannot model), the rule would read the reference's own
plain-double error only, as make_golden_vf.golden_case redraws.

The files are written by make_golden_vf.write_npz (fixed time stamp), and a plain run keeps the measured constants a file already
holds, so it reproduces the committed files bit for bit.

Usage:  python tests/golden/make_golden_func_entries.py --jobs 8 [name ...]
        python tests/golden/make_golden_func_entries.py --constants      (measure the oracle, write kappa into the metadata)
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_pathfuncs as pf  # noqa: E402
from make_golden_defect_entries import DE, ME, NARROW, PLAIN, REVERSED, WIDELAM, blocks_of  # noqa: E402
from make_golden_vf import write_npz  # noqa: E402

mp.mp.dps = 50
OUT = os.path.join(HERE, "func_entries")
FLAGS = (PLAIN, PLAIN, PLAIN, NARROW, REVERSED, WIDELAM)
LDS_BUDGET = 40 * 1024 - 64


def stage_class(ir: int, orr: int) -> int:
    """FuncStage<F>::APW of csrc/func_kernels.h, restated: applications per workgroup of the staged block kinds (0: direct stores)"""
    ld = (ir * (ir + 1) // 2 + orr * ir) | 1
    return next((a for a in (64, 32, 16, 8, 4) if a * ld * 8 <= LDS_BUDGET), 0)


# --------------------------------------------------------------------------- the value formulas that are new here
def pathcon(z, M):
    x0, x1, x2, t, u0, u1 = z
    return [x0 * x0 + x1 * u0 - M.sin(x2), u0 * u0 + u1 * u1 - 1.0 + t * x0 * M.exp(-x1)]


def pairwise(z, M):
    return [z[0] * z[2] - z[1] * z[3] - 0.5]


def integrand_wide7(y, M):
    return y[0] * y[1] * M.sin(y[2]) + M.exp(-0.5 * (y[3] * y[4])) * M.sqrt(1.0 + y[5] * y[5]) + y[6] * y[6] * y[0] / (2.0 + y[1] * y[1])


INTEGRANDS = {"integrand_quad2": pf.integrand_quad2, "integrand_powp": pf.integrand_powp, "integrand_wide7": integrand_wide7}
USER = {"pathcon": pathcon, "pairprod": pairwise}

# name -> (kind, args, IR, OR, staging class).  kind / args are what tests/func_checker.py reads from the metadata to call the oracle
# and to build the product's DSL definition.
FUNCTIONS = {
    "lgl_mesh_spacing3": ("lgl_mesh_spacing", dict(cs=3), 3, 1, 64),
    "lgl_mesh_spacing4": ("lgl_mesh_spacing", dict(cs=4), 4, 2, 64),
    "single_mesh_spacing_ac": ("single_mesh_spacing", dict(scale=1.0), 3, 1, 64),
    "pathcon": ("user", dict(oracle="pathcon"), 6, 2, 64),
    "pairwise": ("user", dict(oracle="pairprod"), 4, 1, 64),
    "lgl_integral2_powp": ("lgl_integral", dict(cs=2, xv=3, pv=1, integrand="integrand_powp"), 9, 1, 64),
    "lgl_integral3_powp": ("lgl_integral", dict(cs=3, xv=3, pv=1, integrand="integrand_powp"), 13, 1, 32),
    "lgl_integral4_quad2": ("lgl_integral", dict(cs=4, xv=2, pv=0, integrand="integrand_quad2"), 12, 1, 32),
    "control_spline3_2": ("control_spline", dict(cs=3, usize=2, order=1), 15, 2, 32),
    "control_spline4_2": ("control_spline", dict(cs=4, usize=2, order=2), 21, 4, 16),
    "control_spline4_2_o1": ("control_spline", dict(cs=4, usize=2, order=1), 21, 2, 16),
    "control_spline4_3": ("control_spline", dict(cs=4, usize=3, order=2), 28, 6, 8),
    "lgl_integral4_wide7": ("lgl_integral", dict(cs=4, xv=7, pv=0, integrand="integrand_wide7"), 32, 1, 8),
    "control_spline4_4": ("control_spline", dict(cs=4, usize=4, order=2), 35, 8, 4),
    "control_spline4_5": ("control_spline", dict(cs=4, usize=5, order=2), 42, 10, 0),
}


def seed_of(name: str) -> int:
    return 20261000 + 10 * list(FUNCTIONS).index(name)


# --------------------------------------------------------------------------- inputs
def _times(rng, cs, two, flags):
    t = pf.nodes(rng, cs, two)
    if flags & NARROW:
        t = t[0] + 1e-4 * (t - t[0])
    if flags & REVERSED:
        t = t[-1] - (t - t[0])
    return t


def application_inputs(name: str, k: int):
    """(z[IR], lam[OR], ac[nconst] or None) of fixture application k: float64, what every code under test is given"""
    kind, a, IR, OR, _ = FUNCTIONS[name]
    flags = FLAGS[k]
    rng = np.random.default_rng(seed_of(name) + k)
    ac = None
    if kind == "lgl_mesh_spacing":
        z = _times(rng, a["cs"], False, flags)
    elif kind == "single_mesh_spacing":
        t = _times(rng, 4, False, flags)
        j = 1 + int(rng.integers(0, 2))
        z = t[[0, j, 3]]
        ac = np.array([float(pf.TAB["4"]["CardinalSpacings"][j]) + rng.uniform(-0.05, 0.05)])      # a different s per application
    elif kind == "user":
        z = rng.uniform(-1.5, 1.5, IR)
        if flags & NARROW:
            z = 1e-4 * z
        if flags & REVERSED:
            z = -z
    elif kind == "lgl_integral":
        cs, xv, pv = a["cs"], a["xv"], a["pv"]
        t = _times(rng, cs, False, flags)
        z = np.concatenate([np.column_stack([rng.uniform(-1, 1, (cs, xv)), t]).ravel(), rng.uniform(0.5, 1.5, pv)])
    else:
        t = _times(rng, a["cs"], True, flags)
        z = np.column_stack([t] + [rng.uniform(-1, 1, t.size) for _ in range(a["usize"])]).ravel()
    assert z.size == IR
    lam = rng.uniform(-2, 2, OR)
    if flags & WIDELAM:
        lam = np.where(rng.uniform(size=OR) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6.0, 3.0, OR)
        lam[0], lam[-1] = 1e-6, -1e3                                   # the span is there whatever the draw
        if OR > 2:
            lam[rng.choice(np.arange(1, OR - 1), size=min(2, OR - 2), replace=False)] = 0.0
    return z, lam, ac


def value(name: str, z, ac):
    """The outputs of the function over inputs ``z`` (a list of DE)"""
    kind, a, _, _, _ = FUNCTIONS[name]
    if kind == "lgl_mesh_spacing":
        return pf.lgl_mesh_spacing(z, a["cs"])
    if kind == "single_mesh_spacing":
        return pf.single_mesh_spacing(z, float(ac[0]), a["scale"])
    if kind == "user":
        return USER[a["oracle"]](z, ME)
    if kind == "lgl_integral":
        integrand = INTEGRANDS[a["integrand"]]
        return pf.lgl_integral(z, a["cs"], a["xv"], a["pv"], lambda y, _m: integrand(y, ME))    # (lgl_integral passes make_golden's MP)
    return pf.control_spline(z, a["cs"], a["usize"], a["order"])


def compute_application(name: str, k: int):
    z, lam, ac = application_inputs(name, k)
    d = value(name, [DE.var(mp.mpf(float(v)), i, z.size) for i, v in enumerate(z)], ac)
    out = blocks_of(d, z, lam)
    if ac is not None:
        out["ac"] = ac
    return out


def path_of(name: str) -> str:
    return os.path.join(OUT, name + ".npz")


def stored_constants():
    """The measured constants the committed files hold (None before --constants has run once)"""
    for name in FUNCTIONS:
        if os.path.exists(path_of(name)):
            with np.load(path_of(name)) as f:
                c = json.loads(str(f["meta"])).get("constants")
            if c:
                return c
    return None


def file_bytes(name: str, apps, constants) -> bytes:
    kind, a, IR, OR, cls = FUNCTIONS[name]
    assert cls == stage_class(IR, OR) and apps[0]["x"].shape == (IR,) and apps[0]["lam"].shape == (OR,)
    meta = dict(generator="tests/golden/make_golden_func_entries.py", dps=mp.mp.dps, function=name, kind=kind, args=a, IR=IR, OR=OR,
                NKKT=IR * (IR + 1) // 2 + OR * IR, stage_class=cls, flags=list(FLAGS), seeds=[seed_of(name) + k for k in range(len(FLAGS))],
                constants=constants)
    data = {k: np.stack([s[k] for s in apps]) for k in apps[0]}
    data["meta"] = np.array(json.dumps(meta))
    buf = io.BytesIO()
    write_npz(buf, data)
    return buf.getvalue()


def _task(args):
    return args, compute_application(*args)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4, help="worker processes")
    ap.add_argument("--constants", action="store_true", help="measure the oracle against the fixtures, write kappa into every file")
    ap.add_argument("only", nargs="*", help="fixture names (default: all)")
    a = ap.parse_args(argv)
    if a.constants:
        return write_constants()
    names = [n for n in FUNCTIONS if not a.only or n in a.only]
    tasks = sorted(((n, k) for n in names for k in range(len(FLAGS))), key=lambda t: -FUNCTIONS[t[0]][2])     # the wide ones first
    constants = stored_constants()
    import multiprocessing
    done = {n: {} for n in names}
    os.makedirs(OUT, exist_ok=True)
    with multiprocessing.get_context("fork").Pool(a.jobs) as pool:
        for (n, k), app in pool.imap_unordered(_task, tasks):
            done[n][k] = app
            if len(done[n]) == len(FLAGS):
                with open(path_of(n), "wb") as f:
                    f.write(file_bytes(n, [done[n][j] for j in range(len(FLAGS))], constants))
                print("wrote", n, os.path.getsize(path_of(n)), flush=True)
    return 0


def write_constants():
    """The four kappa of tests/func_checker.py, measured on the oracle (never on the device), into every file."""
    sys.path.insert(0, os.path.dirname(HERE))
    import func_checker as fc
    constants = fc.measure_constants()
    for name in FUNCTIONS:
        with np.load(path_of(name)) as f:
            data = {k: f[k] for k in f.files}
        meta = json.loads(str(data["meta"]))
        meta["constants"] = constants
        data["meta"] = np.array(json.dumps(meta))
        write_npz(path_of(name), data)
    print(json.dumps(constants, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
